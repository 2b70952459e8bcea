"""Per-(node, type) products over the compact pair tables of graph.SidePairs: Y[r] = H[node[r]] @ W_{type(r)}."""
import torch

from .. import _lib
from ..config import settings as _cfg
from ..dense import (GEMM_NN, GEMM_NT, GEMM_TN, limb_dense_sel, limb_gemm_tn_tiles, limb_shape_ok, limb_tn_tiles_supported, panel_gemm,
                     sel_image)
from ..weight_grad_stream import fork
from .segment import _check_f32, _seg_reduce_raw


class _TypedLinear(torch.autograd.Function):
    """Y[r] = H[node[r]] @ W_{type(r)} for the compact rows of one graph.SidePairs.

    The table is a batch of [chunk, Din] tiles, each of ONE edge type (type blocks are padded to the tile size), so the
    L per-type transforms are ONE batched GEMM with the weight picked per tile; the dense path computes
    H @ [W_0|..|W_{L-1}] for ALL V*L (node,type) rows instead.  Backward: dX = dY W^T (batched), per-tile partial
    weight gradients X^T dY (batched) summed per type by the gather-reduce kernel, and the per-row dX summed back into
    their nodes over the node -> rows CSR (ascending type order); no atomics anywhere."""

    @staticmethod
    def forward(ctx, H, side, *weights):
        V, Din = H.shape
        Dout = weights[0].shape[1]
        c = side.chunk
        Hz = torch.cat([H, H.new_zeros((1, Din))])                            # row V = the padding rows' input
        X = Hz.index_select(0, side.node)                                     # [P, Din]
        Wt = torch.stack(weights).index_select(0, side.chunk_type)            # [tiles, Din, Dout]
        Y = torch.bmm(X.view(-1, c, Din), Wt).view(side.P, Dout)
        ctx.side, ctx.num_nodes, ctx.shape = side, V, (len(weights), Din, Dout)
        ctx.save_for_backward(X, Wt)
        return Y

    @staticmethod
    def backward(ctx, gY):
        X, Wt = ctx.saved_tensors
        side, c = ctx.side, ctx.side.chunk
        L, Din, Dout = ctx.shape
        gY = gY.contiguous()
        gH = None
        if ctx.needs_input_grad[0]:
            gX = torch.bmm(gY.view(-1, c, Dout), Wt.transpose(1, 2)).view(side.P, Din)
            gH = _seg_reduce_raw(_lib.AGG_SUM, gX, side.node_rowptr, 1, side.node_col, None, ctx.num_nodes)
        gW = [None] * L
        if any(ctx.needs_input_grad[2:]):
            part = torch.bmm(X.view(-1, c, Din).transpose(1, 2), gY.view(-1, c, Dout))   # [tiles, Din, Dout]
            g = _sum_tiles_per_type(part, side, L)
            gW = [g[l] if ctx.needs_input_grad[2 + l] else None for l in range(L)]
        return (gH, None, *gW)


def _sum_tiles_per_type(part, side, L: int):
    """[L, Din, Dout] from the per-tile partials part [tiles, Din, Dout] (every tile of ONE edge type), summed in tile order: by the
    gather-reduce kernel over pieces of `sub` floats where the matrix splits into them, else (odd shapes) by per-type sums."""
    _, Din, Dout = part.shape
    n = Din * Dout
    sub = 1024 if n % 1024 == 0 else (n if n <= 1024 and n % 4 == 0 else 0)
    if not sub:
        return torch.stack([tiles.sum(0) for tiles in part.split(side.chunk_counts)])
    K = n // sub
    rowptr, col = side.weight_grad_plan(K)
    return _seg_reduce_raw(_lib.AGG_SUM, part.view(-1, sub), rowptr, 1, col, None, L * K).view(L, Din, Dout)


def _typed_weight_gradient(H, gY, side, L: int, Din: int, Dout: int):
    """[L, Din, Dout]: per-tile partials gather(H)^T @ gY (one launch), summed per edge type in tile order."""
    node32, _ = side.panel_indices()
    tiles = side.P // side.chunk
    if ((_cfg.typed_tn == "limb" or (_cfg.typed_tn == "auto" and Dout % 256 == 0))
            and limb_tn_tiles_supported(H, gY, node32, side.chunk)):
        # (round 5, isolated at a C5-sized table of 1400 tiles: three-limb TN 405 us vs exact-fp32 panel TN 484 us for
        #  [128, 256] partials, 325 vs 262 us for [128, 128] ones — the panel kernel runs near the fp32 matrix pipe's rate;
        #  the 0.6 / 0.96 ms per launch of the round-4 traces were contention on the side stream, not the kernel)
        part = limb_gemm_tn_tiles(H, gY, node32, side.chunk)                 # [tiles, Din, Dout]
    else:
        part = panel_gemm(GEMM_TN, H, gY, a_rows=node32, batch=tiles, strides=(0, side.chunk * Dout, Din * Dout),
                          dims=(Din, Dout, side.chunk))                      # [tiles, Din, Dout]
    return _sum_tiles_per_type(part, side, L)


def _typed_product(H, side, weights):
    """(Y [P, Dout], W): Y = gather(H) @ W_type over the pair table `side`, one launch.  The limb images of the per-type weights come
    from the step's cache where they can (round 6, dense.weight_image(separate=True): neither a stacked [L, Din, Dout] copy nor a
    split launch in front of the product) and W is None; else W is the stacked copy the product read — split into the scratch limbs,
    or on the exact-fp32 panel kernel — for the backward to keep."""
    Din, Dout = weights[0].shape
    node32, tile_type = side.panel_indices()
    im = sel_image(weights, GEMM_NN) if (_typed_limb_ok(Din, Dout) and _typed_limb_ok(Dout, Din)) else None
    if im is not None:
        return limb_dense_sel(GEMM_NN, H, weights, a_rows=node32, num_rows=side.P, b_select=tile_type,
                              rows_per_select=side.chunk, image=im), None
    W = torch.stack(weights)
    if _typed_limb_ok(Din, Dout):
        return limb_dense_sel(GEMM_NN, H, W, a_rows=node32, num_rows=side.P, b_select=tile_type, rows_per_select=side.chunk), W
    return panel_gemm(GEMM_NN, H, W, a_rows=node32, num_rows=side.P, b_select=tile_type, rows_per_select=side.chunk), W


def _typed_input_gradient(gY, side, weights, W, out=None):
    """dX [P, Din] = dY @ W_type^T per row of the pair table `side`, one launch, into `out` when given.  `weights`: the per-type
    kernels when the forward read their cached images (W is None), else W is the forward's stacked copy."""
    Din, Dout = (weights[0] if W is None else W[0]).shape
    _, tile_type = side.panel_indices()
    if W is None:
        im = sel_image(weights, GEMM_NT)
        if im is not None:
            return limb_dense_sel(GEMM_NT, gY, weights, b_select=tile_type, rows_per_select=side.chunk, image=im, out=out)
        W = torch.stack(weights)                                 # (switched off between forward and backward)
    if _typed_limb_ok(Dout, Din):
        gX = limb_dense_sel(GEMM_NT, gY, W, b_select=tile_type, rows_per_select=side.chunk)
    else:
        gX = panel_gemm(GEMM_NT, gY, W, b_select=tile_type, rows_per_select=side.chunk, dims=(side.P, Din, Dout))
    return gX if out is None else out.copy_(gX)


class _TypedLinearPanel(torch.autograd.Function):
    """_TypedLinear on the row-panel MFMA kernels, for one pair table or several over the same node states H: the gather H[node[r]]
    and the per-tile kernel selection happen in the kernel's load addresses.  Nothing [P, Din] (the gathered rows) and nothing
    [tiles, Din, Dout] (a per-tile copy of the kernels) is materialised, forward or backward.  Per table:
      forward   Y  = gather(H) @ W_type            one launch (NN, gathered rows, per-tile B)
      backward  dX = dY @ W_type^T                 one launch (NT with the kernels as stored)
                dW = per-tile gather(H)^T @ dY     one launch (TN, gathered reduction rows, one product per tile), the per-tile
                                                   partials summed per type by the gather-reduce kernel (tile order)
    and ONE gather-reduce sums the stacked dX rows of all tables into the nodes over `node_csr` (ascending type order).  The two
    per-(node, type) transforms of a GNN-FiLM layer (gnns/gnn_film.py:92-106: messages h_u W_l over the by-source table, FiLM
    weights h_v F_l over the by-target one) are one node over graph.PairTables.node_csr_both instead of two reductions and an
    addition of their [V, D] results (round 6: one launch and ~0.1 ms less per layer of the C5 step).
      tables    ((side, L), ..): graph.SidePairs and how many of *weights, in order, are its per-type kernels
      node_csr  () -> (rowptr, col): the node -> rows CSR over the tables' rows one behind the other
      leaves    the weights themselves, when every one is a leaf parameter"""

    @staticmethod
    def forward(ctx, H, tables, node_csr, leaves, *weights):
        ctx.leaf_params, ctx.node_csr = leaves, node_csr
        outs, kept, saved, at = [], [], [H], 0
        for side, L in tables:
            ws = weights[at:at + L]
            at += L
            Y, W = _typed_product(H, side, ws)
            outs.append(Y)
            # the per-type kernels where the product read their cached images (W is None), else the stacked copy it read
            kept.append((side, (L, *ws[0].shape), W is None, L if W is None else 1))
            saved.extend(ws if W is None else (W,))
        ctx.tables = kept
        ctx.save_for_backward(*saved)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gYs):
        H, *saved = ctx.saved_tensors
        gYs = [g.contiguous() for g in gYs]
        need = ctx.needs_input_grad[4:]
        want_w = any(need)

        def weight_side():
            flat = sum((_typed_weight_gradient(H, g, side, *shape).unbind(0) for (side, shape, _, _), g in zip(ctx.tables, gYs)), ())
            return tuple(g if n else None for g, n in zip(flat, need))

        # The weight gradients (exact-fp32 matrix pipe, ~0.25-0.5 ms per product on a 23-type batch) depend on nothing the input
        # gradient computes: they run on the side stream of the aggregate-first layer's weight gradient, under the memory-bound
        # kernels that follow on the main stream (the row sums, the next layer's fused edge backward); the join is deferred behind
        # the whole backward inside train_step (weight_grad_stream.deferred_weight_gradient_join).
        aside = fork(weight_side, (H, *gYs), ctx.leaf_params, want=want_w and ctx.needs_input_grad[0],
                     join_in_backward=True, contributes=want_w)
        gH = None
        if ctx.needs_input_grad[0]:
            # (one table: its rows need no stacking, the product's own output is reduced)
            stacked = None if len(gYs) == 1 else torch.empty((sum(t[0].P for t in ctx.tables), H.shape[1]), dtype=torch.float32,
                                                             device=H.device)
            at = row = 0
            for (side, _, cached, count), g in zip(ctx.tables, gYs):
                kept = saved[at:at + count]
                out = None if stacked is None else stacked[row:row + side.P]
                gX = _typed_input_gradient(g, side, kept if cached else None, None if cached else kept[0], out=out)
                at, row = at + count, row + side.P
            rowptr, col = ctx.node_csr()
            gH = _seg_reduce_raw(_lib.AGG_SUM, gX if stacked is None else stacked, rowptr, 1, col, None, H.shape[0])
        gWs = aside.join() if aside is not None else (weight_side() if want_w else (None,) * len(need))
        return (gH, None, None, None) + gWs


def _typed_panel(H, tables, node_csr):
    """_TypedLinearPanel over tables ((side, weights), ..): one [P, Dout] table each."""
    allw = [w for _, ws in tables for w in ws]
    leaves = tuple(allw) if all(w.is_leaf and w.requires_grad for w in allw) else None
    return _TypedLinearPanel.apply(H, tuple((side, len(ws)) for side, ws in tables), node_csr, leaves, *allw)


def typed_linear_pair(H, pairs, weights_src, weights_tgt):
    """(typed_linear(H, pairs.src, weights_src), typed_linear(H, pairs.tgt, weights_tgt)) with ONE reduction of both input
    gradients into the nodes (one _TypedLinearPanel over both tables) where the cached limb route applies; else the two separate
    calls."""
    weights_src, weights_tgt = list(weights_src), list(weights_tgt)
    _check_f32(H, "H")
    H = H.contiguous()
    ok = (_typed_panel_ok(H, pairs.src, weights_src) and _typed_panel_ok(H, pairs.tgt, weights_tgt)
          and weights_src[0].shape[0] == weights_tgt[0].shape[0])
    if ok:
        for ws in (weights_src, weights_tgt):
            Din, Dout = ws[0].shape
            ok = ok and _typed_limb_ok(Din, Dout) and _typed_limb_ok(Dout, Din) and sel_image(ws, GEMM_NN) is not None \
                and sel_image(ws, GEMM_NT) is not None
    if not ok:
        return typed_linear(H, pairs.src, weights_src), typed_linear(H, pairs.tgt, weights_tgt)
    return _typed_panel(H, ((pairs.src, weights_src), (pairs.tgt, weights_tgt)), pairs.node_csr_both)


def _typed_limb_ok(k: int, n: int) -> bool:
    """The limb route (relgnn_limb_dense_sel_f32) for a typed product with reduction length k and n output columns."""
    return _cfg.limb_gemm and limb_shape_ok(None, n, k, 128)          # (rows: gathered per (node, type), any number)


def _typed_panel_ok(H, side, weights) -> bool:
    Din, Dout = weights[0].shape
    # (forward: N = Dout; input gradient: N = Din; both must be panel widths)
    return (_cfg.typed == "panel" and H.is_cuda and side.chunk == 512 and Din % 64 == 0
            and Dout % 64 == 0 and side.P > 0 and H.data_ptr() % 16 == 0)


def typed_linear(H, side, weights):
    """[P, Dout] table over the non-empty (node,type) buckets of `side` (graph.SidePairs); weights: L x [Din, Dout]."""
    _check_f32(H, "H")
    H = H.contiguous()
    if _typed_panel_ok(H, side, weights):
        return _typed_panel(H, ((side, list(weights)),), lambda: (side.node_rowptr, side.node_col))[0]
    return _TypedLinear.apply(H, side, *weights)

