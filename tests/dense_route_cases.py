"""The route table of dense.py: which librelgnn entry points a node-side product ends on, case by case.

`cases(dev)` is the list; `record(dev)` runs every case behind a recording proxy of the loaded library handle and returns
{case name: {"calls": [...], "queries": [...], "raises": ...}}.  tests/test_gpu_dense_routes.py compares that with
tests/golden/dense_routes.json.  Run as a script,

    python tests/dense_route_cases.py record tests/golden/dense_routes.json     # the fixture (recorded before dense.py's routing
                                                                                 # was gathered into one decision function)
    python tests/dense_route_cases.py dump DIR                                   # every case's output tensor(s) as DIR/<case>.npy

it uses public names of the package only.  "calls" are the launches in order; "queries" (entry points that launch nothing: shape
lists, workspace and buffer sizes) are kept as a set, since the order in which a host function asks them means nothing.
"""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

TALL, SHORT = 8192, 1000
TANH, RELU, SELU, GELU = 1, 2, 5, 6
_QUERY_WORDS = ("_supported", "_workspace_bytes", "_elements", "_zeros_floats", "_tn_chunks", "_status_string", "_abi_version")


class RecordingLibrary:
    """Stands in for the ctypes handle that _lib.load_library() returns: every relgnn_* attribute read is noted and passed on."""

    def __init__(self, lib):
        self._lib, self.calls, self.queries = lib, [], set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("relgnn_"):
            if name.endswith(_QUERY_WORDS):
                self.queries.add(name)
            else:
                self.calls.append(name)
        return fn


def _rand(dev, shape, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(shape, device=dev, generator=g) * 2 - 1) * scale


def cases(dev):
    """[(name, switches, thunk)]: thunk() builds its operands (seeded) and returns the product's result."""
    from tf_gnn_samples_amd import dense as D
    NN, NT = D.GEMM_NN, D.GEMM_NT
    out = []

    def case(name, fn, **switches):
        out.append((name, switches, fn))

    def A(rows, k, seed=1):
        return _rand(dev, (rows, k), seed)

    def W(k, n, seed=2):
        return _rand(dev, (k, n), seed, 0.08)

    def Y(rows, n, act=RELU, seed=3):
        y = _rand(dev, (rows, n), seed)
        return torch.relu(y) if act == RELU else torch.tanh(y)

    # ---- NN [tall, 768] . [768, 256] ------------------------------------------------------------------------------------------------
    for pc in ("fwd", "0", "1"):
        case("nn_768_256_weight_relu_pc_" + pc, lambda: D.lib_gemm(NN, A(TALL, 768), W(768, 256), relu=True, weight=True), limb_pc=pc)
    case("nn_768_256_weight_linear", lambda: D.lib_gemm(NN, A(TALL, 768), W(768, 256), weight=True))
    case("nn_768_256_weight_bias_relu", lambda: D.lib_gemm(NN, A(TALL, 768), W(768, 256), _rand(dev, (256,), 4), relu=True, weight=True))
    case("nn_768_256_relu", lambda: D.lib_gemm(NN, A(TALL, 768), W(768, 256), relu=True))
    case("nn_768_256_weight_relu_nocache", lambda: D.lib_gemm(NN, A(TALL, 768), W(768, 256), relu=True, weight=True), weight_limb_cache="0")
    # ---- NT of the same shapes --------------------------------------------------------------------------------------------------------
    for pc in ("fwd", "1"):
        case("nt_256_768_weight_pc_" + pc, lambda: D.lib_gemm(NT, A(TALL, 256), W(768, 256), weight=True), limb_pc=pc)
        case("nt_256_768_weight_premask_relu_pc_" + pc,
             lambda: D.lib_gemm(NT, A(TALL, 256), W(768, 256), weight=True, premask=(RELU, Y(TALL, 768))), limb_pc=pc)
    case("nt_256_768_weight_premask_tanh", lambda: D.lib_gemm(NT, A(TALL, 256), W(768, 256), weight=True, premask=(TANH, Y(TALL, 768, TANH))))
    case("nt_256_768_premask_relu_not_weight", lambda: D.lib_gemm(NT, A(TALL, 256), W(768, 256), premask=(RELU, Y(TALL, 768))))
    case("nt_256_768_not_weight", lambda: D.lib_gemm(NT, A(TALL, 256), W(768, 256)))
    case("nt_premask_of_the_wrong_shape", lambda: D.lib_gemm(NT, A(TALL, 256), W(768, 256), weight=True, premask=(RELU, Y(TALL, 512))))
    # ---- NN weight with other activations ---------------------------------------------------------------------------------------------
    for k in (256, 768):
        for name, act in (("tanh", TANH), ("selu", SELU)):
            case("nn_%d_256_weight_%s" % (k, name), lambda k=k, act=act: D.lib_gemm(NN, A(TALL, k), W(k, 256), weight=True, act=act))
    case("nn_256_256_weight_gelu", lambda: D.lib_gemm(NN, A(TALL, 256), W(256, 256), weight=True, act=GELU))
    case("nn_256_256_gelu_not_weight", lambda: D.lib_gemm(NN, A(TALL, 256), W(256, 256), act=GELU))
    case("nn_256_256_tanh_not_weight", lambda: D.lib_gemm(NN, A(TALL, 256), W(256, 256), act=TANH))
    case("nn_short_256_256_weight_tanh_premask",
         lambda: D.lib_gemm(NN, A(SHORT, 256), W(256, 256), weight=True, act=TANH, premask=(RELU, Y(SHORT, 256))))
    # ---- [tall, 128] . [128, 128] -----------------------------------------------------------------------------------------------------
    case("nn_128_128_weight", lambda: D.lib_gemm(NN, A(TALL, 128), W(128, 128), weight=True))
    case("nn_128_128_not_weight", lambda: D.lib_gemm(NN, A(TALL, 128), W(128, 128)))
    case("nn_128_128_weight_tanh", lambda: D.lib_gemm(NN, A(TALL, 128), W(128, 128), _rand(dev, (128,), 4), weight=True, act=TANH))
    case("nn_128_128_tanh_not_weight", lambda: D.lib_gemm(NN, A(TALL, 128), W(128, 128), act=TANH))
    case("nt_128_128_weight", lambda: D.lib_gemm(NT, A(TALL, 128), W(128, 128), weight=True))
    case("nn_128_128_weight_nocache", lambda: D.lib_gemm(NN, A(TALL, 128), W(128, 128), weight=True), weight_limb_cache="0")
    # ---- [tall, 256] . [256, 121] + bias: the cut panels ------------------------------------------------------------------------------
    for cut in ("1", "0"):
        case("nn_256_121_bias_cut_" + cut, lambda: D.lib_gemm(NN, A(TALL, 256), W(256, 121), _rand(dev, (121,), 4), weight=True), limb_cut=cut)
    case("nn_256_121_bias_tanh", lambda: D.lib_gemm(NN, A(TALL, 256), W(256, 121), _rand(dev, (121,), 4), weight=True, act=TANH))

    # ---- NT with a zero-padded [tall, 121] gradient against a [256, 121] weight --------------------------------------------------------
    def padded(tag):
        buf = torch.zeros((TALL, 128), device=dev)
        buf[:, :121] = A(TALL, 121)
        return D.mark_zero_padded(buf[:, :121], 128) if tag else buf[:, :121]

    case("nt_padded_121_premask_relu", lambda: D.lib_gemm(NT, padded(True), W(256, 121), weight=True, premask=(RELU, Y(TALL, 256))))
    case("nt_padded_121", lambda: D.lib_gemm(NT, padded(True), W(256, 121), weight=True))
    case("nt_untagged_121_premask_relu", lambda: D.lib_gemm(NT, padded(False), W(256, 121), weight=True, premask=(RELU, Y(TALL, 256))))
    case("nt_padded_121_gemm_lib", lambda: D.lib_gemm(NT, padded(True), W(256, 121), weight=True, premask=(RELU, Y(TALL, 256))), gemm="lib")
    # ---- shapes outside the limb rule -------------------------------------------------------------------------------------------------
    case("nn_k50", lambda: D.lib_gemm(NN, A(TALL, 50), W(50, 256), weight=True))
    case("nn_k50_relu_bias", lambda: D.lib_gemm(NN, A(TALL, 50), W(50, 256), _rand(dev, (256,), 4), relu=True, weight=True))
    case("nn_k1040", lambda: D.lib_gemm(NN, A(TALL, 1040), W(1040, 256), weight=True))
    for gemm in ("limb", "lib", "panel", "torch"):
        case("nn_short_768_256_gemm_" + gemm, lambda: D.lib_gemm(NN, A(SHORT, 768), W(768, 256), _rand(dev, (256,), 4), relu=True, weight=True), gemm=gemm)
        case("nt_short_256_768_gemm_" + gemm, lambda: D.lib_gemm(NT, A(SHORT, 256), W(768, 256), weight=True), gemm=gemm)
    case("nn_tall_768_256_gemm_panel", lambda: D.lib_gemm(NN, A(TALL, 768), W(768, 256), weight=True), gemm="panel")
    case("nn_tall_k50_gemm_panel", lambda: D.lib_gemm(NN, A(TALL, 50), W(50, 256), weight=True), gemm="panel")
    case("tn_short_gemm_torch", lambda: D.lib_gemm(D.GEMM_TN, A(SHORT, 256), A(SHORT, 128, 5)), gemm="torch")
    case("tn_short_gemm_lib", lambda: D.lib_gemm(D.GEMM_TN, A(SHORT, 256), A(SHORT, 128, 5)), gemm="lib")

    def into(accumulate, **kw):
        res = _rand(dev, (TALL, 256), 6)
        return D.lib_gemm(NN, A(TALL, 768), W(768, 256), out=res, accumulate=accumulate, **kw)

    case("nn_out_accumulate", lambda: into(True, weight=True))
    case("nn_out_overwrite", lambda: into(False, weight=True))
    case("nn_out_accumulate_gemm_torch", lambda: into(True), gemm="torch")
    case("nn_out_overwrite_gemm_torch", lambda: into(False, relu=True), gemm="torch")
    case("nn_out_accumulate_tanh", lambda: into(True, weight=True, act=TANH))
    case("nt_out_premask", lambda: D.lib_gemm(NT, A(TALL, 256), W(768, 256), weight=True, out=_rand(dev, (TALL, 768), 6),
                                              premask=(RELU, Y(TALL, 768))))
    case("nt_expanded_gradient", lambda: D.lib_gemm(NT, A(1, 256).expand(TALL, 256), W(768, 256), weight=True))
    case("nn_column_block_of_a_wider_weight", lambda: D.lib_gemm(NN, A(TALL, 128), W(128, 384)[:, :256], weight=True))
    case("nt_column_block_of_a_wider_weight", lambda: D.lib_gemm(NT, A(TALL, 256), W(256, 384)[:, :256], weight=True))
    case("nn_column_block_128", lambda: D.lib_gemm(NN, A(TALL, 128), W(128, 384)[:, :128], weight=True))
    # ---- the entry points below lib_gemm, called as the package calls them -------------------------------------------------------------
    case("limb_gemm_weight_wrong_k", lambda: D.limb_gemm_weight(A(TALL, 256), W(768, 256), D.WEIGHT_NN))
    case("limb_gemm_weight_bad_xmax", lambda: D.limb_gemm_weight(A(TALL, 768), W(768, 256), D.WEIGHT_NN, xmax=torch.ones(5, device=dev), xgroups=3))
    case("limb_dense_scratch_nt", lambda: D.limb_dense(NT, A(TALL, 256), W(768, 256)))
    case("limb_dense_weight", lambda: D.limb_dense(NN, A(TALL, 768), W(768, 256), weight=True))

    def typed(layout, cached, pc_rows=True, bad_out=False):
        L, V, tiles = 5, 3000, 16
        P = tiles * 512
        g = torch.Generator(device="cpu").manual_seed(7)
        tile_type = torch.sort(torch.randint(0, L, (tiles,), generator=g)).values.to(torch.int32).to(dev)
        node = torch.randint(-1, V, (P,), generator=g).to(torch.int32).to(dev)
        Ws = [W(128, 128, 10 + l) for l in range(L)]
        kw = dict(b_select=tile_type, rows_per_select=512)
        if layout == NN:
            a = A(V, 128)
            kw.update(a_rows=node, num_rows=P)
        else:
            a = A(P, 128)
        if bad_out:
            kw["out"] = torch.empty((P, 64), device=dev)
        if cached:
            return D.limb_dense_sel(layout, a, Ws, image=D.sel_image(Ws, layout), **kw)
        return D.limb_dense_sel(layout, a, torch.stack(Ws), **kw)

    for pc in ("0", "fwd", "1"):
        case("typed_nn_cached_typed_pc_" + pc, lambda: typed(NN, True), typed_pc=pc)
    case("typed_nt_cached_typed_pc_1", lambda: typed(NT, True), typed_pc="1")
    case("typed_nt_cached", lambda: typed(NT, True))
    case("typed_nn_stacked", lambda: typed(NN, False))
    case("typed_nn_cached_bad_out", lambda: typed(NN, True, bad_out=True))
    case("sel_cached_flag", lambda: D.limb_dense_sel(NN, A(TALL, 128), [W(128, 128)], cached=True))
    # ---- weight gradients -------------------------------------------------------------------------------------------------------------
    for V in (36000, 36007):
        for m, n in ((256, 256), (768, 256), (50, 256)):
            for sw in (dict(), dict(tn="lib"), dict(gemm="lib"), dict(gemm="torch"), dict(tn="lib", gemm="lib"), dict(tn="lib", gemm="torch")):
                name = "tn_%d_%dx%d" % (V, m, n) + "".join("_%s_%s" % kv for kv in sorted(sw.items()))
                case(name, lambda V=V, m=m, n=n: D.matmul_tn_splitk(A(V, m), _rand(dev, (V, n), 5, 0.05)), **sw)
    case("tn_short_256x256_tn_lib", lambda: D.matmul_tn_splitk(A(300, 256), A(300, 256, 5)), tn="lib")
    case("tn_row_strided_operands_tn_lib", lambda: D.matmul_tn_splitk(A(36000, 512)[:, :128], A(36000, 512, 5)[:, :256]), tn="lib", gemm="lib")

    # ---- the aggregate-first layer's grouped products ---------------------------------------------------------------------------------
    def grouped(kind, rows, xmax=False, premask=False, relu=False):
        ks = [W(256, 256, 10 + l) for l in range(3)]
        a = A(rows, 768)
        kw = dict(xmax=a.abs().view(rows, 3, 256).amax(2).contiguous(), xgroups=3) if xmax else {}
        if kind == "nn":
            return D.grouped_nn_gemm(a, ks, relu=relu, **kw)
        return D.grouped_nt_gemm(a, ks, premask=(RELU, Y(rows, 256)) if premask else None, **kw)

    case("grouped_nn", lambda: grouped("nn", TALL, relu=True))
    case("grouped_nn_pc_0", lambda: grouped("nn", TALL, relu=True), limb_pc="0")
    case("grouped_nn_xmax_pair", lambda: grouped("nn", TALL, xmax=True, relu=True), limb="pair")
    case("grouped_nn_short", lambda: grouped("nn", SHORT, relu=True))
    case("grouped_nn_gemm_lib", lambda: grouped("nn", TALL), gemm="lib")
    case("grouped_nt", lambda: grouped("nt", TALL))
    case("grouped_nt_pc_1", lambda: grouped("nt", TALL), limb_pc="1")
    case("grouped_nt_premask", lambda: grouped("nt", TALL, premask=True))
    case("grouped_nt_premask_pc_1", lambda: grouped("nt", TALL, premask=True), limb_pc="1")
    case("grouped_nt_xmax_pair", lambda: grouped("nt", TALL, xmax=True), limb="pair")
    case("grouped_nt_xmax_pair_premask", lambda: grouped("nt", TALL, xmax=True, premask=True), limb="pair")
    case("grouped_nt_short", lambda: grouped("nt", SHORT))
    case("grouped_nt_short_premask", lambda: grouped("nt", SHORT, premask=True))

    # ---- dense_multi, mm_into, and one Dense layer through autograd --------------------------------------------------------------------
    def multi(rows, k, n, L=5, grad=False):
        ks = [W(k, n, 10 + l).requires_grad_(grad) for l in range(L)]
        x = A(rows, k).requires_grad_(grad)
        y = D.dense_multi(x, ks)
        if not grad:
            return y
        y.backward(_rand(dev, tuple(y.shape), 8, 0.05))
        return (y.detach(), x.grad) + tuple(k.grad for k in ks)

    case("dense_multi_5x128x128", lambda: multi(TALL, 128, 128))
    case("dense_multi_5x128x128_backward", lambda: multi(TALL, 128, 128, grad=True))
    case("dense_multi_short", lambda: multi(SHORT, 128, 128))
    case("dense_multi_9_kernels", lambda: multi(TALL, 128, 128, L=9))
    case("dense_multi_k64", lambda: multi(TALL, 64, 128))
    case("dense_multi_nocache", lambda: multi(TALL, 128, 128), weight_limb_cache="0")
    case("dense_multi_gemm_lib", lambda: multi(TALL, 128, 128), gemm="lib")
    case("mm_into_limb", lambda: D.mm_into(NN, A(TALL, 256), W(256, 256), torch.empty((TALL, 512), device=dev)[:, :256]))
    case("mm_into_limb_nt", lambda: D.mm_into(NT, A(TALL, 256), W(256, 256), torch.empty((TALL, 256), device=dev)))
    case("mm_into_torch", lambda: D.mm_into(NN, A(SHORT, 256), W(256, 256), torch.empty((SHORT, 256), device=dev)))
    case("mm_into_torch_gemm_lib", lambda: D.mm_into(NT, A(TALL, 256), W(256, 256), torch.empty((TALL, 256), device=dev)), gemm="lib")

    # ---- the thin launch wrappers: every entry point the module calls appears in the table --------------------------------------------
    def limbs():
        a, w = A(TALL, 768), W(768, 256)
        wl = D.limb_split(w, transpose=True)
        return D.limb_gemm(D.limb_split(a), wl, _rand(dev, (256,), 4), RELU), D.limb_gemm_xf32(a, wl)

    def tn_pair(scales):
        a, g = A(36007, 768), _rand(dev, (36007, 256), 5, 0.05)
        assert D.limb_tn_supported(a, g)
        return D.limb_gemm_tn(a, g, scales(a), scales(g))

    def tn_tiles():
        V, tiles, chunk = 3000, 16, 512
        a, g = A(V, 128), _rand(dev, (tiles * chunk, 128), 5, 0.05)
        rows = torch.randint(-1, V, (tiles * chunk,), generator=torch.Generator(device="cpu").manual_seed(7)).to(torch.int32).to(dev)
        assert D.limb_tn_tiles_supported(a, g, rows, chunk)
        return D.limb_gemm_tn_tiles(a, g, rows, chunk)

    def tn_group():
        u, V = 128, 36007
        x, h, gxk = A(V, u), A(V, u, 9), _rand(dev, (V, 3 * u), 5, 0.05)
        gK, gU, gb = torch.empty((u, 3 * u), device=dev), torch.empty((u, 3 * u), device=dev), torch.empty(3 * u, device=dev)
        products = [(x, gxk, gK), (h, gxk[:, :2 * u], gU[:, :2 * u]), (h, gxk[:, 2 * u:].contiguous(), gU[:, 2 * u:])]
        assert D.tn_stream_group_ok(products)
        D.tn_stream_group(products, colsum=gb)
        return gK, gU, gb

    def tn_into():
        wide = torch.zeros((128, 384), device=dev)
        D.tn_stream_into(A(36007, 128), _rand(dev, (36007, 256), 5, 0.05), wide[:, :256])
        return wide

    case("limbs_split_and_multiplied", limbs)
    case("limb_gemm_tn_column_scales", lambda: tn_pair(D.col_absmax))
    case("limb_gemm_tn_operand_scales", lambda: tn_pair(D.absmax))
    case("limb_gemm_tn_tiles", tn_tiles)
    case("tn_stream_group_with_column_sums", tn_group)
    case("tn_stream_into_a_column_block", tn_into)
    case("tn_stream_gemm_accumulate", lambda: D.tn_stream_gemm(A(36007, 128), _rand(dev, (36007, 256), 5, 0.05), out=torch.ones((128, 256), device=dev)))
    case("col_absmax_of_18_columns", lambda: D.col_absmax(A(TALL, 18)))
    case("column_sum_of_a_row_strided_block", lambda: D.column_sum(A(TALL, 256)[:, :121]))
    case("act_bwd_from_output_tanh", lambda: D.act_bwd_from_output(TANH, Y(TALL, 256, TANH), A(TALL, 256)))

    def layer(act, rows=TALL, k=256, n=256):
        x = torch.relu(A(rows, k)).requires_grad_(True)
        kernel, bias = W(k, n).requires_grad_(True), _rand(dev, (n,), 4).requires_grad_(True)
        y = D.dense_act(x, kernel, bias, act) if act else D.dense(x, kernel, bias)
        y.backward(_rand(dev, (rows, n), 8, 0.05))
        return y.detach(), x.grad, kernel.grad, bias.grad

    case("dense_layer_linear", lambda: layer(0))
    case("dense_layer_tanh", lambda: layer(TANH))
    case("dense_layer_relu_head_121", lambda: layer(RELU, n=121))
    case("dense_layer_tanh_short", lambda: layer(TANH, rows=SHORT))
    return out


def run(dev, each=None):
    """Every case behind the recording proxy: {name: {"calls", "queries", "raises"}}; each(name, result) sees every result."""
    from tf_gnn_samples_amd import _lib, config, dense as D
    real = _lib.load_library()
    table = {}
    try:
        for name, switches, fn in cases(dev):
            D.clear_caches()
            rec = _lib._lib = RecordingLibrary(real)
            raised = result = None
            try:
                with config.override(**switches):
                    result = fn()
            except Exception as e:            # (recorded: a route that refuses is part of the table)
                raised = type(e).__name__
            finally:
                _lib._lib = real
            torch.cuda.synchronize(dev)
            table[name] = {"calls": rec.calls, "queries": sorted(rec.queries), "raises": raised}
            if each is not None and result is not None:
                each(name, result)
    finally:
        _lib._lib = real
        D.clear_caches()
    return table


def main(argv):
    import numpy as np
    dev = torch.device("cuda:0")
    if argv[0] == "record":
        table = run(dev)
        Path(argv[1]).write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
        print("%d cases, %d entry points" % (len(table), len({c for r in table.values() for c in r["calls"] + r["queries"]})))
    elif argv[0] == "dump":
        out = Path(argv[1])
        out.mkdir(parents=True, exist_ok=True)

        def each(name, result):
            for i, t in enumerate(result if isinstance(result, tuple) else (result,)):
                np.save(out / ("%s.%d.npy" % (name, i)), t.detach().cpu().numpy())

        table = run(dev, each)
        (out / "routes.json").write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
        print("%d cases dumped under %s" % (len(table), out))
    else:
        raise SystemExit("usage: dense_route_cases.py record FILE | dump DIR")


if __name__ == "__main__":
    main(sys.argv[1:])
