"""The limb images of the step's WEIGHT operands: split once per optimizer step, all of them in one launch.

A weight is the right operand of two or three products per step (forward, input gradient) and changes once per step.  Its limb
image (three bf16 limbs per fp32 value, csrc/limb_gemm.hip; `pair`: two fp16 limbs) is kept until the weights change: the
optimizer's fused update writes through raw pointers (tensor versions do not move) and says so through weights_changed(); every
other in-place write moves the tensor's version, which is compared too.  The first request after a change re-splits every image
that the previous step used (relgnn_limb_split_multi_f32); an image may be several matrices side by side along k (the per-edge-
type kernels of a layer), so neither the stacked [L*Din, Dout] operand of the forward product nor the stacked W^T of the input
gradient is ever formed in fp32.  C2: 8 split launches + 3 stacks + 3 re-layouts per step -> 1 launch.

ONE structure holds all of it (_CACHE): a generation counter and, per (device, stream), a _Table that owns its images and
everything that names them — the general index (kind, layout, address / shape / stride of every matrix), the identity index in
front of it (the tensor objects themselves: sel_image) and the marshalled argument arrays of the sets of images that are re-split
together.  ONE rule says whether an image may serve a request (_image_state, asked by both indices), ONE function takes an image
out of a table (_Table.evict: afterwards nothing here refers to the image or its device buffer), ONE function allocates one
(_new_image).  Under stream capture nothing is cached (a replay re-runs kernels, not this code) and the image is split on every
request — unless capture_image_cache() is open, whose tables live exactly as long as it is."""
import ctypes
import weakref

import torch

from . import _lib
from .config import settings as _cfg

GEMM_NN, GEMM_NT, GEMM_TN = 0, 1, 2          # the product layouts of dense.py (which takes them from here)
WEIGHT_NN, WEIGHT_NT = "nn", "nt"


class _PerStream(dict):
    """Scratch keyed by (device, raw stream handle): products issued on different streams may run concurrently and must not
    share it.  Bounded: at most `limit` streams per cache are remembered, the least recently used entry goes first (a process
    that keeps creating streams — graph captures, user streams — would otherwise pin 64 MB per stream for its lifetime, and a
    recycled stream handle would find another stream's entry).  Dropping an entry only returns its memory to torch's caching
    allocator, which hands it out again in stream order of the stream it was allocated on; dense.clear_caches() empties all of
    them."""

    def __init__(self, limit: int = 4):
        super().__init__()
        self.limit = limit

    def lookup(self, key):
        v = self.get(key)
        if v is not None:                      # move to the back: most recently used
            del self[key]
            self[key] = v
        return v

    def store(self, key, value):
        self.pop(key, None)
        while len(self) >= self.limit:
            del self[next(iter(self))]
        self[key] = value
        return value


def _weight_matrices(w):
    """A weight operand as a list of 2-D matrices laid side by side along k: a matrix, a [L, ., .] stack or a sequence."""
    if torch.is_tensor(w):
        return [w] if w.dim() == 2 else list(w.unbind(0))
    return list(w)


def _weight_image_shape(ws, kind: str):
    """(N, K) of B [N, K] = [w_0^T | w_1^T | ..] (WEIGHT_NN: w_l [K_l, N]) or [w_0 | w_1 | ..] (WEIGHT_NT: w_l [N, K_l])."""
    # (a single matrix whose k extent is not a multiple of 16 — the 121-label head — fills its last k-tile with zeros)
    k = sum(m.shape[0] if kind == WEIGHT_NN else m.shape[1] for m in ws)
    if len(ws) == 1:
        k = (k + 15) // 16 * 16
    return (ws[0].shape[1] if kind == WEIGHT_NN else ws[0].shape[0]), k


def weight_image_ok(ws, kind: str) -> bool:
    ws = _weight_matrices(ws)
    n = ws[0].shape[1] if kind == WEIGHT_NN else ws[0].shape[0]
    for m in ws:
        if not (m.is_cuda and m.dtype == torch.float32 and m.dim() == 2 and m.stride(1) == 1 and m.stride(0) >= m.shape[1]
                and (len(ws) == 1 or (m.stride(0) % 4 == 0 and m.data_ptr() % 16 == 0))):
            return False                   # (a single matrix may have rows of any alignment — [256, 121]: the split reads element-wise)
        if (m.shape[1] if kind == WEIGHT_NN else m.shape[0]) != n or ((m.shape[0] if kind == WEIGHT_NN else m.shape[1]) % 16 != 0
                                                                     and len(ws) > 1):
            return False
    return True


def _weight_image_items(ws, kind: str, buf: torch.Tensor, per: int = 0):
    """(X, ldx, rows, cols, transpose, out, kt_offset, kt_total) per matrix of the image.  per > 0 (`separate`): every matrix is
    an image of its own, matrix l at element l * per of buf."""
    total = _weight_image_shape(ws[:1] if per else ws, kind)[1] // 16
    items, kt = [], 0
    for l, m in enumerate(ws):
        items.append((m.data_ptr(), m.stride(0), m.shape[0], m.shape[1], 1 if kind == WEIGHT_NN else 0,
                      buf.data_ptr() + 2 * per * l, 0 if per else kt, total))
        kt += ((m.shape[0] if kind == WEIGHT_NN else m.shape[1]) + 15) // 16
    return items


class _WeightImage:
    # (no strong reference to the weights unless its table pins them; pair: two fp16 limbs, `wmax` = the device float the image's
    # scale comes from; refs / versions: per matrix, of the tensor that owns its storage — the matrix itself or its _base)
    __slots__ = ("key", "id_key", "refs", "pins", "items", "versions", "gen", "used_gen", "buf", "pair", "wmax")


def _new_image(ws, kind: str, pair: bool, separate: bool, key, pin: bool) -> "_WeightImage":
    """A never-split image of the matrices ws: THE place that sizes and allocates an image buffer."""
    lib = _lib.load_library()
    im = _WeightImage()
    rows, cols = _weight_image_shape(ws[:1] if separate else ws, kind)
    per = int(lib.relgnn_limb16_elements(rows, cols) if pair else lib.relgnn_limb_elements(rows, cols))
    im.buf = torch.empty(per * len(ws) if separate else per, dtype=torch.bfloat16, device=ws[0].device)
    im.items = _weight_image_items(ws, kind, im.buf, per if separate else 0)
    bases = [m._base if m._base is not None else m for m in ws]
    im.refs, im.pins = [weakref.ref(b) for b in bases], (bases if pin else None)
    im.key, im.id_key, im.pair, im.wmax, im.gen, im.versions, im.used_gen = key, None, pair, None, -1, [None] * len(ws), -1
    return im


_FRESH, _STALE, _FOREIGN = 0, 1, 2


def _image_state(im: "_WeightImage", ws, gen: int) -> int:
    """THE validity rule, asked by the identity index and by the general index alike: may the cached image `im` serve a request for
    the matrices ws?  Per matrix: the tensor that owns the storage is the same object as when the image was made (weakref), the
    matrix sits at the same address with the same row stride (`p.data = other` moves a parameter without moving its version), and
    its version and the global generation are those of the last split.
      _FRESH    yes
      _STALE    the same matrices in the same place, written since (version / weights_changed()): re-split into the same buffer
      _FOREIGN  other tensors, or these somewhere else: not their image — evict"""
    state = _FRESH if im.gen == gen else _STALE
    for w, r, v, it in zip(ws, im.refs, im.versions, im.items):
        base = w._base
        if r() is not (w if base is None else base) or w.data_ptr() != it[0] or w.stride(0) != it[1]:
            return _FOREIGN
        if w._version != v:
            state = _STALE
    return state


def _marshal(items):
    """The leading arguments of the two split entry points: the count and one ctypes array per field of the items."""
    n = len(items)
    cols = list(zip(*items))
    vp, i64, i32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int32 * n
    return (n, vp(*cols[0]), i64(*cols[1]), i32(*cols[2]), i32(*cols[3]), i32(*cols[4]), vp(*cols[5]), i32(*cols[6]), i32(*cols[7]))


def _split_weight_images(images, marshalled: dict) -> None:
    """The split launches for `images` of one table.  marshalled: that table's {ids of a set of images: launch arguments}."""
    triples = [im for im in images if not im.pair]
    pairs = [im for im in images if im.pair]
    if triples:
        # the argument arrays of a set of images are the same every step (an image's items never change): built once per set — a
        # 23-type, 10-layer model re-splits ~1400 matrices per step, and marshalling them anew cost milliseconds of host time.
        # The key is the images' ids alone: the table holds every image named there, and _Table.evict drops the entry with the image.
        key = tuple(map(id, triples))
        ent = marshalled.get(key) or _marshal([it for im in triples for it in im.items])
        if len(triples) > 4:                           # (small sets are cheap to marshal and vary more)
            marshalled[key] = ent
        _lib.launch("relgnn_limb_split_multi_f32", *ent)
    if pairs:           # two fp16 limbs: one magnitude per image first (its power-of-two scale), then the limbs — three launches
        wm = torch.empty(len(pairs), dtype=torch.float32, device=pairs[0].buf.device)
        for i, im in enumerate(pairs):
            im.wmax = wm[i:i + 1]
        items = [it for im in pairs for it in im.items]
        image = [i for i, im in enumerate(pairs) for _ in im.items]
        _lib.launch("relgnn_limb16_split_multi_f32", *_marshal(items), (ctypes.c_int32 * len(image))(*image), len(pairs), wm.data_ptr())


class _Table:
    """The images of one (device, stream) and every index that names them.  pin: the images hold strong references to their
    weights (the tables of capture_image_cache(): the addresses recorded into the graph stay alive for the capture's duration)."""

    def __init__(self, pin: bool = False):
        self.images = {}          # (kind, pair, separate, (address, rows, cols, row stride) per matrix) -> _WeightImage
        self.by_identity = {}     # (kind, id() per matrix) -> a `separate` image of tensors that are no views, also in images
        self.marshalled = {}      # (id() per image of a set that was split together) -> ctypes arguments of that launch
        self.pin = pin

    def evict(self, im: "_WeightImage") -> None:
        """Forget im: out of both indices, and every marshalled argument array that mentions it (they hold raw addresses).
        (images[k] is im exactly when im.key == k, by_identity[k] is im exactly when im.id_key == k: image() keeps it so.)"""
        self.images.pop(im.key, None)
        self.by_identity.pop(im.id_key, None)
        for k in [k for k in self.marshalled if id(im) in k]:
            del self.marshalled[k]

    def known(self, ws, kind: str, gen: int):
        """The fresh image of exactly these tensor objects, or None.  In front of the general index because a training step asks for
        the same parameters' images five or six times per layer, and building the general key (addresses, shapes, strides, bases of
        every matrix) costs more host time than the split launch it saves when a layer has 23 of them (measured, round 6: C5
        31.2 -> 32.7 ms with the general lookup alone, eager)."""
        im = self.by_identity.get((kind,) + tuple(map(id, ws)))
        if im is not None and im.gen == gen and _image_state(im, ws, gen) == _FRESH:      # (gen first: spares the loop once per step)
            im.used_gen = gen
            return im
        return None

    def image(self, ws, kind: str, pair: bool, separate: bool, gen: int) -> "_WeightImage":
        indexable = separate and not pair
        im = self.known(ws, kind, gen) if indexable else None
        if im is not None:
            return im
        key = (kind, pair, separate) + tuple((m.data_ptr(), m.shape[0], m.shape[1], m.stride(0)) for m in ws)
        im = self.images.get(key)
        state = _image_state(im, ws, gen) if im is not None else _FOREIGN
        if state == _FOREIGN:
            if im is not None:
                self.evict(im)                               # another tensor lives at that address now
            im = self.images[key] = _new_image(ws, kind, pair, separate, key, self.pin)
        if indexable and all(m._base is None for m in ws):  # (a view is a new object on every call: nothing to find it by)
            id_key = (kind,) + tuple(map(id, ws))
            old = self.by_identity.get(id_key)
            if old is not None and old is not im:
                self.evict(old)                              # these objects' image from before their storage was replaced
            self.by_identity.pop(im.id_key, None)            # (im may have been asked for through other objects on the same storage)
            im.id_key, self.by_identity[id_key] = id_key, im
        if state != _FRESH:
            todo = [im]
            for other in [o for o in self.images.values() if o is not im]:
                alive = [r() for r in other.refs]
                if any(b is None for b in alive) or other.used_gen < gen - 1:       # gone, or not part of the last step: forget it
                    self.evict(other)
                elif other.gen != gen or other.versions != [b._version for b in alive]:
                    todo.append(other)
            _split_weight_images(todo, self.marshalled)
            for t in todo:
                t.gen, t.versions = gen, [r()._version for r in t.refs]
        im.used_gen = gen
        return im


class _ImageCache:
    def __init__(self):
        self.gen = 0                          # moved by weights_changed()
        self.streams = _PerStream(limit=8)    # (device, stream) -> _Table
        self.capture = None                   # the same for requests under stream capture, while capture_image_cache() is open

    def table(self, device):
        """The table that serves requests on the current stream, or None where nothing may be cached: the switch is off, or the
        stream is capturing outside capture_image_cache()."""
        capturing = torch.cuda.is_current_stream_capturing()
        tables = self.capture if capturing else self.streams
        if tables is None or _cfg.weight_limb_cache != "1":
            return None
        key = (device, _lib.current_stream())
        return tables.lookup(key) or tables.store(key, _Table(pin=capturing))


_CACHE = _ImageCache()


def clear() -> None:
    """Drop every cached image (the next request re-splits).  Never needed for correctness."""
    _CACHE.streams.clear()
    if _CACHE.capture is not None:
        _CACHE.capture.clear()


def image_count(device) -> int:
    """How many images the table of `device` and the current stream holds (tests; creates and touches nothing)."""
    table = _CACHE.streams.get((device, _lib.current_stream()))
    return len(table.images) if table is not None else 0


class capture_image_cache:
    """Around the capture of ONE training step into a hipGraph: limb images split inside the capture are reused by later products of
    the same capture (forward -> backward) until weights_changed() — which the captured optimizer update calls — drops them.
    Within one captured training step the weights change once, at its end: an image split for the forward serves the backward too
    (Sparse_Graph_Model.capture_train_step opens this around the capture)."""

    def __enter__(self):
        _CACHE.capture = _PerStream(limit=8)
        return self

    def __exit__(self, *exc):
        _CACHE.capture = None


def weights_changed() -> None:
    """Tell the limb-image cache that parameters were rewritten in place by something torch's version counters do not see:
    a kernel that writes through raw pointers (models/sparse_graph_model.py: the fused clip + Adam launch; a hipGraph replay of
    it), `p.data.copy_()` / `p.data.mul_()`, a third-party optimizer that updates `.data`, a parameter broadcast.  Ordinary
    in-place tensor operations on the parameter itself (`p.add_()`, `p.copy_()` under no_grad) move its version and are noticed
    without this call.  PUBLIC CONTRACT of the default route (config gemm=limb, weight_limb_cache=1): whoever writes weights
    behind torch's back calls tf_gnn_samples_amd.dense.weights_changed() (cheap: a counter) — or runs with
    RELGNN_WEIGHT_LIMB_CACHE=0, which re-splits on every product."""
    _CACHE.gen += 1
    if _CACHE.capture is not None:
        _CACHE.capture.clear()


def weight_limbs(w, kind: str) -> torch.Tensor:
    """The bf16-triple limb image (flat buffer) of a weight operand: weight_image(w, kind).buf."""
    return weight_image(w, kind).buf


def weight_image(w, kind: str, pair: bool = False, separate: bool = False) -> "_WeightImage":
    """The limb image of a weight operand as the right operand B [N, K] of relgnn_limb_gemm_xf32 (pair: of relgnn_limb16_gemm_xf32:
    two fp16 limbs, .wmax = the device float its scale comes from); .buf is the flat 16-bit buffer.  w: a matrix, a
    [L, ., .] stack or a sequence of matrices (laid side by side along k):
      WEIGHT_NN  w_l [K_l, N]:  [x_0 | x_1 | ..] @ [w_0; w_1; ..] = sum_l x_l @ w_l     (Dense forward; gnns/rgcn.py:96-98 summed over
                                                                                          the edge types in one product)
      WEIGHT_NT  w_l [N, K_l]:  [g_0 | g_1 | ..] @ [w_0 | w_1 | ..]^T = sum_l g_l @ w_l^T   (the input gradients of the same)
    separate: one image PER matrix, one behind the other in the buffer (matrix l at element l * relgnn_limb_elements(N, K); every
    matrix the same shape, N % 128 == 0) — the per-edge-type operands of relgnn_limb_gemm_sel_xf32 (round 6: the typed transforms
    and the D = 128 Dense layers no longer re-split their weights in front of every product).
    Valid until the next weights_changed() / in-place write to a matrix; on the current stream."""
    ws = _weight_matrices(w)
    table = _CACHE.table(ws[0].device) or _Table()          # (nothing may be cached: a table that lives for this request — one split)
    return table.image(ws, kind, pair, separate, _CACHE.gen)


def sel_weights_cacheable(ws, layout: int) -> bool:
    """May the 128-column panel product take its weights from the step's limb-image cache (weight_image(separate=True))?  ws: the
    weight matrices as the caller holds them (parameters or views of parameters: something whose storage outlives the product and
    whose version moves when it is written) — all the same shape, N % 128 == 0, K % 16 == 0."""
    ws = _weight_matrices(ws)
    kind = WEIGHT_NN if layout == GEMM_NN else WEIGHT_NT
    n, k = (ws[0].shape[1], ws[0].shape[0]) if layout == GEMM_NN else (ws[0].shape[0], ws[0].shape[1])
    return (_cfg.weight_limb_cache == "1" and n % 128 == 0 and k % 16 == 0 and all(m.shape == ws[0].shape for m in ws)
            and weight_image_ok(ws[:1], kind) and all(weight_image_ok([m], kind) for m in ws[1:]))


def sel_image(ws, layout: int):
    """The cached limb images of the weight matrices `ws` (one image per matrix, one behind the other) for the 128-column panel
    products, or None when they cannot come from the cache (shapes, switches): sel_weights_cacheable() and then
    weight_image(separate=True) — behind a look by the IDENTITY of the weight tensors (_Table.known), which answers all but the
    first request of a step without evaluating either."""
    ws = _weight_matrices(ws)
    if not ws[0].is_cuda:
        return None
    kind = WEIGHT_NN if layout == GEMM_NN else WEIGHT_NT
    table = _CACHE.table(ws[0].device)
    im = table.known(ws, kind, _CACHE.gen) if table is not None else None
    if im is not None or not sel_weights_cacheable(ws, layout):
        return im
    return weight_image(ws, kind, separate=True)
