"""NumPy restatement of include/relgnn_sparse_gradient.h: the named-row arrays of a transposed row pointer, the compact structure with
its remapped long-row plan, and the summation order of relgnn_mt_l2norm in float64 — slot sums in ascending element index, the 64-lane
xor butterfly, the four-wave tree, the butterfly over the 32 partials, (float)sqrt.

Every float64 operation here is one IEEE operation in the order the kernels perform it (a float32's square is exact in float64), so
finite results are compared bit for bit; NaN payloads are compared between the two device launches only."""
import numpy as np

SLOTS, BLOCK, CHUNKS, WAVE = 8192, 256, 32, 64


# ---- named rows ---------------------------------------------------------------------------------------------------------------------
def named_arrays(rowptr_t):
    """(words int32 [T], slot int32 [F + 1], rowptr_c int32 [T + 1]) of an int row pointer [F + 1]."""
    rowptr_t = np.asarray(rowptr_t, np.int64)
    named = rowptr_t[1:] > rowptr_t[:-1]
    words = np.flatnonzero(named).astype(np.int32)
    slot = np.concatenate([[0], np.cumsum(named)]).astype(np.int32)
    rowptr_c = np.array([rowptr_t[f] for f in words] + [rowptr_t[-1]], np.int32)
    return words, slot, rowptr_c


def compact_plan(slabs_t, combos_t, slot):
    """The transposed plan's slabs int32 [S, 4] and combos int32 [C, 3] with every row field mapped through slot."""
    slabs = np.array(slabs_t, np.int32).reshape(-1, 4)
    combos = np.array(combos_t, np.int32).reshape(-1, 3)
    for table in (slabs, combos):
        for entry in table:
            entry[0] = slot[entry[0]]
    return slabs, combos


def compact_structure(rowptr_t, slabs_t, combos_t):
    """-> dict of every array of the compact form (col, val and ws_rows are the transposed structure's own)."""
    words, slot, rowptr_c = named_arrays(rowptr_t)
    slabs, combos = compact_plan(slabs_t, combos_t, slot)
    return {"words": words, "slot": slot, "rowptr": rowptr_c, "slabs": slabs, "combos": combos}


def held_words(lengths, num_nodes, seed=0):
    """(rowptr, col, val, shape) of a CSR matrix [num_nodes, len(lengths)] whose word f is held by lengths[f] nodes: its transposed
    row f has that length."""
    rng = np.random.default_rng([5, seed])
    lengths = np.asarray(lengths, np.int64)
    node = np.concatenate([np.sort(rng.choice(num_nodes, size=k, replace=False)) for k in lengths] + [np.zeros(0, np.int64)])
    word = np.repeat(np.arange(len(lengths)), lengths)
    order = np.lexsort((word, node))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=num_nodes))])
    val = (rng.standard_normal(len(node)) + 3).astype(np.float32)
    return rowptr, word[order], val, (num_nodes, len(lengths))


MIXED_LENGTHS = {3: 1, 7: 128, 8: 129, 100: 512, 101: 513, 250: 1100, 299: 2}      # word -> holders: one-, two- and three-slab rows


def mixed_lengths(F=300):
    lengths = np.zeros(F, np.int64)
    lengths[list(MIXED_LENGTHS)] = list(MIXED_LENGTHS.values())
    return lengths


# ---- the norm's order -----------------------------------------------------------------------------------------------------------------
def _butterfly(lanes):
    """64 doubles -> 64 doubles: x += x[lane ^ off] for off = 32 .. 1, every lane at once."""
    x = np.array(lanes, np.float64)
    index = np.arange(WAVE)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            x = x + x[index ^ off]
    return x


def tree(slot_sums):
    """slot sums float64 [8192] -> (partials float64 [32], norm float32)."""
    slot_sums = np.asarray(slot_sums, np.float64).reshape(CHUNKS, BLOCK // WAVE, WAVE)
    partials = np.empty(CHUNKS, np.float64)
    with np.errstate(all="ignore"):
        for b in range(CHUNKS):
            r = [_butterfly(slot_sums[b, w])[0] for w in range(BLOCK // WAVE)]
            partials[b] = (r[0] + r[1]) + (r[2] + r[3])
        total = _butterfly(np.concatenate([partials, np.zeros(WAVE - CHUNKS)]))[0]
        return partials, np.float32(np.sqrt(total))


def dense_slot_sums(g, descending=False):
    """Slot s adds double(x) * double(x) over the elements i = s, s + 8192, ... of the flattened array to +0.0, in ascending i
    (descending=True: the wrong order, for the test that the inputs can tell the two apart)."""
    flat = np.ascontiguousarray(g, np.float32).reshape(-1).astype(np.float64)
    acc = np.zeros(SLOTS, np.float64)
    passes = range(0, len(flat), SLOTS)
    with np.errstate(all="ignore"):
        for first in (reversed(passes) if descending else passes):
            piece = flat[first:first + SLOTS]
            acc[:len(piece)] = acc[:len(piece)] + piece * piece
    return acc


def compact_slot_sums(words, values, descending=False):
    """The same sums from the named rows alone: row t holds the elements words[t] * n .. + n of the dense array; each slot takes
    them in ascending t."""
    values = np.ascontiguousarray(values, np.float32).astype(np.float64)
    n = values.shape[1] if values.ndim == 2 else 0
    acc = np.zeros(SLOTS, np.float64)
    order = range(len(words))
    with np.errstate(all="ignore"):
        for t in (reversed(order) if descending else order):
            at = (int(words[t]) * n + np.arange(n)) % SLOTS          # distinct: n <= 1024
            acc[at] = acc[at] + values[t] * values[t]
    return acc


def dense_norm(g, descending=False):
    return tree(dense_slot_sums(g, descending))


def compact_norm(words, values, descending=False):
    return tree(compact_slot_sums(words, values, descending))


def bits64(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits32(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def spread_values(rng, words, n):
    """float32 [len(words), n] for the rows `words` of a [F, n] gradient, magnitudes spread over about 2^-20 .. 2^20 so that the order
    of every sum shows in its bits: the exponent of an element rises with the BLOCK its slot belongs to (the 32 partials differ by
    2^40 end to end, so the butterfly over them rounds), with a jitter of 2^+-3 inside a block (the terms of a slot and the slots of
    a block are comparable, so a slot summed the other way round changes its block's partial instead of drowning in it)."""
    words = np.asarray(words, np.int64)
    block = ((words[:, None] * n + np.arange(n)) % SLOTS) // BLOCK
    exponent = -20 + 40 * block / (CHUNKS - 1) + rng.uniform(-3, 3, block.shape)
    return (rng.standard_normal(block.shape) * np.exp2(exponent)).astype(np.float32)


def named_sets(rng, F, n):
    """name -> ascending int32 words: one row, all rows, every (8192 / n)-th row (one residue: every row falls on the same slots),
    the first and last rows, a random tenth."""
    period = max(1, SLOTS // n)
    tenth = np.sort(rng.choice(F, size=max(1, F // 10), replace=False))
    sets = {"one": [F // 3], "all": np.arange(F), "one residue": np.arange(1, F, period), "ends": [0, F - 1], "tenth": tenth}
    return {k: np.asarray(v, np.int32) for k, v in sets.items()}


NORM_SHAPES = [(5000, 4), (5000, 12), (300, 64), (300, 256), (300, 1024)]       # (F, n): F * n > 8192, so slots wrap


def norm_case(F, n, name):
    """(words, values [T, n]) of one GPU case, from a seed of its own."""
    rng = np.random.default_rng([77, F, n])
    sets = named_sets(rng, F, n)
    words = sets[name]
    return words, spread_values(np.random.default_rng([78, F, n, sorted(sets).index(name)]), words, n)


def to_dense(words, values, F):
    dense = np.zeros((F, values.shape[1]), np.float32)
    dense[np.asarray(words, np.int64)] = values
    return dense
