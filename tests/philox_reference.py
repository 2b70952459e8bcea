"""NumPy restatement of Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) and of the keep rule of csrc/dropout.hip.
A helper, not a test: tests/test_layer_dropout_cpu.py pins it to the Random123 known-answer vectors, the GPU tests use it as the
reference for the kernels' masks."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two -> the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(w, dtype=np.uint64) & MASK32 for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & MASK32 for w in key]
    for r in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                    # 32 x 32 -> 64: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return c


def threshold(keep_prob):
    return int(round(float(keep_prob) * float(1 << 24)))


def keep_mask(n, keep_prob, seed, replica, step, stream, element_offset=0):
    """bool[n]: element i is kept iff (word >> 8) < T, word = output word (element_offset + i) % 4 of the Philox call with
    key (seed, replica) and counter (g lo, g hi, stream, step), g = (element_offset + i) // 4."""
    e = np.arange(n, dtype=np.uint64) + np.uint64(element_offset)
    g = e >> np.uint64(2)
    words = philox4x32_10((g & MASK32, g >> np.uint64(32), stream, int(step) & 0xffffffff), (int(seed) & 0xffffffff, replica))
    lane = (e & np.uint64(3)).astype(np.int64)
    word = np.choose(lane, [np.broadcast_to(w, e.shape) for w in words])
    return (word >> np.uint64(8)) < np.uint64(threshold(keep_prob))


def dropout_f32(x, keep_prob, mask):
    """(x / keep_prob) * mask in fp32, the reference's order of operations (oracle/model.py:31-35)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (x / np.float32(keep_prob)) * np.asarray(mask, dtype=np.float32).reshape(x.shape)
