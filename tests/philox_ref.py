"""Host restatement (numpy) of the dropout mask that include/lcrec.h defines: Philox4x32-10 keyed by the seed, counted by
(element index / 4, position, step).  Shared by tests/test_dropout_host.py and tests/test_gpu_dropout.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> [..., 4] uint32 words."""
    c = [np.asarray(v, dtype=np.uint64) & _LOW for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(p):
    """(T, s): keep iff word >= T; a kept value is x * s (one fp32 multiply)."""
    return min(2 ** 32 - 1, int(float(p) * 4294967296.0)), np.float32(1.0 / (1.0 - float(p)))


def words(shape, seed, step, position, row_offset=0):
    """The uint32 word of every element of a [rows, features] tensor (features % 4 == 0)."""
    n, feat = shape
    assert feat % 4 == 0
    seed = int(seed) & (2 ** 64 - 1)
    q = np.arange(n * feat // 4, dtype=np.uint64) + np.uint64(row_offset * feat // 4)
    w = philox4x32_10((q & _LOW, q >> _32, np.uint64(position), np.uint64(int(step) & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, seed >> 32))
    return w.reshape(n, feat)


def keep_mask(shape, p, seed, step, position, row_offset=0):
    """bool [rows, features]: True where the element is kept."""
    return words(shape, seed, step, position, row_offset) >= np.uint32(threshold(p)[0])
