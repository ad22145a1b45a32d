"""The random stream of the library's Dropout (include/ftx.h: ftx_dropout) restated in numpy, from the contract alone: Philox4x32-10,
the counter layout, the threshold, the keep rule and the scale.  tests/test_dropout_host.py holds it to Random123's published
vectors; tests/test_dropout_gpu.py holds the kernels to it bit for bit."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers of counter words 0 and 2
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments
U32 = np.uint64(0xFFFFFFFF)
U64 = (1 << 64) - 1


def philox4x32_10(counter, key):
    """Ten rounds on counter = (c0, c1, c2, c3) and key = (k0, k1): arrays (or scalars) of values < 2^32 that broadcast -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + np.uint64(W0)) & U32, (k1 + np.uint64(W1)) & U32
    return tuple(np.broadcast_to(c, np.broadcast(c0, c1, c2, c3).shape).astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    """thr = (uint32) floor((double) p * 2^32), of p as it is given.  The entries take p as a float32: keep_mask and dropout below
    round it first, as passing it to them does (float32(0.3) gives 1288490240, the double 0.3 gives 1288490188)."""
    return int(np.floor(float(p) * 4294967296.0))


def scale(p):
    """(float) (1.0 / (1.0 - (double) p)), of p as it is given."""
    return np.float32(1.0 / (1.0 - float(p)))


def uniform_words(n, seed, call, elem0=0):
    """u of the n logical elements elem0 .. elem0 + n - 1 (wrapping at 2^64) of draw (seed, call): uint32 (n,)."""
    seed, call, elem0 = int(seed) & U64, int(call) & U64, int(elem0) & U64
    g = np.arange(n, dtype=np.uint64) + np.uint64(elem0)      # uint64 addition wraps
    q, lane = g >> np.uint64(2), (g & np.uint64(3)).astype(np.int64)
    words = philox4x32_10((q & U32, q >> np.uint64(32), call & 0xFFFFFFFF, call >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(words, 0)[lane, np.arange(n)] if n else np.zeros(0, dtype=np.uint32)


def keep_mask(n, p, seed, call, elem0=0):
    """keep iff u >= thr, thr of the float32 p: bool (n,)."""
    return uniform_words(n, seed, call, elem0) >= np.uint32(threshold(np.float32(p)))


def dropout(x, p, seed, call, elem0=0):
    """x * (keep ? scale : 0) in float32 over the flattened x: one multiply per element, so NaN / Inf in a dropped element give NaN."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    factor = np.where(keep_mask(x.size, p, seed, call, elem0), scale(np.float32(p)), np.float32(0.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (x.reshape(-1) * factor).reshape(x.shape)
