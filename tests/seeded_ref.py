"""The counter-based noise of include/mmd.h (mmd_ctr_fill) restated in numpy, for tests/test_seeded_cpu.py and tests/test_seeded_gpu.py
(test infrastructure): Philox4x32-10 on (element >> 2, draw, sample id, tag) keyed with the seed, the words' uniforms and the Box-Muller
normals in float64."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
X_T = 0xFFFFFFFF

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

# the (seed, sample id, draw, tag) blocks of 2^20 values whose moments the GPU tests check at 5 sigma (the CPU test holds the float64
# emulation of each to 4 sigma): three blocks, and for each a partner that differs in the tag, the id or the draw alone
SEED = 42
NBLOCK = 1 << 20
BLOCKS = [(SEED, 0, X_T, 0), (SEED, 7, 3, 1), (SEED, 2 ** 32 - 1, 0, 2)]
PARTNERS = [(SEED, 0, X_T, 1), (SEED, 8, 3, 1), (SEED, 2 ** 32 - 1, 1, 2)]       # other tag / id k + 1 / draw i + 1


def philox(c0, c1, c2, c3, k0, k1):
    """Vectorised over the counter words (arrays or ints); returns four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LO for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(seed, sid, draw, tag, per):
    """uint32 [per]: the words of one sample's elements in layout order."""
    q = np.arange((per + 3) // 4, dtype=np.uint64)
    w = philox(q, draw, sid, tag, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=1).reshape(-1)[:per]


def normals64(w):
    """float64 Box-Muller of the words of whole quads and a tail (the tail's partner words are not needed: a cosine needs both words
    of its pair, so the caller passes words cut from full quads - pad with words(...) of the next multiple of 4)."""
    n = len(w)
    assert n % 4 == 0
    u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    ua, ub = u[0::2], u[1::2]
    rho = np.sqrt(-2.0 * np.log(ua))
    z = np.empty(n)
    z[0::2] = rho * np.cos(2.0 * np.pi * ub)
    z[1::2] = rho * np.sin(2.0 * np.pi * ub)
    return z


def normals(seed, sid, draw, tag, per):
    return normals64(words(seed, sid, draw, tag, (per + 3) // 4 * 4))[:per]


def scores(z):
    """|statistic - expectation| / standard error for mean, variance, fourth moment and lag-1 correlation of n N(0,1) values."""
    n = len(z)
    return {"mean": abs(z.mean()) * np.sqrt(n), "var": abs(z.var() - 1.0) / np.sqrt(2.0 / n),
            "m4": abs((z ** 4).mean() - 3.0) / np.sqrt(96.0 / n), "lag1": abs((z[:-1] * z[1:]).mean()) * np.sqrt(n - 1)}


def corr_score(a, b):
    return abs((a * b).mean()) * np.sqrt(len(a))
