"""numpy restatements for the graph-replayed DPM-Solver++ step (include/mmd.h: mmd_dpmpp_*).

The selection.  |x| as IEEE bits (sign stripped) is order-preserving for non-negative floats, so rank r of |x| is rank r of the 31-bit
integers.  The kernels split them 11 + 10 + 10:
    level 0  every workgroup of DPMPP_CHUNK elements counts the top 11 bits in LDS and flushes its non-empty bins into the sample's table
    level 1  every workgroup re-derives, from the level-0 table, the bin b0 that holds the rank and the rank left inside it, then counts
             bits 19..10 of the elements whose top 11 bits equal b0 (one table per wanted rank: the lower and the upper neighbour)
    level 2  the same one level down: prefix (b0, b1) from the level-0 and level-1 tables, counts bits 9..0
    final    walks the three tables: bits = b0 << 20 | b1 << 10 | b2
and the quantile is vlo + (vhi - vlo) frac with pos = q (per - 1) in double, lo = floor(pos), hi = min(lo + 1, per - 1),
frac = float(pos - lo), the lerp as one fused multiply-add: what abs_quantile_kernel computes.  select() restates this with the
workgroup structure kept (so that a lost flush can be seeded); np.partition on the integers is the independent reference."""
import numpy as np

CHUNK = 4096
L0_BINS, L_BINS = 2048, 1024
WS_WORDS = L0_BINS + 4 * L_BINS
Q_CASES = (0.0, 0.5, 0.995, 1.0)
TINY_SIZES = (8 * 3 * 16 * 16, 512)            # the tiny model's video and audio samples
PER_CASES = (1, 2, 3, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5) + TINY_SIZES
INPUT_KINDS = ("normal_0.3", "normal_1", "normal_4", "equal", "ties", "zeros_denormals", "share11", "share21", "inf")


def absbits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def ranks(per, q):
    """(lo, hi, frac) as quantile_ranks of the kernels: q is the fp32 value the C ABI receives."""
    pos = float(np.float32(q)) * float(per - 1)
    lo = int(np.floor(pos))
    hi = lo + 1 if lo + 1 < per else lo
    return lo, hi, np.float32(pos - lo)


def lerp32(vlo, vhi, frac):
    """fmaf(vhi - vlo, frac, vlo): the difference rounded to fp32, the product exact in float64 (24 x 24 bits), one rounding of the sum
    (exact unless the float64 sum itself rounds: 53 bits against at most 48 + alignment - equal on every case of these tests)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(vhi) - np.float32(vlo)
        return np.float32(np.float64(d) * np.float64(frac) + np.float64(vlo))


def lerp64(vlo, vhi, frac):
    """the same interpolation in float64 throughout: stands beside lerp32"""
    with np.errstate(invalid="ignore"):
        return np.float64(vlo) + (np.float64(vhi) - np.float64(vlo)) * np.float64(frac)


def partition_bits(x, rank):
    """the independent reference: the rank-th smallest |x| as bits"""
    b = absbits(x).reshape(-1)
    return int(np.partition(b, rank)[rank])


def hist0(x):
    """level-0 table of one sample"""
    return np.bincount(absbits(x).reshape(-1) >> 20, minlength=L0_BINS).astype(np.uint32)


def _find(table, rank):
    """the bin of `table` that holds `rank` and the rank inside it (find_bin of the kernels); a rank past the total leaves (0, 0)"""
    c = np.cumsum(table.astype(np.int64))
    if rank >= c[-1]:
        return 0, 0
    b = int(np.searchsorted(c, rank, side="right"))
    return b, int(rank - (c[b - 1] if b else 0))


def _pass(b, chunks, shift, prefix, defect_drop):
    """one grid-wide histogram pass: per workgroup a private table, then the flush"""
    table = np.zeros(L0_BINS if prefix is None else L_BINS, dtype=np.int64)
    for w, (lo, hi) in enumerate(chunks):
        part = b[lo:hi]
        if prefix is not None:
            part = part[(part >> (shift + 10)) == prefix]
        digit = (part >> shift) & (len(table) - 1)
        if w == defect_drop:                          # seeded defect: one workgroup's flush is lost
            continue
        table += np.bincount(digit, minlength=len(table))
    return table


def select(x, q, defect=None):
    """The quantile of |x| (one sample, any shape) by the three-level scheme -> (fp32 value, (bits_lo, bits_hi)).
    defect: None | "rank_off_by_one" | "dropped_flush" | "prefix_wrong_level"."""
    b = absbits(x).reshape(-1).astype(np.int64)
    per = b.size
    lo, hi, frac = ranks(per, q)
    if defect == "rank_off_by_one":
        lo, hi = min(lo + 1, per - 1), min(hi + 1, per - 1)
    chunks = [(s, min(s + CHUNK, per)) for s in range(0, per, CHUNK)]
    drop = 0 if defect == "dropped_flush" else None      # the first workgroup: a full chunk
    t0 = _pass(b, chunks, 20, None, None)
    out = []
    for rank in (lo, hi):
        b0, r0 = _find(t0, rank)
        t1 = _pass(b, chunks, 10, b0, drop)
        b1, r1 = _find(t1, r0)
        if defect == "prefix_wrong_level":             # seeded defect: level 2 filters on the level-0 bin alone
            part = b[(b >> 20) == b0]
            t2 = np.bincount(part & (L_BINS - 1), minlength=L_BINS)
        else:
            t2 = _pass(b, chunks, 0, (b0 << 10) | b1, None)
        b2, _ = _find(t2, r1)
        out.append((b0 << 20) | (b1 << 10) | b2)
    v = [np.array([o], dtype=np.uint32).view(np.float32)[0] for o in out]
    return lerp32(v[0], v[1], frac), tuple(out)


def reference(x, q):
    """-> (fp32 by np.partition + lerp32, float64 by np.partition + lerp64) for one sample"""
    per = x.size
    lo, hi, frac = ranks(per, q)
    v = [np.array([partition_bits(x, r)], dtype=np.uint32).view(np.float32)[0] for r in (lo, hi)]
    return lerp32(v[0], v[1], frac), lerp64(v[0], v[1], frac)


def make_input(kind, N, per, seed=0):
    """float32 [N, per], no NaN"""
    rng = np.random.RandomState(seed + 17 * per)
    if kind.startswith("normal_"):
        x = rng.standard_normal((N, per)) * float(kind.split("_")[1])
    elif kind == "equal":
        x = np.full((N, per), -0.75)
    elif kind == "ties":              # three values, long runs of each: the ranks of every q fall inside or at the edge of a run
        x = rng.choice(np.array([0.5, -0.5, 2.0, -1.25]), size=(N, per))
    elif kind == "zeros_denormals":
        x = rng.choice(np.array([0.0, -0.0, 1e-45, -3e-45, 1e-39, -1e-39, 1.1754944e-38]), size=(N, per))
    elif kind in ("share11", "share21"):      # every value shares its top 11 (21) magnitude bits: levels 1 and 2 (2 alone) decide
        free = 20 if kind == "share11" else 10
        bits = (np.uint32(0x3F9) << np.uint32(20)) | (np.uint32(0x155) << np.uint32(10) if kind == "share21" else np.uint32(0))
        low = rng.randint(0, 1 << free, size=(N, per)).astype(np.uint32)
        sign = rng.randint(0, 2, size=(N, per)).astype(np.uint32) << np.uint32(31)
        return (bits | low | sign).view(np.float32)
    elif kind == "inf":
        x = rng.standard_normal((N, per))
        x[:, ::7] = np.inf
        x[:, 3::11] = -np.inf
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)
