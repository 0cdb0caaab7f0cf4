"""float64 restatement of the forward jump of resampled masked sampling (mmd_renoise_ctr, include/mmd.h), the element-wise bound its fp32
result must keep, and an independent restatement of the schedule walk (masking.repaint_schedule).

The kernel, element i = n * per + r of x [N, F, C, HW] (per = F C HW), level m[n] in [0, T), jump of J levels:
    a = jtab[0][m[n]] = sqrt(ac[m + J] / ac[m]),  b = jtab[1][m[n]] = sqrt(1 - ac[m + J] / ac[m])      (fp32 roundings of float64 values)
    x[i] = a x[i] + b z[i]        z = the counter normal of (element r, draw[n], ids[n], tag)
    m[n] outside [0, T): the sample is not written

The bound comes from the kernel's own arithmetic - two rounded products and one rounded sum, u = 2^-24 the unit roundoff of fp32:
    fl(fl(a x) + fl(b z)) = ((a x)(1 + d1) + (b z)(1 + d2)) (1 + d3),  |d| <= u
    |err| <= 2 u (|a x| + |b z|)(1 + u)
A fused multiply-add drops one of d1 / d2 and only tightens it.

The schedule, restated from the state's point of view rather than as the walk of masking.repaint_schedule: the levels are cut into
blocks of J reverse steps above each jump level m (a multiple of J with m + J <= T - 1); the steps above the highest block run once; each
block then runs U times, with a jump back up between two runs; what is left below the lowest jump level - nothing, as level 0 is one - runs
once.  Draws: visit r of step i is i + r T, the k-th jump 0x80000000 + k."""
import numpy as np

U = 2.0 ** -24
# (N, F, C, HW): the smallest shapes of masked_ref.SMALL - quads straddle a channel, a frame and the sample's end (315 = 4 * 78 + 3),
# audio (F = 1, 1603 = 4 * 400 + 3), samples shorter than a quad, N = 1 and 3
SHAPES = [(3, 3, 3, 35), (1, 3, 3, 35), (3, 1, 1, 1603), (1, 1, 1, 1603), (3, 1, 1, 1), (1, 1, 1, 2), (3, 1, 3, 1), (1, 1, 1, 5)]
JUMP_DRAW = 0x80000000

# (T, J, U): the issue's example first; J = 1, J = T - 1, J that does not divide T - 1, U = 1, long schedules
TRIPLES = [(8, 2, 2), (4, 1, 2), (8, 2, 1), (8, 7, 2), (8, 7, 3), (8, 3, 2), (8, 3, 4), (9, 3, 2), (10, 3, 3), (2, 1, 2), (2, 1, 5), (3, 2, 2),
           (3, 1, 3), (16, 4, 3), (17, 4, 2), (250, 10, 10), (250, 10, 1), (100, 99, 2), (1000, 10, 2), (1, 1, 1)]


def schedule(T, J, U):
    """-> [("step", i, draw) | ("jump", m, draw)] by blocks (see the module's docstring)"""
    if J is None or U == 1:
        return [("step", i, i) for i in range(T - 1, -1, -1)]
    levels = [m for m in range(T) if m % J == 0 and m + J <= T - 1]
    out, k = [], 0
    if not levels:
        return [("step", i, i) for i in range(T - 1, -1, -1)]
    top = max(levels) + J                      # the highest level a jump reaches
    out += [("step", i, i) for i in range(T - 1, top, -1)]
    for m in sorted(levels, reverse=True):
        for r in range(U):
            out += [("step", i, i + r * T) for i in range(m + J, m, -1)]
            if r < U - 1:
                out.append(("jump", m, JUMP_DRAW + k))
                k += 1
    out += [("step", i, i) for i in range(min(levels), -1, -1)]
    return out


def evaluations(T, J, U):
    """The issue's count: T + (U - 1) J |M|"""
    M = [m for m in range(T) if m % J == 0 and m + J <= T - 1]
    return T + (U - 1) * J * len(M)


def alphas_cumprod(name, T):
    """float64 alphas_cumprod of the named schedule (Nichol & Dhariwal 2021), restated"""
    if name == "linear":
        betas = np.linspace(0.0001 * 1000 / T, 0.02 * 1000 / T, T, dtype=np.float64)
    elif name == "cosine":
        f = lambda t: np.cos((t + 0.008) / 1.008 * np.pi / 2) ** 2      # noqa: E731
        betas = np.array([min(1 - f((i + 1) / T) / f(i / T), 0.999) for i in range(T)], dtype=np.float64)
    else:
        raise ValueError(name)
    return np.cumprod(1.0 - betas)


def jump_coef(ac, J):
    """float64 (a [T], b [T]) from alphas_cumprod; zero where m + J > T - 1"""
    T = len(ac)
    a, b = np.zeros(T), np.zeros(T)
    for m in range(T - J):
        ratio = ac[m + J] / ac[m]
        a[m], b[m] = np.sqrt(ratio), np.sqrt(1.0 - ratio)
    return a, b


def make_case(shape, seed=0):
    """x, z: float32 [N, per]"""
    N, F, C, HW = shape
    rng = np.random.RandomState(seed)
    per = F * C * HW
    return rng.standard_normal((N, per)).astype(np.float32), rng.standard_normal((N, per)).astype(np.float32)


def levels(N, T, J):
    """per-sample jump levels of the kernel cases: 0, the highest level a jump may leave, one in between"""
    cyc = (0, T - 1 - J, (T - 1 - J) // 2)
    return np.array([cyc[n % 3] for n in range(N)], dtype=np.int64)


def jump64(x, z, tab, m, defect=None):
    """-> (y float64 [N, per], bound float64 [N, per]); x / z float32 [N, per], tab the fp32 [2, T] table, m the levels.  A level outside
    [0, T) keeps x (bound 0)."""
    tab = np.asarray(tab, dtype=np.float64)
    T = tab.shape[1]
    ok = (m >= 0) & (m < T)
    mm = np.where(ok, m, 0)
    a, b = tab[0][mm], tab[1][mm]
    if defect == "rows_swapped":               # seeded defect: a and b taken from each other's row
        a, b = b, a
    ax, bz = a[:, None] * x.astype(np.float64), b[:, None] * z.astype(np.float64)
    y = np.where(ok[:, None], ax + bz, x.astype(np.float64))
    bound = np.where(ok[:, None], 2.0 * U * (np.abs(ax) + np.abs(bz)) * (1.0 + U), 0.0)
    return y, bound


def emulate32(x, z, tab, m, fused=True, defect=None):
    """The kernel in fp32 numpy: b z rounded, then (fused) a x kept exact - the product of two fp32 values is exact in float64 - in a sum
    that is rounded once, or two rounded products and a rounded sum."""
    tab = np.asarray(tab, dtype=np.float32)
    T = tab.shape[1]
    ok = (m >= 0) & (m < T)
    mm = np.where(ok, m, 0)
    a, b = tab[0][mm], tab[1][mm]
    if defect == "rows_swapped":
        a, b = b, a
    bz = b[:, None] * z
    if fused:
        v = (a[:, None].astype(np.float64) * x.astype(np.float64) + bz.astype(np.float64)).astype(np.float32)
    else:
        v = a[:, None] * x + bz
    assert v.dtype == np.float32
    return np.where(ok[:, None], v, x)


def violations(got, y, bound):
    return int((np.abs(got.astype(np.float64) - y) > bound).sum())
