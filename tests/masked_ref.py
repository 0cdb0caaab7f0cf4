"""float64 restatement of mmd_cond_replace (include/mmd.h) and the element-wise bound its fp32 result must keep.

The kernel, element i = n * per + r of x [N, F, C, HW] (per = F C HW):
    f = r // (C HW),  c = (r // HW) % C,  p = r % HW          the element's frame, channel, position
    cell = mask[n * mask_stride + f * HW + p]                   one cell per (frame, position), shared by the channels
    cell set:  x[i] = A[n] known[i] + B[n] eps[i]               A, B = tab2[t[n]], tab2[T + t[n]]  (or the host scalars)
    else:      x[i] is not written

The bound comes from the kernel's own arithmetic - two rounded products and one rounded sum, u = 2^-24 the unit roundoff of fp32:
    fl(fl(A k) + fl(B e)) = ((A k)(1 + d1) + (B e)(1 + d2)) (1 + d3),  |d| <= u
    |err| <= u (|A k| + |B e|) + u (|A k| + |B e|)(1 + u) <= 2 u (|A k| + |B e|)(1 + u)
A fused multiply-add drops one of d1 / d2 and only tightens it.  Unknown cells have no error to bound: they keep x bit for bit."""
import numpy as np

U = 2.0 ** -24
T_CYCLE = (0, -1, 7)          # per-sample timesteps of the cases: 0, T - 1, 7, ...

# (N, F, C, HW): quads straddle a mask row, a channel, a frame and the sample's end; audio (F = 1); samples shorter than a quad
VIDEO, AUDIO = (3, 3, 3, 35), (2, 1, 1, 1603)
SMALL = [VIDEO, AUDIO, (2, 1, 1, 1), (2, 1, 1, 2), (3, 1, 3, 1), (2, 1, 1, 5)]
# past the 4096 x 256 grid cap, so the grid-stride loop runs twice: elements (memory form), quads (counter form)
BIG_MEMORY, BIG_COUNTER = (2, 3, 3, 58563), (2, 1, 1, 2100001)
MASKS = [("null", False), ("ones", False), ("ones", True), ("zeros", False), ("zeros", True), ("random", False), ("random", True),
         ("last", False), ("last", True)]


def timesteps(N, T):
    return np.array([T_CYCLE[n % 3] % T for n in range(N)], dtype=np.int64)


def make_mask(kind, per_sample, shape, seed=0):
    """-> (uint8 [rows, F*HW] or None, mask_stride): rows = N for a per-sample mask, 1 for a batch-shared one."""
    N, F, _, HW = shape
    if kind == "null":
        return None, 0
    rows = N if per_sample else 1
    rng = np.random.RandomState(1000 + seed)
    if kind == "ones":
        m = np.ones((rows, F * HW), dtype=np.uint8)
    elif kind == "zeros":
        m = np.zeros((rows, F * HW), dtype=np.uint8)
    elif kind == "random":
        m = (rng.rand(rows, F * HW) < 0.5).astype(np.uint8) * rng.randint(1, 256, size=(rows, F * HW)).astype(np.uint8)      # non-zero = known
    elif kind == "last":
        m = np.zeros((rows, F * HW), dtype=np.uint8)
        m[-1, -1] = 1
    else:
        raise ValueError(kind)
    return m, (F * HW if per_sample else 0)


def make_case(shape, seed=0):
    """x, known, eps: float32 [N, per]"""
    N, F, C, HW = shape
    rng = np.random.RandomState(seed)
    per = F * C * HW
    return tuple(rng.standard_normal((N, per)).astype(np.float32) * s for s in (1.0, 0.5, 1.0))


def known_cells(shape, mask, stride, defect=None):
    """bool [N, per]: the elements the kernel replaces, from the flat index as the kernel derives it"""
    N, F, C, HW = shape
    per = F * C * HW
    r = np.arange(per, dtype=np.int64)
    f, c, p = r // (C * HW), (r // HW) % C, r % HW
    if mask is None:
        return np.ones((N, per), dtype=bool)
    flat = np.asarray(mask, dtype=np.uint8).reshape(-1)
    cell = f * HW + p
    if defect == "channel_in_cell":                    # seeded defect: the element's own offset taken for its cell
        cell = ((f * C + c) * HW + p) % (F * HW)
    if defect == "batch_stride_ignored":               # seeded defect: every sample reads the first sample's cells
        stride = 0
    n = np.arange(N, dtype=np.int64)[:, None]
    return flat[n * stride + cell[None, :]] != 0


def replace64(x, known, eps, shape, mask, stride, A, B, defect=None):
    """-> (y float64 [N, per], on bool [N, per], bound float64 [N, per]); x / known / eps float32 [N, per], A / B the per-sample
    coefficients (fp32 values).  Off the known cells y = x and the bound is 0."""
    A, B = np.asarray(A, dtype=np.float64).reshape(-1), np.asarray(B, dtype=np.float64).reshape(-1)
    if defect == "t_of_sample_0":                      # seeded defect: one timestep for the whole batch
        A, B = np.full_like(A, A[0]), np.full_like(B, B[0])
    on = known_cells(shape, mask, stride, defect)
    ak, be = A[:, None] * known.astype(np.float64), B[:, None] * eps.astype(np.float64)
    y = np.where(on, ak + be, x.astype(np.float64))
    bound = np.where(on, 2.0 * U * (np.abs(ak) + np.abs(be)) * (1.0 + U), 0.0)
    return y, on, bound


def emulate32(x, known, eps, shape, mask, stride, A, B, fused=False, defect=None):
    """The kernel in fp32 numpy: two rounded products and a rounded sum, or (fused) one product kept exact - the product of two
    fp32 values is exact in float64 - in the sum that is rounded once."""
    A32, B32 = np.asarray(A, dtype=np.float32).reshape(-1), np.asarray(B, dtype=np.float32).reshape(-1)
    if defect == "t_of_sample_0":
        A32, B32 = np.full_like(A32, A32[0]), np.full_like(B32, B32[0])
    on = known_cells(shape, mask, stride, defect)
    be = B32[:, None] * eps
    if fused:
        v = (A32[:, None].astype(np.float64) * known.astype(np.float64) + be.astype(np.float64)).astype(np.float32)
    else:
        v = A32[:, None] * known + be
    assert v.dtype == np.float32
    return np.where(on, v, x)


def violations(got, y, bound):
    return int((np.abs(got.astype(np.float64) - y) > bound).sum())


def qtab(T=1000):
    """q_sample's [2, T] fp32 table of the linear schedule, as GaussianDiffusion.device_tables builds it"""
    betas = np.linspace(0.0001, 0.02, T, dtype=np.float64) * (1000 / T)
    ac = np.cumprod(1.0 - betas)
    return np.stack([np.sqrt(ac), np.sqrt(1.0 - ac)]).astype(np.float32)
