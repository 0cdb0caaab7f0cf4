"""float64 restatement of the stochastic data-prediction multistep solver (SDE-DPM-Solver++, orders 1 and 2): its coefficients on a
float64 schedule, the update mmd_dpmpp_sde_update performs (include/mmd.h), the table-driven loop DPM_Solver.sample_graph_sde drives with
it, and the bounds the fp32 results must keep.  Shared by tests/test_dpm_sde_cpu.py and tests/test_dpm_sde_gpu.py (test infrastructure).

The method, per stream: s -> t, lambda = log(alpha / sigma), h = lambda_t - lambda_s > 0, E = -expm1(-2 h), m0 the data prediction at s, m1 the
one of the evaluation before, z ~ N(0, I):
    x_t = c0 x_s + c1 m0 + c2 m1 + cz z,   c0 = (sigma_t / sigma_s) e^-h,  cm = alpha_t E,  cz = sigma_t sqrt(E)
    first order: c1 = cm, c2 = 0;   second order, r0 = (lambda_s - lambda_prev) / h: c1 = cm (1 + 1 / (2 r0)), c2 = -cm / (2 r0)
    (I1) c0 alpha_s + c1 + c2 = alpha_t          (I2) c0^2 sigma_s^2 + cz^2 = sigma_t^2

Bound of the update kernel (u = 2^-24, the unit roundoff of fp32; all inputs are fp32 values, so the float64 restatement has errors of
2^-53 relative, which the (1 + u) factors below absorb).  The kernel forms, in this order,
    v1 = fl(c0 x)  v2 = fma(c1, m0, v1)  [kind 1: v3 = fma(c2, M1, v2)]  v = fma(cz, z, v_last)
one rounded product and n - 1 fused multiply-adds, each one rounding: n = 3 operations at kind 0, n = 4 at kind 1.  Every term passes
through at most n roundings, so
    |v - sum_i c_i v_i| <= ((1 + u)^n - 1) sum_i |c_i v_i|.
With thresholding m0 = clamp_scale(m0raw, s): sn = max(s, 1) and the clamp are exact, d = fl(sn / max_val) and m0 = fl(clamp / d) are one
correctly rounded division each (the library is built without fast-math), so m0 = m0_64 (1 + e), |e| <= EM = 2 u / (1 - u); that error
rides the c1 term through its n - 1 fmas and adds |c1 m0_64| EM (1 + u)^n.  The denoise row (kind 2) copies: |x - m0_64| <= |m0_64| EM, and
so does the history: |M1 - m0_64| <= |m0_64| EM.  Without thresholding EM = 0 and M1, the denoise row are exact.

Bound of the tables (sde_tables / _sde_coefs against (I1) and (I2)).  _sde_coefs takes the fp32 values lam~, la~, sig~ that
DPM_Solver._sc() delivers, widens them and works in float64 (errors of 2^-53 relative, absorbed below), and rounds c0, c1, c2, cz to fp32
once: a relative error of u each.  (I2) holds for ANY lam, sig - e^-2h cancels - so with sig_s = sig~_s, sig_t = sig~_t
    |c0^2 sig_s^2 + cz^2 - sig_t^2| <= ((1 + u)^2 - 1)(c0^2 sig_s^2 + cz^2).
(I1) with alpha = exp(la~) holds when e^-h = (alpha_s sig_t) / (sig_s alpha_t), i.e. when lam~ = la~ - log sig~ exactly.  The fp32
schedule computes w = fl(1 - fl(exp(fl(2 la~)))) ONCE per time in both marginal_std and marginal_lambda (the same operations on the same
value), sig~ = fl(sqrt(w)) (correctly rounded: log sig~ = log(w) / 2 + e, |e| <= u / (1 - u)) and lam~ = fl(la~ - fl(0.5 fl(log w))) with a
logf of at most 1 ulp = 2 u relative (glibc, SLEEF u10), so
    |lam~ - (la~ - log sig~)| <= DL(tau) = u / (1 - u) + 2 u |log sig~| (1 + u) + u |lam~|
and e^-h is off by a factor e^d, |d| <= D = DL(s) + DL(t).  Then c0 alpha_s + cm - alpha_t = alpha_t rho^2 e^d (1 - e^d) with rho the
consistent e^-h, at most alpha_t e^(-2 h + 2 D) (e^D - 1) in magnitude with the h of lam~.  c1 + c2 = cm up to float64 rounding.  So
    |c0 alpha_s + c1 + c2 - alpha_t| <= u (|c0| alpha_s + |c1| + |c2|) + alpha_t e^(-2 h + 2 D) (e^D - 1)."""
import numpy as np

import seeded_ref as S

U = 2.0 ** -24
EM = 2.0 * U / (1.0 - U)
FIRST, SECOND, DENOISE = 0, 1, 2

# the kernel cases of the GPU tests: N F C HW with 6147 elements a sample (a ragged last quad, and unaligned samples 1 and 2)
N, F, C, HW = 3, 3, 3, 683
PER = F * C * HW
CASES = [(cmf, with_s) for cmf in (1, 2) for with_s in (True, False)]
# one table row of each kind and a second second-order row; the denoise row's cz is NOT zero: the kernel must not read it
TAB_C0 = np.array([0.99, 0.61, 5.0, 0.14], dtype=np.float32)
TAB_C1 = np.array([0.043, 1.325, 5.0, 0.426], dtype=np.float32)
TAB_C2 = np.array([7.0, -0.4417, 5.0, -0.142], dtype=np.float32)          # row 0 is first order: its c2 must not be applied
TAB_KIND = np.array([FIRST, SECOND, DENOISE, SECOND], dtype=np.float32)
TAB_CZ = np.array([0.9885, 0.4262, 3.0, 0.0682], dtype=np.float32)
ROWS = 4
K_CASES = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 2), (3, 2, 0)]
S_VALUES = np.array([0.4, 1.3, 2.9], dtype=np.float32)
MAX_VAL = 1.5
SEED, IDS = 0x1234ABCD5678, (11, 2 ** 32 - 1, 7)          # sample id 7 is row 2 of 3
DEFECTS = ["noise_dropped", "cz_next_row", "c2_at_first", "noise_at_denoise", "m1_before_clamp", "draw_k0"]


# ----------------------------------------------------------------------------- the float64 schedule and coefficients
def alphas_cumprod(kind, T=1000):
    """float64 alphas_cumprod of the 'linear' and 'cosine' beta schedules (Ho et al. 2020; Nichol & Dhariwal 2021)."""
    if kind == "linear":
        betas = np.linspace(1e-4, 0.02, T, dtype=np.float64) * (1000 / T)
    elif kind == "cosine":
        f = lambda t: np.cos((t + 0.008) / 1.008 * np.pi / 2) ** 2      # noqa: E731
        i = np.arange(T, dtype=np.float64)
        betas = np.minimum(1 - f((i + 1) / T) / f(i / T), 0.999)
    else:
        raise ValueError(kind)
    return np.cumprod(1.0 - betas)


class Schedule64:
    """The 'discrete' VP schedule in float64: log alpha known at t_i = (i + 1) / T, linear in between."""

    def __init__(self, ac):
        self.T = len(ac)
        self.t = np.arange(1, self.T + 1, dtype=np.float64) / self.T
        self.la_knots = 0.5 * np.log(np.asarray(ac, dtype=np.float64))

    def la(self, t):
        return np.interp(t, self.t, self.la_knots)

    def sigma(self, t):
        return np.sqrt(-np.expm1(2.0 * self.la(t)))

    def lam(self, t):
        return self.la(t) - np.log(self.sigma(t))

    def t_of_lam(self, lam):
        la = -0.5 * np.logaddexp(0.0, -2.0 * lam)
        return np.interp(la, self.la_knots[::-1], self.t[::-1])

    def grid(self, skip_type, steps):
        t_T, t_0 = 1.0, 1.0 / self.T
        if skip_type == "logSNR":
            return self.t_of_lam(np.linspace(self.lam(t_T), self.lam(t_0), steps + 1))
        if skip_type == "time_uniform":
            return np.linspace(t_T, t_0, steps + 1)
        if skip_type == "time_quadratic":
            return np.linspace(t_T ** 0.5, t_0 ** 0.5, steps + 1) ** 2
        raise ValueError(skip_type)


def coefs64(lam_prev, lam_s, lam_t, alpha_t, sig_s, sig_t):
    """(c0, c1, c2, cz) in float64 from the formulas of the module docstring; lam_prev None: first order."""
    h = lam_t - lam_s
    E = -np.expm1(-2.0 * h)
    c0, cm, cz = sig_t / sig_s * np.exp(-h), alpha_t * E, sig_t * np.sqrt(E)
    if lam_prev is None:
        return c0, cm, 0.0, cz
    r0 = (lam_s - lam_prev) / h
    return c0, cm * (1.0 + 1.0 / (2.0 * r0)), -cm / (2.0 * r0), cz


def schedule_rows64(sch, skip_type, steps, order):
    """Per update row i of a grid: (alpha_s, sigma_s, alpha_t, sigma_t, (c0, c1, c2, cz)) on the float64 schedule."""
    g = sch.grid(skip_type, steps)
    out = []
    for i in range(steps):
        second = order == 2 and i > 0
        c = coefs64(sch.lam(g[i - 1]) if second else None, sch.lam(g[i]), sch.lam(g[i + 1]), np.exp(sch.la(g[i + 1])), sch.sigma(g[i]),
                    sch.sigma(g[i + 1]))
        out.append((np.exp(sch.la(g[i])), sch.sigma(g[i]), np.exp(sch.la(g[i + 1])), sch.sigma(g[i + 1]), c))
    return out


def dl(lam32, sig32):
    """DL of the module docstring: how far the fp32 lambda may lie from la~ - log sig~."""
    return U / (1.0 - U) + 2.0 * U * abs(np.log(float(sig32))) * (1.0 + U) + U * abs(float(lam32))


def table_bounds(c, alpha_s, alpha_t, sig_s, lam_s, lam_t, sig_t):
    """(bound of I1, bound of I2) for a table row c = (c0, c1, c2, cz) (fp32 values) and the fp32 schedule values of its two times,
    all widened to float64; alpha = exp(la~)."""
    c0, c1, c2, cz = (float(v) for v in c)
    D = dl(lam_s, sig_s) + dl(lam_t, sig_t)
    h = float(lam_t) - float(lam_s)
    b1 = U * (abs(c0) * alpha_s + abs(c1) + abs(c2)) + alpha_t * np.exp(-2.0 * h + 2.0 * D) * np.expm1(D)
    b2 = ((1.0 + U) ** 2 - 1.0) * (c0 ** 2 * float(sig_s) ** 2 + cz ** 2)
    return b1, b2


# ----------------------------------------------------------------------------- the update
def clamp_scale64(m0raw, s, max_val):
    """float64 clamp(m0raw, -sn, sn) max_val / sn, sn = max(s[n], 1); m0raw [N, per], s fp32 [N] or None."""
    m = m0raw.astype(np.float64)
    if s is None:
        return m
    sn = np.maximum(np.asarray(s, dtype=np.float64), 1.0)[:, None]
    return np.clip(m, -sn, sn) * (float(max_val) / sn)


def update64(x, m0raw, m1, z, tab, cz, k, s=None, max_val=1.0):
    """The update in float64.  x, m0raw (the first C channels of the model output), m1, z: [N, per] (fp32 or float64 values); tab fp32
    [6, rows], cz fp32 [rows], k int [N].  -> (y, M1 out, bound of y, bound of M1 out), float64 [N, per]; a k outside the table leaves
    x and m1 (bounds 0)."""
    x, m1, z = (np.asarray(a, dtype=np.float64) for a in (x, m1, z))
    m0 = clamp_scale64(np.asarray(m0raw), s, max_val)
    em = EM if s is not None else 0.0
    y, mo, by, bm = x.copy(), m1.copy(), np.zeros_like(x), np.zeros_like(x)
    rows = tab.shape[1]
    for n, kn in enumerate(int(v) for v in k):
        if not 0 <= kn < rows:
            continue
        c0, c1, c2, kind = (float(tab[j, kn]) for j in (2, 3, 4, 5))
        mo[n], bm[n] = m0[n], np.abs(m0[n]) * em
        if int(kind) == DENOISE:
            y[n], by[n] = m0[n], np.abs(m0[n]) * em
            continue
        terms = [c0 * x[n], c1 * m0[n]] + ([c2 * m1[n]] if int(kind) == SECOND else []) + [float(cz[kn]) * z[n]]
        nops = len(terms)
        y[n] = sum(terms)
        by[n] = ((1.0 + U) ** nops - 1.0) * sum(np.abs(t) for t in terms) + np.abs(terms[1]) * em * (1.0 + U) ** nops
    return y, mo, by, bm


def _fma32(c, t, v):
    """fl32(c t + v) for fp32 arrays: the product of two fp32 values is exact in float64."""
    return (np.float64(c) * t.astype(np.float64) + v.astype(np.float64)).astype(np.float32)


def emulate32(x, m0raw, m1, z, tab, cz, k, s=None, max_val=1.0, defect=None, z_k0=None):
    """The kernel's term order in fp32 numpy -> (x out, M1 out) fp32.  defect: one of DEFECTS; z_k0: the noise drawn at k[0] for every
    sample (what "draw_k0" reads instead of z)."""
    x, m0raw, m1, z = (np.asarray(a, dtype=np.float32) for a in (x, m0raw, m1, z))
    m0 = m0raw.copy()
    if s is not None:
        sn = np.maximum(np.asarray(s, dtype=np.float32), np.float32(1.0))[:, None]
        m0 = (np.clip(m0, -sn, sn) / (sn / np.float32(max_val))).astype(np.float32)
    if defect == "draw_k0":
        z = np.asarray(z_k0, dtype=np.float32)
    y, mo = x.copy(), m1.copy()
    rows = tab.shape[1]
    for n, kn in enumerate(int(v) for v in k):
        if not 0 <= kn < rows:
            continue
        c0, c1, c2 = (np.float32(tab[j, kn]) for j in (2, 3, 4))
        kind = int(tab[5, kn])
        czk = np.float32(cz[(kn + 1) % rows] if defect == "cz_next_row" else cz[kn])
        mo[n] = m0raw[n] if defect == "m1_before_clamp" else m0[n]
        if kind == DENOISE:
            y[n] = _fma32(czk, z[n], m0[n]) if defect == "noise_at_denoise" else m0[n]
            continue
        v = _fma32(c1, m0[n], c0 * x[n])
        if kind == SECOND or defect == "c2_at_first":
            v = _fma32(c2, m1[n], v)
        y[n] = v if defect == "noise_dropped" else _fma32(czk, z[n], v)
    return y, mo


def violations(got, want, bound):
    return int((np.abs(np.asarray(got, dtype=np.float64) - want) > bound).sum())


def make_case(cm_factor, with_s, seed=0):
    """The inputs of one kernel case -> dict of numpy arrays: x, m1 fp32 [N, per]; mo fp32 [N, F, Cm, HW] (the model output; the
    variance channels of Cm = 2C hold large values that must not be read); tab fp32 [6, 4]; cz fp32 [4]; s fp32 [N] or None."""
    rng = np.random.RandomState(100 + seed)
    x = rng.standard_normal((N, PER)).astype(np.float32)
    m1 = rng.standard_normal((N, PER)).astype(np.float32)
    mo = (rng.standard_normal((N, F, C * cm_factor, HW)) * 1.5).astype(np.float32)
    if cm_factor == 2:
        mo[:, :, C:] += 1000.0
    tab = np.zeros((6, ROWS), dtype=np.float32)
    tab[0], tab[1] = 1.7, -1.3          # cx, ce: the update must not read them
    tab[2], tab[3], tab[4], tab[5] = TAB_C0, TAB_C1, TAB_C2, TAB_KIND
    return dict(x=x, m1=m1, mo=mo, m0raw=np.ascontiguousarray(mo[:, :, :C]).reshape(N, PER), tab=tab, cz=TAB_CZ.copy(),
                s=S_VALUES.copy() if with_s else None, max_val=MAX_VAL)


def counter_noise64(k, tag, ids=IDS, seed=SEED, per=PER):
    """float64 [N, per]: the counter normals of the samples `ids` at draw k[n] (a k outside 32 bits is taken modulo 2^32, as the
    kernel takes the low word)."""
    return np.stack([S.normals(seed, sid, int(kn) & 0xFFFFFFFF, tag, per) for sid, kn in zip(ids, k)])


# ----------------------------------------------------------------------------- the table-driven loop
def run(tabs, data_fn, x_T, noise_fn, stream="video"):
    """sample_graph_sde's loop for one stream in float64: tabs = sde_tables' dictionary (or any with "rows", "tab", "cz"), data_fn(x, i) the
    (thresholded) data prediction of evaluation i, noise_fn(i) the z of update row i -> the final state.  Kinds as the kernel reads them."""
    tab, cz = tabs["tab"][stream].astype(np.float64), tabs["cz"][stream].astype(np.float64)
    x, m1 = np.asarray(x_T, dtype=np.float64), None
    for i in range(tabs["rows"]):
        m0 = np.asarray(data_fn(x, i), dtype=np.float64)
        kind = int(tab[5, i])
        if kind == DENOISE:
            x = m0
        else:
            x = tab[2, i] * x + tab[3, i] * m0 + (tab[4, i] * m1 if kind == SECOND else 0.0) + cz[i] * np.asarray(noise_fn(i), dtype=np.float64)
        m1 = m0
    return x


# ----------------------------------------------------------------------------- marginal preservation
M_N, M_ROWS, M_SEED, M_TAG = 4, 8, 20221102, 0
M_IDS = (0, 1, 2, 3)
_MARGINAL = {}


def marginal_case():
    """One stream of M_N x PER elements carried through 8 first-order rows of a logSNR grid with a perfect data prediction m0 = mu:
    x_0 = alpha mu + sigma eps at row 0 (eps = the counter's x_T draw), z of row i = the counter normal at draw i.  -> dict with the
    fp32 table / cz / x_0 / mu the kernel gets, the float64 result `want` of the SAME fp32 inputs with the float64 Box-Muller normals,
    the carried bound, and alpha_t, sigma_t at the end.

    The carried bound: the kernel's x_i differs from the float64 x_i by e_i (e_0 = 0: x_0 is an input), its normals from the float64
    ones by at most K u |z64| element by element (tests/test_seeded_gpu.py: K), so after a row
        e_(i+1) = (|c0| e_i + |cz| K u |z64|)(1 + u)^3 + ((1 + u)^3 - 1)(|c0| (|x_i| + e_i) + |c1 mu| + |cz z64| (1 + K u))
    - the update's own bound evaluated on the values the kernel may hold."""
    if _MARGINAL:
        return _MARGINAL
    from test_seeded_gpu import K
    sch = Schedule64(alphas_cumprod("linear"))
    rows = schedule_rows64(sch, "logSNR", M_ROWS, 1)
    tab = np.zeros((6, M_ROWS), dtype=np.float32)
    cz = np.zeros(M_ROWS, dtype=np.float32)
    for i, (_, _, _, _, c) in enumerate(rows):
        tab[2, i], tab[3, i], tab[4, i], cz[i] = c
    rng = np.random.RandomState(5)
    mu = rng.uniform(-1.0, 1.0, size=(M_N, PER)).astype(np.float32)
    eps = np.stack([S.normals(M_SEED, sid, S.X_T, M_TAG, PER) for sid in M_IDS])
    x0 = (rows[0][0] * mu + rows[0][1] * eps).astype(np.float32)
    x, e = x0.astype(np.float64), np.zeros((M_N, PER))
    g = (1.0 + U) ** 3
    for i in range(M_ROWS):
        z = np.stack([S.normals(M_SEED, sid, i, M_TAG, PER) for sid in M_IDS])
        c0, c1, czi = float(tab[2, i]), float(tab[3, i]), float(cz[i])
        local = (g - 1.0) * (abs(c0) * (np.abs(x) + e) + np.abs(c1 * mu) + np.abs(czi * z) * (1.0 + K * U))
        e = (abs(c0) * e + abs(czi) * K * U * np.abs(z)) * g + local
        x = c0 * x + c1 * mu.astype(np.float64) + czi * z
    _MARGINAL.update(tab=tab, cz=cz, x0=x0, mu=mu, want=x, bound=e, alpha_t=rows[-1][2], sigma_t=rows[-1][3])
    return _MARGINAL


def marginal_scores(x, mu, alpha_t, sigma_t):
    """|statistic - expectation| / standard error of the mean and the variance of r = x - alpha_t mu over all n elements, which a
    marginal-preserving solver leaves N(0, sigma_t^2): se(mean) = sigma_t / sqrt(n), se(var) = sigma_t^2 sqrt(2 / n)."""
    r = (np.asarray(x, dtype=np.float64) - alpha_t * np.asarray(mu, dtype=np.float64)).reshape(-1)
    n = r.size
    return abs(r.mean()) / (sigma_t / np.sqrt(n)), abs(r.var() - sigma_t ** 2) / (sigma_t ** 2 * np.sqrt(2.0 / n))
