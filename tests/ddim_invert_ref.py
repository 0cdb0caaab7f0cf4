"""Float64 restatements and error bounds for DDIM inversion (tests/test_ddim_invert_cpu.py, tests/test_ddim_invert_gpu.py).

mmd_slerp (include/mmd.h).  slerp64 is the closed form in float64.  The kernel forms dot, |a|^2, |b|^2 as fp64 sums of exact products, the
weights in fp64, rounds each weight to fp32 once and writes fma(w_a, a, fl(w_b b)).  With u = 2^-24 (fp32 round to nearest) and
e_w = u + W_REL, where W_REL = 1e-12 is the relative allowance on the fp64 weights for the order of the fp64 sums and the fp64 acos / sin
(the sums carry at most per * 2^-53 < 2e-10 relative error only in a worst case that fp64 pairwise sums of 2^11 terms never approach;
the weights' sensitivity to c is at most 1 / sin(theta) <= 32 inside the slerp branch):
    |w_a - W_a| <= e_w |W_a|, |w_b - W_b| <= e_w |W_b|                         W = the float64 weight, w = the kernel's fp32 weight
    p = fl(w_b b):      |p - W_b b| <= |W_b b| (u (1 + e_w) + e_w)              one product rounding
    S = w_a a + p exact inside the fma: |S - y| <= e_w |W_a a| + |W_b b| (u (1 + e_w) + e_w),     y = W_a a + W_b b
    out = fl(S):        |out - S| <= u |S| <= u (|y| + |S - y|)                 one fused add (a separate add of a rounded w_a a would
                                                                                 cost one more u |W_a a|: the kernel spells the fma out)
    |out - y| <= (1 + u) (e_w |W_a a| + |W_b b| (u (1 + e_w) + e_w)) + u |y| + 2^-149           (the last term: a subnormal result)
The bound assumes the kernel and the reference take the same branch: the test inputs keep |c| < 0.99 or |c| > 0.99999 (branch_margin_ok).

The zero-head recursion.  With the model's output exactly zero, encode step i (mmd_ddim_update, flag 8, eps prediction, no clipping) is, in
the kernel's order with the fp32 table values cr = sqrt(1 / ac[i]), crm1 = sqrt(1 / ac[i] - 1), an = ac[i + 1]:
    x0  = fl(cr x)                                  (cr x - crm1 0: whichever product the compiler fuses, the other term is an exact zero)
    eps = (cr x - x0) / crm1                        separate: fl(cr x) - x0 = 0;  contracted to fma(cr, x, -x0): the exact rounding residual
                                                    rho of the product, |rho| <= u |cr x|, so |eps| <= u |cr x| / crm1 (1 + u)
    res = x0 sqrtf(an) + sqrtf(1 - an) eps          two roundings at most on the first term (product, add), sqrtf within one ulp
The float64 reference recursion is y <- y cr sa with sa = sqrt(an) in float64 of the fp32 an; the bound is carried step by step:
    e' = cr sa e + (|y| + e) cr (5 u sa + sb u / crm1) (1 + 8 u) + 2^-149,      sb = sqrt(1 - an) (1 + 2 u)
5 u sa: one u for x0's rounding, two for sqrtf(an) against the float64 root (its own rounding and the root's), two for the product and the
add of the result; sb u / crm1: the eps term above, which a run cannot tell us about - it follows from the contraction the compiler may
apply."""
import numpy as np

U = 2.0 ** -24
W_REL = 1e-12
SWITCH = 0.9995
TINY = 2.0 ** -149

PERS = (1, 5, 1023, 1024, 1025, 3 * 8 * 8 * 4)
NS = (1, 3)
SEED = 20261021


# ----------------------------------------------------------------------------- slerp
def cosine64(a, b):
    """(c clamped, na nb) per row in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dot, na, nb = (a * b).sum(1), (a * a).sum(1), (b * b).sum(1)
    den = na * nb
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(den != 0, np.clip(dot / np.sqrt(np.where(den != 0, den, 1.0)), -1.0, 1.0), 0.0)
    return c, den


def weights64(a, b, lam):
    """the float64 weights (W_a, W_b) [N] of mmd_slerp's definition"""
    lam = np.asarray(lam, np.float64)
    c, den = cosine64(a, b)
    chord = (den == 0) | (np.abs(c) > SWITCH)
    theta = np.arccos(np.where(chord, 0.0, c))          # (any angle with sin != 0 where the chord is taken)
    s = np.sin(theta)
    return np.where(chord, 1.0 - lam, np.sin((1.0 - lam) * theta) / s), np.where(chord, lam, np.sin(lam * theta) / s)


def slerp64(a, b, lam):
    """closed-form float64 slerp of the rows of a, b [N, per] at lam [N] -> (y, W_a, W_b)"""
    wa, wb = weights64(a, b, lam)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return wa[:, None] * a + wb[:, None] * b, wa, wb


def combine_bound(a, b, wa, wb, y):
    """the per-element bound on |out - y| derived in the module docstring"""
    ea = np.abs(wa[:, None] * np.asarray(a, np.float64))
    eb = np.abs(wb[:, None] * np.asarray(b, np.float64))
    e_w = U + W_REL
    return (1 + U) * (e_w * ea + eb * (U * (1 + e_w) + e_w)) + U * np.abs(y) + TINY


def violations(got, want, bound):
    got = np.asarray(got, np.float64)
    return int((~(np.abs(got - want) <= bound)).sum())          # a NaN counts


def branch_margin_ok(a, b):
    """every row sits well inside one branch: |c| < 0.99 (slerp), |c| > 0.99999 or a zero row (chord)"""
    c, den = cosine64(a, b)
    return bool(np.all((den == 0) | (np.abs(c) < 0.99) | (np.abs(c) > 0.99999)))


def _round_sum32(P, p):
    """fl32(P + p) with ONE rounding for float64 P (an exact product of two fp32 values) and p: the fma's result.  s = fl64(P + p) and its
    exact error r (TwoSum) give the true sum s + r; rounding s to fp32 differs from rounding s + r only where s sits exactly on a midpoint
    of two fp32 neighbours (midpoints are float64 numbers and rounding is monotonic), and there r decides the side."""
    s = P + p
    t = s - P
    r = (P - (s - t)) + (p - t)
    f = s.astype(np.float32)
    d = s - f.astype(np.float64)
    other = np.nextafter(f, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)), dtype=np.float32)
    tie = (d != 0) & (s == (f.astype(np.float64) + other.astype(np.float64)) / 2) & (r != 0)
    return np.where(tie & (np.sign(r) == np.sign(d)), other, f).astype(np.float32)


def emulate(a, b, lam, defect=None, prefill=0.0):
    """The kernel in numpy: fp64 sums of the fp32 data, fp64 weights rounded to fp32 once, out = fl(w_a a + fl(w_b b)) with the fused add
    rounded once (_round_sum32).  defect seeds one fault:
      "range"        the sums miss the last quarter of every row
      "no_guard"     c reaches acos as computed, without the clamp and the |c| test in front of it (with the test in place the clamp is
                     never the last guard: "no_clamp" alone changes no bit, which the CPU test asserts as well)
      "no_clamp"     the clamp alone is missing
      "swap"         w_a and w_b change places
      "tail"         the last element of every row is not written (stays `prefill`)"""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    a64, b64, lam64 = a32.astype(np.float64), b32.astype(np.float64), np.asarray(lam, np.float32).astype(np.float64)
    per = a32.shape[1]
    hi = per - per // 4 if defect == "range" else per
    dot, na, nb = (a64[:, :hi] * b64[:, :hi]).sum(1), (a64[:, :hi] ** 2).sum(1), (b64[:, :hi] ** 2).sum(1)
    den = na * nb
    wa, wb = 1.0 - lam64, lam64.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in range(a32.shape[0]):
            if den[n] == 0:
                continue
            c = dot[n] / np.sqrt(den[n])
            if defect not in ("no_guard", "no_clamp"):
                c = min(max(c, -1.0), 1.0)
            if defect != "no_guard" and abs(c) > SWITCH:
                continue
            theta = np.arccos(c)
            s = np.sin(theta)
            wa[n], wb[n] = np.sin((1.0 - lam64[n]) * theta) / s, np.sin(lam64[n] * theta) / s
    if defect == "swap":
        wa, wb = wb, wa
    wa32, wb32 = wa.astype(np.float32), wb.astype(np.float32)
    with np.errstate(invalid="ignore"):
        p = (wb32[:, None] * b32).astype(np.float32)          # fp32 x fp32 rounded once
        out = _round_sum32(wa32[:, None].astype(np.float64) * a64, p.astype(np.float64))
    if defect == "tail":
        out[:, -1] = prefill
    return out


def slerp_case(N, per, kind="random", seed=SEED):
    """fp32 inputs (a, b, lam) of one kernel case.  random: independent normal rows (|c| ~ 1 / sqrt(per), or exactly +-1 at per = 1, both
    far from the switch; rows at per = 5 are redrawn until |c| < 0.9); same: b = a; opposite: b = -a; zero: the first row of a is zero."""
    rng = np.random.default_rng(seed + 7919 * N + per)
    a = rng.standard_normal((N, per)).astype(np.float32)
    b = rng.standard_normal((N, per)).astype(np.float32)
    for _ in range(100):
        c, _ = cosine64(a, b)
        bad = (np.abs(c) >= 0.9) & (np.abs(c) <= 0.99999)
        if not bad.any():
            break
        b[bad] = rng.standard_normal((int(bad.sum()), per)).astype(np.float32)
    lam = rng.uniform(0.05, 0.95, N).astype(np.float32)
    if kind == "same":
        b = a.copy()
    elif kind == "opposite":
        b = -a
    elif kind == "zero":
        a[0] = 0.0
    elif kind != "random":
        raise ValueError(kind)
    return a, b, lam


# ----------------------------------------------------------------------------- levels
def encode_indices(T, to_level=None):
    to_level = T - 1 if to_level is None else to_level
    assert 1 <= to_level <= T - 1
    return list(range(to_level))


def decode_indices(T, from_level=None):
    from_level = T - 1 if from_level is None else from_level
    assert 0 <= from_level <= T - 1
    return list(range(from_level, -1, -1))


# ----------------------------------------------------------------------------- the zero-head recursion
def zero_head_encode(x, alphas_cumprod, to_level):
    """x [.. any shape] fp32 level-0 state, alphas_cumprod float64 [T] -> (y, bound) after encode steps 0 ... to_level - 1 with a model
    that returns exactly zero: the float64 recursion on the fp32 table values and the carried bound of the module docstring."""
    ac = np.asarray(alphas_cumprod, np.float64)
    cr_t = np.sqrt(1.0 / ac).astype(np.float32).astype(np.float64)
    crm1_t = np.sqrt(1.0 / ac - 1.0).astype(np.float32).astype(np.float64)
    an_t = np.append(ac[1:], 0.0).astype(np.float32).astype(np.float64)
    y = np.asarray(x, np.float32).astype(np.float64)
    e = np.zeros_like(y)
    for i in range(to_level):
        cr, crm1, an = cr_t[i], crm1_t[i], an_t[i]
        sa, sb = np.sqrt(an), np.sqrt(1.0 - an) * (1 + 2 * U)
        e = cr * sa * e + (np.abs(y) + e) * cr * (5 * U * sa + sb * U / crm1) * (1 + 8 * U) + TINY
        y = y * cr * sa
    return y, e
