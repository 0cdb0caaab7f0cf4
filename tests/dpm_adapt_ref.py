"""Numpy float64 restatement of the device controller of DPM_Solver.sample_graph_adaptive (include/mmd.h: mmd_dpm_adapt_control), of the
order in which mmd_dpm_adapt_close sums its error terms, of mmd_dpm_adapt_commit, and of the whole loop; and the comparisons the GPU tests
make between the device and this restatement (compare_control, compare_partials, compare_commit), so that the CPU tests can show each of
them flagging a seeded defect.

`defect` names one deliberate deviation: "E_not_fp32", "h_not_capped", "prev_on_reject", "chunk_order", "s1_at_h"."""
import numpy as np

CHUNK = 4096
REJECT, ACCEPT, IDLE = 0, 1, 2
F32 = np.float32


class Schedule:
    """The discrete VP schedule in float64: log alpha at the knots t_i = (i + 1) / T, linear in between, the end segments extended."""

    def __init__(self, log_alpha):
        self.la = np.asarray(log_alpha, dtype=np.float64)
        self.T = len(self.la)
        self.t = (np.arange(self.T, dtype=np.float64) + 1.0) / self.T

    @staticmethod
    def _interp(q, xp, yp):
        hi = min(max(int(np.searchsorted(xp, q, side="left")), 1), len(xp) - 1)
        lo = hi - 1
        return yp[lo] + (q - xp[lo]) * (yp[hi] - yp[lo]) / (xp[hi] - xp[lo])

    def log_alpha(self, t):
        return self._interp(float(t), self.t, self.la)

    def alpha(self, t):
        return np.exp(self.log_alpha(t))

    def sigma(self, t):
        return np.sqrt(-np.expm1(2.0 * self.log_alpha(t)))

    def lam(self, t):
        la = self.log_alpha(t)
        return la - 0.5 * np.log(-np.expm1(2.0 * la))

    def inv_lam(self, lam):
        m = -2.0 * float(lam)
        q = -0.5 * (m + np.log1p(np.exp(-m)) if m > 0.0 else np.log1p(np.exp(m)))
        return self._interp(q, self.la[::-1], self.t[::-1])

    def model_time(self, t):
        """model_wrapper.get_model_input_time on the time rounded to fp32: every operation in fp32, then truncation."""
        return int((F32(t) - F32(1.0 / self.T)) * F32(self.T))


def rows(S, s, h, lam_s, defect=None):
    """Everything the next trial reads: {"t", "s1", "tm_s", "tm_s1", "f64": the 16 rows of ftab before rounding, "ftab": after}."""
    t = S.inv_lam(lam_s + h)
    s1 = S.inv_lam(lam_s + (h if defect == "s1_at_h" else 0.5 * h))
    al_s, al_1, al_t = S.alpha(s), S.alpha(s1), S.alpha(t)
    sg_s, sg_1, sg_t = S.sigma(s), S.sigma(s1), S.sigma(t)
    h_t, h_1 = S.lam(t) - lam_s, S.lam(s1) - lam_s
    first = -(al_t * np.expm1(-h_t))
    c2 = (0.5 / 0.5) * first
    c1 = first - c2
    f = np.array([1.0 / al_s, -sg_s / al_s, sg_t / sg_s, first, sg_1 / sg_s, -(al_1 * np.expm1(-h_1)),
                  1.0 / al_1, -sg_1 / al_1, sg_t / sg_s, c1, c2, 0.0, al_s, sg_s, al_1, sg_1], dtype=np.float64)
    return {"t": t, "s1": s1, "tm_s": S.model_time(s), "tm_s1": S.model_time(s1), "f64": f, "ftab": f.astype(F32)}


def init_state(S, p):
    """The controller's init for one sample: state dict with its first rows."""
    s = float(p["t_T"])
    st = {"s": s, "h": float(p["h_init"]), "lam_s": S.lam(s), "lam_0": S.lam(p["t_0"]), "E": 0.0, "attempts": 0, "accepted": 0,
          "flag": IDLE, "done": False, "fault": False}
    st["done"] = abs(st["s"] - p["t_0"]) <= p["t_err"]
    st["rows"] = rows(S, st["s"], st["h"], st["lam_s"])
    return st


def error_norm(sums, pers, defect=None):
    """E of one sample from its streams' fp64 sums: the maximum of sqrt(sum / per), rounded to fp32 (unless the defect says not)."""
    vals = [np.sqrt(np.float64(sv) / np.float64(per)) for sv, per in zip(sums, pers)]
    if defect == "E_not_fp32":
        return float(max(vals))
    return float(max(F32(v) for v in vals))


def control(S, p, st, E, defect=None):
    """One trial's end for one sample (or the batch, with E its maximum): the new state dict.  A finished sample idles; a non-finite E
    faults and changes nothing but the flag."""
    st = dict(st)
    if st["done"]:
        st["flag"] = IDLE
        return st
    if not np.isfinite(E):
        st["flag"], st["fault"] = REJECT, True
        return st
    st["E"] = E
    st["attempts"] += 1
    if E <= 1.0:
        st["s"] = st["rows"]["t"]
        st["lam_s"] = S.lam(st["s"])
        st["accepted"] += 1
        st["flag"] = ACCEPT
    else:
        st["flag"] = REJECT
    h = p["theta"] * st["h"] * (1.0 / np.sqrt(np.float64(E))) if E > 0.0 else np.inf
    st["h"] = float(h) if defect == "h_not_capped" else float(min(h, st["lam_0"] - st["lam_s"]))
    if abs(st["s"] - p["t_0"]) <= p["t_err"]:
        st["done"] = True
        return st
    st["rows"] = rows(S, st["s"], st["h"], st["lam_s"], defect)
    return st


# ----------------------------------------------------------------------------- the error sums of mmd_dpm_adapt_close
def error_terms(hi, lo, prev, atol, rtol):
    """fp32 element terms e = (hi - lo) / max(atol, rtol max(|lo|, |prev|)), dpm_err_kernel's expression operation by operation."""
    hi, lo, prev = (np.asarray(v, dtype=F32).reshape(-1) for v in (hi, lo, prev))
    delta = np.maximum(F32(atol), F32(rtol) * np.maximum(np.abs(lo), np.abs(prev)))
    return (hi - lo) / delta


def chunk_sums(e, defect=None):
    """The kernel's partial sums of one sample's terms e (fp32 [per]), bit for bit: a chunk is CHUNK elements; thread t of 256 adds the
    squares of its quads 4 t + 1024 i + j in ascending order (each square is exact in fp64), then the fixed tree over the threads."""
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    out = []
    for c0 in range(0, len(e), CHUNK):
        sq = np.zeros(CHUNK, dtype=np.float64)
        part = e[c0:c0 + CHUNK]
        sq[:len(part)] = part * part
        q = sq.reshape(CHUNK // 1024, 256, 4)          # [i, thread, j]
        acc = np.zeros(256, dtype=np.float64)
        order = [(i, j) for i in range(q.shape[0]) for j in range(4)]
        for i, j in (reversed(order) if defect == "chunk_order" else order):
            acc = acc + q[i, :, j]
        o = 128
        while o > 0:
            acc[:o] = acc[:o] + acc[o:2 * o]
            o >>= 1
        out.append(acc[0])
    return np.array(out, dtype=np.float64)


def fold(chunks):
    """The controller's fold of a sample's chunks: ascending."""
    s = np.float64(0.0)
    for v in chunks:
        s = s + v
    return s


def commit(flag, x, xb, prev, lo, defect=None):
    """(x, PREV) after mmd_dpm_adapt_commit of one sample."""
    if flag == ACCEPT:
        return x, lo.copy()
    if flag == REJECT:
        return xb.copy(), (lo.copy() if defect == "prev_on_reject" else prev)
    return x, prev


# ----------------------------------------------------------------------------- the comparisons of the GPU tests
def ulp_diff(a, b):
    """distance of two fp32 arrays in units in the last place (sign-magnitude order of the bits)"""
    def key(v):
        i = np.asarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def compare_control(got, want, rel=1e-12):
    """got / want: state dicts (the device's read back, the restatement's).  Returns the list of what differs - decisions, flags,
    counters and timesteps exactly, s / h / t / s1 within `rel` relative, fp32 rows within 1 ulp - and the largest relative deviation."""
    bad, worst = [], 0.0
    for k in ("attempts", "accepted", "flag", "done", "fault"):
        if int(got[k]) != int(want[k]):
            bad.append((k, got[k], want[k]))
    for k in ("s", "h", "lam_s"):
        d = abs(got[k] - want[k]) / max(abs(want[k]), 1e-300)
        worst = max(worst, d)
        if not d <= rel:
            bad.append((k, got[k], want[k], d))
    if not want["done"] and not want["fault"]:
        for k in ("t", "s1"):
            d = abs(got["rows"][k] - want["rows"][k]) / abs(want["rows"][k])
            worst = max(worst, d)
            if not d <= rel:
                bad.append((k, got["rows"][k], want["rows"][k], d))
        for k in ("tm_s", "tm_s1"):
            if int(got["rows"][k]) != int(want["rows"][k]):
                bad.append((k, got["rows"][k], want["rows"][k]))
        u = ulp_diff(got["rows"]["ftab"], want["rows"]["ftab"])
        if u.max() > 1:
            bad.append(("ftab", int(u.argmax()), int(u.max())))
    return bad, worst


def compare_partials(got, e):
    """got: the device's partial sums of one sample, e: its fp32 terms.  The sums must be the restated order's bit for bit, and their
    fold within (elements + chunks) 2^-53 relative of numpy's fp64 sum of the squares (the bound of a fixed-order fp64 sum of
    non-negative terms).  Returns the list of what fails."""
    bad = []
    want = chunk_sums(e)
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    if got.shape != want.shape or not np.array_equal(got.view(np.int64), want.view(np.int64)):
        bad.append(("order", got, want))
    ref = float(np.sum(np.asarray(e, dtype=np.float64) ** 2))
    bound = (len(e) + len(want)) * 2.0 ** -53 * ref
    if not abs(float(fold(got)) - ref) <= bound:
        bad.append(("bound", float(fold(got)), ref, bound))
    return bad


def compare_commit(got, want):
    """(x, PREV) pairs, bit for bit."""
    return [name for name, g, w in zip(("x", "PREV"), got, want)
            if not np.array_equal(np.asarray(g, dtype=F32).view(np.int32), np.asarray(w, dtype=F32).view(np.int32))]


# ----------------------------------------------------------------------------- the whole loop
def adaptive_loop(S, p, x, model, thresholding=True, max_val=1.0, control_rule="batch", max_attempts=1000, defect=None):
    """The loop of sample_graph_adaptive in float64 coefficients and fp32 tensors.  x: {"video", "audio"} float32 arrays [B, ...];
    model(x, tm int64 [B]) -> {"video", "audio"} eps arrays.  Returns (x, {"trials", "accepted", "nfe", "tm": the model timesteps of
    every evaluation, "E": [trial][sample], "margin": the smallest |E - 1|})."""
    keys = ("video", "audio")
    B = x["video"].shape[0]
    x = {k: np.asarray(x[k], dtype=F32).copy() for k in keys}
    prev = {k: v.copy() for k, v in x.items()}
    st = [init_state(S, p) for _ in range(B)]
    info = {"trials": 0, "nfe": 0, "tm": [], "E": []}

    def bc(v, a):
        return np.asarray(v, dtype=F32).reshape((-1,) + (1,) * (a.ndim - 1))

    def predict(x, eps, cx, ce):
        out = {}
        for k in keys:
            v = bc(cx, x[k]) * x[k] + bc(ce, x[k]) * eps[k]
            if thresholding:
                sq = np.quantile(np.abs(v).reshape(B, -1).astype(np.float64), 0.995, axis=1).astype(F32)
                sq = bc(np.maximum(sq, F32(1.0)), v)
                v = np.clip(v, -sq, sq) / (sq / F32(max_val))
            out[k] = v.astype(F32)
        return out
    while not all(s["done"] for s in st):
        if info["trials"] >= max_attempts:
            raise RuntimeError(f"not done after {info['trials']} trial steps")
        f = np.stack([s["rows"]["ftab"] for s in st], axis=1)          # [16, B]
        tm_s, tm_1 = (np.array([s["rows"][k] for s in st], dtype=np.int64) for k in ("tm_s", "tm_s1"))
        live = np.array([not s["done"] for s in st])
        m0 = predict(x, model(x, tm_s), f[0], f[1])
        xb = x
        lo = {k: (bc(f[2], x[k]) * x[k] + bc(f[3], x[k]) * m0[k]).astype(F32) for k in keys}
        x1 = {k: (bc(f[4], x[k]) * x[k] + bc(f[5], x[k]) * m0[k]).astype(F32) for k in keys}
        m1 = predict(x1, model(x1, tm_1), f[6], f[7])
        hi = {k: (bc(f[8], x[k]) * xb[k] + bc(f[9], x[k]) * m0[k] + bc(f[10], x[k]) * m1[k]).astype(F32) for k in keys}
        info["tm"] += [tm_s, tm_1]
        info["nfe"] += 2
        info["trials"] += 1
        Es = []
        for n in range(B):
            sums, pers = [], []
            for k in keys:
                e = error_terms(hi[k][n], lo[k][n], prev[k][n], p["atol"], p["rtol"])
                sums.append(fold(chunk_sums(e)))
                pers.append(e.size)
            Es.append(error_norm(sums, pers, defect))
        if control_rule == "batch":
            Es = [max(Es)] * B
        info["E"].append(list(Es))
        new = {k: hi[k].copy() for k in keys}
        for n in range(B):
            if not live[n]:
                for k in keys:
                    new[k][n] = xb[k][n]
                continue
            st[n] = control(S, p, st[n], Es[n], defect)
            for k in keys:
                new[k][n], prev[k][n] = commit(st[n]["flag"], hi[k][n], xb[k][n], prev[k][n], lo[k][n], defect)
        x = new
    info["accepted"] = [s["accepted"] for s in st]
    info["attempts"] = [s["attempts"] for s in st]
    info["margin"] = min(abs(e - 1.0) for row in info["E"] for e in row)
    return x, info
