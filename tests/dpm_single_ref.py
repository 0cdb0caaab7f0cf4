"""Numpy restatement of mmd_dpm_single_update (include/mmd.h) and of the loop DPM_Solver.sample_graph_singlestep drives with it: the three
row kinds on fp32 data with the kernel's roundings - one rounded product, then one fma per further term, the fma emulated as in
dpmpp_ref.lerp32 (the product exact in float64, 24 x 24 bits, and one rounding of the sum).  `defect` seeds one of the mistakes the
CPU tests must flag."""
import numpy as np

OPEN, STAGE, DENOISE = 0, 1, 2
DEFECTS = ("stage_reads_x", "ms_overwritten", "c1_c2_swapped")


def mul32(c, a):
    return (np.float32(c) * a.astype(np.float32)).astype(np.float32)


def fma32(c, a, v):
    """fmaf(c, a, v) on fp32 arrays a, v with the fp32 scalar c."""
    return (np.float64(np.float32(c)) * a.astype(np.float64) + v.astype(np.float64)).astype(np.float32)


def m0_of(form, row, x, src):
    """form 0: the source itself; form 1: cx x + ce eps."""
    return src.astype(np.float32) if form == 0 else fma32(row[1], src, mul32(row[0], x))


def update(row, x, XB, MS, m0, defect=None):
    """One row (cx, ce, c0, c1, c2, kind) applied to the state: returns the new (x, XB, MS)."""
    c0, c1, c2, kind = row[2], row[3], row[4], int(row[5])
    if defect == "c1_c2_swapped":
        c1, c2 = c2, c1
    if kind == OPEN:
        return fma32(c1, m0, mul32(c0, x)), x.copy(), m0.copy()
    if kind == STAGE:
        base = x if defect == "stage_reads_x" else XB
        new = fma32(c2, m0, fma32(c1, MS, mul32(c0, base)))
        return new, XB, (m0.copy() if defect == "ms_overwritten" else MS)
    return m0.copy(), XB, MS


def run(tabs, eps_fn, x_T, predict_x0, defect=None):
    """The loop over the rows of DPM_Solver.singlestep_tables: eps_fn(x: {stream: array}, tm: int) -> {stream: array} is the model."""
    x = {k: v.astype(np.float32) for k, v in x_T.items()}
    XB = {k: np.zeros_like(v) for k, v in x.items()}
    MS = {k: np.zeros_like(v) for k, v in x.items()}
    for j in range(tabs["rows"]):
        eps = eps_fn(x, tabs["tm"][j])
        for k in x:
            row = tabs["tab"][k][:, j]
            form = 1 if (predict_x0 or int(row[5]) == DENOISE) else 0
            x[k], XB[k], MS[k] = update(row, x[k], XB[k], MS[k], m0_of(form, row, x[k], eps[k]), defect)
    return x
