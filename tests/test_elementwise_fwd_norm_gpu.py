"""The GroupNorm forward kernels of mmd_norm.hip against float64, ELEMENT BY ELEMENT (tests/errbound_fwd.py: the references, the bounds
and their derivation, the selection rules, the case lists; tests/test_errbound_fwd_cpu.py: the metric proven on seeded defects).

Every case calls the kernel through mm_diffusion.ops with NaN-prefilled outputs, builds the reference with torch double ops on the
STORED operands - never with a libmmd kernel - and admits ZERO elements outside the per-element bound; column-slice cases also assert
that the buffer around the output view is untouched.

Worst error / bound ratio per kernel, as printed by the tests (`-s`) on an MI355X (a record of headroom, not a tolerance):

    kernel                                   dtype  cases  worst ratio
    gn_apply (act off and on)                bf16      63        0.996
    gn_apply (act off and on)                f32       39        0.518
    gn_small (act off and on)                bf16      14        0.995
    gn_small (act off and on)                f32       11        0.187
    gn_group mean / rstd / a / b             bf16       9        0.176
    gn_group mean / rstd / a / b             f32        9        0.182
    gn_group y                               bf16       9        0.996
    gn_group y                               f32        9        0.173
    gn_finalize_stats a / b / mean / rstd    f32        6        0.991
    add_rowbias                              bf16       2        0.991
    add_rowbias                              f32        2        0.999

Every case: zero violating elements, zero non-finite outputs.  The ratios near 1 are the single store rounding used up by an element
next to a rounding midpoint: 2**-8 |ref| in bf16, and for gn_finalize_stats and add_rowbias in fp32 the whole budget is one or a few u.
The statistics of gn_small / gn_group sit at 0.2: the depth bound grants every addition of the chain a full u, random roundings add
like its square root.  Run time on an MI355X: 2.4 s for the 155 cases.
"""
import pytest
import torch

import errbound as E
import errbound_fwd as W

pytestmark = pytest.mark.gpu

F32 = torch.float32
DT = W.DT
SENTINEL = 1e4            # around every column slice: read by mistake it breaks every bound


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mm_diffusion import ops as o
    return o


def _cu(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _slice_of(t, extra, pad, fill=None):
    """t (fill given: that value in t's shape) as columns [pad, pad + C) of a buffer `extra` columns wider; returns (buffer, view)."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), SENTINEL, dtype=t.dtype, device=t.device)
    view = buf[:, pad:pad + t.shape[1]]
    view.copy_(t if fill is None else torch.full_like(t, fill))
    return buf, view


def _out(like, extra=0, pad=0):
    """A NaN-prefilled output of like's shape; extra > 0: as a column slice.  Returns (buffer, view)."""
    if not extra:
        o = torch.full_like(like, float("nan"))
        return o, o
    return _slice_of(like, extra, pad, float("nan"))


def _untouched(buf, pad, C, what):
    assert bool((buf[:, :pad] == SENTINEL).all()) and bool((buf[:, pad + C:] == SENTINEL).all()), f"{what}: wrote outside the output view"


# --------------------------------------------------------------------------- gn_apply
@pytest.mark.parametrize("case", W.apply_cases(), ids=lambda c: c[0])
def test_gn_apply_elementwise(ops, case):
    name, dt, C, kind, N, Tn, HW, big, strided = case
    x, a, b, slices, geom = W.apply_inputs(dt, C, kind, N, Tn, HW, big)
    x, a, b, slices = _cu(x, a, b, slices)
    xs = x[slices]
    xin = _slice_of(x, 40, 16)[1] if strided else x
    worst = 0.0
    for act in (False, True):
        ref, bound = W.apply_ref(xs, a, b, act, DT[dt])
        buf, out = _out(x, 48 if strided else 0, 8)
        ops.gn_apply(xin, a, b, ops.Geom(*geom), act=act, out=out)
        worst = max(worst, E.check(out[slices].flatten(0, 1), ref.flatten(0, 1), bound.flatten(0, 1), what=f"gn_apply {name} act={act}"))
        if strided:
            _untouched(buf, 8, C, f"gn_apply {name}")
    print(f"\nRATIO gn_apply {dt} {name}: {worst:.3f}")


# --------------------------------------------------------------------------- gn_small
@pytest.mark.parametrize("case", W.small_cases(), ids=lambda c: c[0])
def test_gn_small_elementwise(ops, case):
    name, dt, C, kind, N, Tn, HW, big = case
    x, gamma, beta, _, slices, geom = W.gn_inputs(dt, C, kind, N, Tn, HW, big, 51, film=False)
    x, gamma, beta, slices = _cu(x, gamma, beta, slices)
    strided = Tn == 5                                        # x and out as column slices with ldx != ldy
    xin = _slice_of(x, 40, 16)[1] if strided else x
    worst = 0.0
    for act in (False, True):
        r = W.two_pass_ref(x, gamma, beta, None, slices, act, DT[dt], "small")
        buf, out = _out(x, 48 if strided else 0, 8)
        ops.gn_small(xin, gamma, beta, ops.Geom(*geom), act=act, out=out)
        worst = max(worst, E.check(out, r["y"], r["e_y"], what=f"gn_small {name} act={act}"))
        if strided:
            _untouched(buf, 8, C, f"gn_small {name}")
    print(f"\nRATIO gn_small {dt} {name}: {worst:.3f}")


# --------------------------------------------------------------------------- gn_group
@pytest.mark.parametrize("case", W.group_cases(), ids=lambda c: c[0])
def test_gn_group_elementwise(ops, case):
    name, dt, C, kind, N, Tn, HW, big, film, act, mode, strided = case
    x, gamma, beta, fl, slices, geom = W.gn_inputs(dt, C, kind, N, Tn, HW, big, 51, film=film)
    x, gamma, beta, fl, slices = _cu(x, gamma, beta, fl, slices)
    S = geom[0]
    r = W.two_pass_ref(x, gamma, beta, fl, slices, act, DT[dt], "group")
    xin = _slice_of(x, 44, 8)[1] if strided else x
    nan = lambda *s: torch.full(s, float("nan"), dtype=F32, device="cuda")
    a, b = (nan(S, C), nan(S, C)) if mode != "tensor" else (None, None)
    buf, out = _out(x, 44 if strided else 0, 16) if mode != "affine" else (None, None)
    mr = nan(S, 32, 2)
    ops.gn_group(xin, gamma, beta, ops.Geom(*geom), film=fl, a=a, b=b, out=out, act=act, mr=mr)
    what = f"gn_group {name}"
    worst = max(E.check(mr[..., 0], r["mean"], r["e_mean"], what=what + ": mr_out mean"),
                E.check(mr[..., 1], r["rstd"], r["e_rstd"], what=what + ": mr_out rstd"))
    if a is not None:
        worst = max(worst, E.check(a, r["a"], r["e_a"], what=what + ": a"), E.check(b, r["b"], r["e_b"], what=what + ": b"))
    wy = 0.0
    if out is not None:
        wy = E.check(out, r["y"], r["e_y"], what=what + ": y")
        if strided:
            _untouched(buf, 16, C, what)
    print(f"\nRATIO gn_group {dt} {name}: stats {worst:.3f} y {wy:.3f}")


# --------------------------------------------------------------------------- gn_finalize_stats, stage-wise
@pytest.mark.parametrize("case", W.finalize_cases(), ids=lambda c: c[0])
def test_gn_finalize_stats_elementwise(ops, case):
    name, C, S, nrec, ratio, film, strided = case
    rec, gamma, beta, fl = _cu(*W.finalize_inputs(C, S, nrec, ratio, film))
    Tn = nrec * 64
    r = W.finalize_ref(rec, C, S, Tn, gamma, beta, fl)
    if strided:                                              # the record view as a column slice of a wider record buffer
        wide = torch.full((rec.shape[0], C // 4 + 24, 2), SENTINEL, dtype=F32, device="cuda")
        wide[:, 8:8 + C // 4] = rec
        rec = wide[:, 8:8 + C // 4]
    nan = lambda *s: torch.full(s, float("nan"), dtype=F32, device="cuda")
    a, b, mr = nan(S, C), nan(S, C), nan(S, 32, 2)
    ops.gn_finalize_stats(rec, gamma, beta, ops.Geom.per_sample(S, Tn), film=fl, a=a, b=b, mr=mr)
    what = f"gn_finalize_stats {name}"
    worst = max(E.check(a, r["a"], r["e_a"], what=what + ": a"), E.check(b, r["b"], r["e_b"], what=what + ": b"),
                E.check(mr[..., 0], r["mean"], r["e_mean"], what=what + ": mean"), E.check(mr[..., 1], r["rstd"], r["e_rstd"], what=what + ": rstd"))
    print(f"\nRATIO gn_finalize_stats f32 {name}: {worst:.3f}")


# --------------------------------------------------------------------------- add_rowbias
@pytest.mark.parametrize("case", W.ROWBIAS_CASES, ids=str)
def test_add_rowbias_elementwise(ops, case):
    dt, N, rps, C, strided = case
    x, e = _cu(*W.rowbias_inputs(dt, N, rps, C))
    ref, bound = W.rowbias_ref(x, e, rps, DT[dt])
    buf, xio = _slice_of(x, 40, 16) if strided else (None, x.clone())
    ein = _slice_of(e, 12, 4)[1] if strided else e
    ops.add_rowbias(xio, ein, rps)
    worst = E.check(xio, ref, bound, what=f"add_rowbias {case}")
    if strided:
        _untouched(buf, 16, C, f"add_rowbias {case}")
    print(f"\nRATIO add_rowbias {dt} {case}: {worst:.3f}")
