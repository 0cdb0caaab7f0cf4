"""The layout-edge convolutions of mmd_edge.hip against float64, ELEMENT BY ELEMENT: mmd_stem_conv (per-pixel, strip, MFMA),
mmd_head_conv (strip, cooperative, plain) and the head as mmd_head_gemm + mmd_head_gather (tests/errbound_fwd.py: the references, the
bounds and their derivation, the host-side selection rules that name the kernel a case reaches, the case lists;
tests/test_errbound_fwd_cpu.py: the metric proven on seeded defects).

Every case calls the kernel through mm_diffusion.ops with NaN-prefilled outputs, builds the reference with torch double ops on the
STORED operands - never with a libmmd kernel - and admits ZERO elements outside the per-element bound; column-slice cases also assert
that the buffer around the output view is untouched.  head_gemm + head_gather is checked at three levels: P against float64, y
against float64 from the STORED P, and end to end.  Not reached: the plain head kernel's second grid-stride pass (over 2 M rows).

Worst error / bound ratio per kernel variant, as printed by the tests (`-s`) on an MI355X (a record of headroom, not a tolerance):

    kernel / variant                          dtype  cases  worst ratio
    stem_conv per-pixel                       f32        3        0.193
    stem_conv per-pixel                       bf16       3        0.991
    stem_conv strip                           f32        4        0.466
    stem_conv strip                           bf16       4        0.993
    stem_conv MFMA (NB 1-4, K = 3, pipelined) bf16      12        0.995
    head_conv strip                           bf16      10        0.008
    head_conv strip (incl. second pass)       f32       11        0.016
    head_conv coop (incl. second pass)        bf16       9        0.017
    head_conv coop                            f32        8        0.015
    head_conv plain                           bf16       4        0.075
    head_conv plain                           f32        2        0.009
    head_gemm: P                              bf16       8        0.409
    head_gather: y from the stored P          f32        8        0.249
    head_gemm + head_gather end to end        bf16       8        0.179

Every case: zero violating elements, zero non-finite outputs.  The bf16 stem sits near 1 because its budget is the single store
rounding (2**-8 |ref|) and some element always lies next to a rounding midpoint; the fp32 kernels sit far below 1 because the
any-order bound (K + 2) u sum |terms| grants every one of up to 13824 additions a full u.  Run time on an MI355X: 2.0 s for the 78 cases.
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


def _slice(rows, C, dtype, extra, pad, fill):
    """A [rows, C] view at columns [pad, pad + C) of a SENTINEL buffer `extra` columns wider, filled with `fill` (a tensor or a value)."""
    buf = torch.full((rows, C + extra), SENTINEL, dtype=dtype, device="cuda")
    view = buf[:, pad:pad + C]
    view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    return buf, view


def _untouched(buf, pad, C, what):
    assert bool((buf[:, :pad] == SENTINEL).all()) and bool((buf[:, pad + C:] == SENTINEL).all()), f"{what}: wrote outside the output view"


# --------------------------------------------------------------------------- mmd_stem_conv
@pytest.mark.parametrize("c", W.stem_cases(), ids=lambda c: c["name"])
def test_stem_conv_elementwise(ops, c):
    x, w, bias = _cu(*W.edge_inputs(c))
    taps, dims, dt = W.TAPS[c["taps"]], (c["F"], c["H"], c["W"]), DT[c["dt"]]
    M, Cout = c["N"] * c["F"] * c["H"] * c["W"], c["Cout"]
    extra = 40 if c["y_strided"] else 0
    assert W.stem_variant(c["dt"], c["Cin"], c["W"], Cout, taps, Cout + extra) == c["variant"]
    ref, bound = W.edge_ref(W.api_to_rows(x), w, bias, taps, dims, dt)
    buf, out = _slice(M, Cout, dt, extra, 8 if extra else 0, float("nan"))
    ops.stem_conv(x, w, bias, out, c["N"], c["F"], c["Cin"], c["H"], c["W"], taps)
    worst = E.check(out, ref, bound, pixels=c["H"] * c["W"], what=f"stem_conv {c['name']}")
    if extra:
        _untouched(buf, 8, Cout, c["name"])
    print(f"\nRATIO stem {c['variant']} {c['dt']} {c['name']}: {worst:.3f}")


# --------------------------------------------------------------------------- mmd_head_conv
@pytest.mark.parametrize("c", W.head_cases(), ids=lambda c: c["name"])
def test_head_conv_elementwise(ops, c):
    x, w, bias = _cu(*W.edge_inputs(c))
    taps, dims = W.TAPS[c["taps"]], (c["F"], c["H"], c["W"])
    N, Fr, Hh, Ww, Co = c["N"], c["F"], c["H"], c["W"], c["Co"]
    assert W.head_variant(c["dt"], c["Cin"], Co, len(taps), Ww, not c["y_off"])[0] == c["variant"]
    ref, bound = W.edge_ref(x, w, bias, taps, dims, F32)
    xin = _slice(x.shape[0], c["Cin"], x.dtype, 40, 16, x)[1] if c["x_strided"] else x
    n = N * Fr * Co * Hh * Ww
    flat = torch.full((n + 8,), SENTINEL, dtype=F32, device="cuda")
    off = 1 if c["y_off"] else 0                             # y_off: the output starts 4 bytes past a 16-byte boundary
    assert flat.data_ptr() % 16 == 0
    y = flat[off:off + n].view(N, Fr, Co, Hh, Ww)
    y.fill_(float("nan"))
    ops.head_conv(xin, w, bias, y, N, Fr, Hh, Ww, taps)
    worst = E.check(W.api_to_rows(y), ref, bound, pixels=Hh * Ww, what=f"head_conv {c['name']}")
    assert bool((flat[:off] == SENTINEL).all()) and bool((flat[off + n:] == SENTINEL).all()), f"{c['name']}: wrote outside the output"
    print(f"\nRATIO head {c['variant']} {c['dt']} {c['name']}: {worst:.3f}")


# --------------------------------------------------------------------------- mmd_head_gemm + mmd_head_gather
@pytest.mark.parametrize("case", W.HEAD_GEMM_CASES, ids=lambda c: c[0])
def test_head_gemm_gather_elementwise(ops, case):
    name, Co, tk, N, Fr, Hh, Ww, S = case
    taps, dims = W.TAPS[tk], (Fr, Hh, Ww)
    x, a, b, w, bias = _cu(*W.head_gemm_inputs(Co, tk, N, Fr, Hh, Ww, S))
    M, NO = x.shape[0], len(taps) * Co
    geom = ops.Geom.per_sample(S, M // S)
    xin = _slice(M, 128, x.dtype, 40, 16, x)[1] if S == 2 else x          # the 384-row slices: x as a column slice
    wimg = ops.head_gemm_pack(w)
    P = torch.full((NO, M), float("nan"), dtype=F32, device="cuda")
    ops.head_gemm(xin, a, b, geom, True, wimg, P, NO)
    Pref, eP = W.head_gemm_ref(x.view(S, M // S, 128), a, b, True, w, W.head_gemm_unpack(wimg))
    r1 = E.check(P, Pref, eP, what=f"head_gemm {name}: P")
    y = torch.full((N, Fr, Co, Hh, Ww), float("nan"), dtype=F32, device="cuda")
    ops.head_gather(P, bias, y, N, Fr, Hh, Ww, Co, taps)
    yr = W.api_to_rows(y)
    r2 = E.check(yr, *W.head_gather_ref(P, bias, Co, taps, dims), pixels=Hh * Ww, what=f"head_gather {name}: y from the stored P")
    r3 = E.check(yr, *W.head_gather_ref(Pref, bias, Co, taps, dims, eP), pixels=Hh * Ww, what=f"head_gemm + head_gather {name}: end to end")
    print(f"\nRATIO head_gemm bf16 {name}: P {r1:.3f} gather {r2:.3f} end-to-end {r3:.3f}")
