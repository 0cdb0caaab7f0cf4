"""The element-wise metric of tests/errbound_fused.py (fused VideoConv, temporal attention block), proven on the CPU on exactly the case
lists tests/test_elementwise_fused_gpu.py runs.

1. `rn_bf16` rounds to nearest even straight from float64: exact midpoints go to the even neighbour, their float64 neighbours to the
   nearer side - where `t.double().to(torch.bfloat16)` (through float32) rounds twice and gets it wrong; on float32 inputs it equals
   torch's own single rounding.  `dev` is zero away from a midpoint and one step next to it.
2. The staged references without their restated roundings equal torch's own float64 operators (F.conv2d + F.conv1d behind the affine;
   F.group_norm, the qkv / proj_out matmuls and softmax) to 1e-12.
3. Faithful fp32 emulations of both chains - the kernel's rounding points, its K order in the spatial GEMM, its summation order in the
   in-register GroupNorm, P as a bf16 hi + lo pair - have ZERO violating elements on every case, and the validity condition of the
   attention propagation (sum_j p eta < 1/2) holds on every case, the spike case included.
4. Every seeded defect of errbound_fused.VCONV_DEFECTS / TATTN_DEFECTS is flagged on at least one case - except those of
   errbound_fused.TATTN_BLIND, which are asserted to stay inside the bound on every case, as the module's docstring states.  One run
   (`-s` prints these lines; "cases" = launches the defect applies to):

       defect                                              worst error / bound   flagged on
       vconv: padding normalised instead of zero                        1350     12 of 12 cases
       vconv: halo corner slot from the wrong pixel                      130      6 of 18 (those with an interior patch corner)
       vconv: temporal tap across the sample boundary                    254     12 of 12
       vconv: zero frame holds bf16(bias_s)                              894     18 of 18
       vconv: chunk c's affine applied to chunk c + 1                     60     10 of 10
       vconv: truncating output store                                    1.67     9 of 18
       tattn: keys of the wave's other pixel not masked                 19.7      7 of 7
       tattn: heads swapped in the projection's K order                 30.2      7 of 7
       tattn: residual from the neighbouring row                         597      7 of 7
       tattn: GroupNorm statistics of the neighbouring pixel            43.1      7 of 7
       tattn: truncating output store                                   1.21      1 of 7 (2x8-offset)
       tattn: row sum taken from the rounded P                          0.63      0 of 7: BLIND SPOT
5. A double rounding of an intermediate (T or O: the accumulator rounded to bf16 in front of the bias / the 1 / l scaling and again
   behind it) is evaluated on every case: flagged on the single-chunk VideoConv case only.  The test prints the violations, the share
   of output bits that differ from the clean emulation and the rel-L2 distance per case, and asserts what errbound_fused's docstring
   says: on the VideoConv more than 3 % of the bits differ on every case (test_vconv_gpu.py::test_vconv_vs_two_launch_path's "> 97 %
   bitwise equal" sees it), on the attention block it stays inside the bound everywhere.
"""
import functools

import pytest
import torch
import torch.nn.functional as F_

import errbound as E
import errbound_fused as Z
from helpers import rel_l2

BF = torch.bfloat16


# --------------------------------------------------------------------------- rn_bf16, dev
def test_rn_bf16_midpoints_and_neighbours():
    g = torch.Generator().manual_seed(1)
    lo = (torch.randn(4096, generator=g) * torch.exp2(torch.randint(-20, 20, (4096,), generator=g).float())).to(BF)
    lo = torch.cat([lo, torch.tensor([1.0, -1.0, 255.0, 0.99609375, 2.0 ** -126, 1.1754944e-38 * 4]).to(BF)])
    bits = lo.view(torch.int16).int()
    up = (bits + 1).short().view(BF)                                   # the next bf16 away from zero (crosses binades correctly)
    lo64, up64 = lo.double(), up.double()
    mid = (lo64 + up64) / 2                                             # exact in float64
    even = torch.where(bits % 2 == 0, lo64, up64)
    assert torch.equal(Z.rn_bf16(mid), even)
    inf = torch.full_like(mid, float("inf"))
    toward_up = torch.nextafter(mid, torch.where(up64 > mid, inf, -inf))
    toward_lo = torch.nextafter(mid, torch.where(lo64 > mid, inf, -inf))
    assert torch.equal(Z.rn_bf16(toward_up), up64) and torch.equal(Z.rn_bf16(toward_lo), lo64)
    assert torch.equal(Z.rn_bf16(lo64), lo64) and torch.equal(Z.rn_bf16(torch.zeros(3, dtype=torch.float64)), torch.zeros(3, dtype=torch.float64))
    # through float32 the neighbour of a midpoint first becomes the midpoint, then ties to even: wrong for every odd `lo` / even `up`
    twice = toward_up.to(BF).double()
    assert int((twice != up64).sum()) > 1000 and torch.equal(twice[bits % 2 == 1], up64[bits % 2 == 1])
    # float32 inputs: torch's own (single) rounding
    f = torch.randn(100000, generator=g) * 3
    assert torch.equal(Z.rn_bf16(f.double()), f.to(BF).double())
    sub = torch.tensor([2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -134, 2.0 ** -127 + 2.0 ** -134], dtype=torch.float64)   # bf16 subnormals: spacing 2**-133
    assert torch.equal(Z.rn_bf16(sub), torch.tensor([2.0 ** -133, 2.0 ** -132, 0.0, 2.0 ** -127], dtype=torch.float64))


def test_dev_is_zero_away_from_midpoints():
    z = torch.tensor([1.0, 1.00390625, 1.0039, 1.0117, 1.0 - 2.0 ** -10], dtype=torch.float64)    # 1.00390625 = the midpoint of 1 and 1 + 2**-7
    s, d = Z.dev(z, torch.full_like(z, 1e-5))
    assert torch.equal(s, torch.tensor([1.0, 1.0, 1.0, 1.0078125, 1.0], dtype=torch.float64))
    assert torch.equal(d, torch.tensor([0.0, 2.0 ** -7, 2.0 ** -7, 0.0, 0.0], dtype=torch.float64))
    s, d = Z.dev(z, torch.zeros_like(z))
    assert not d.any()
    s, d = Z.dev(torch.tensor([1.0], dtype=torch.float64), torch.tensor([0.0121], dtype=torch.float64))     # beyond the second midpoint above, the first below
    assert float(d) == 2.0 ** -6


# --------------------------------------------------------------------------- shared operands and references (built once per case)
@functools.lru_cache(maxsize=None)
def _vconv(name, gn):
    ops = Z.vconv_case(name, gn)
    ref, bound = Z.vconv_ref(*ops)
    return ops, ref, bound


@functools.lru_cache(maxsize=None)
def _tattn(name):
    ops = Z.tattn_case(name)
    ref, bound, validity = Z.tattn_ref(*ops)
    return ops, ref, bound, validity


VC = [(c[0], gn) for c in Z.VCONV_CASES for gn in Z.VCONV_GN]
TA = [c[0] for c in Z.TATTN_CASES]


# --------------------------------------------------------------------------- the references are torch's operators
@pytest.mark.parametrize("name,gn", [("2x4x8-c96", "silu"), ("1x12x12-c64", "none"), ("2x4x8-c96-oneslice", "affine")])
def test_vconv_reference_is_torch(name, gn):
    (x, ws, wt, bs, bt, a, b, act, N, Hh, Ww), _, _ = _vconv(name, gn)
    ref, _ = Z.vconv_ref(x, ws, wt, bs, bt, a, b, act, N, Hh, Ww, rounded=False)
    Cin = x.shape[1]
    v = x.double().reshape(N, 16, Hh, Ww, Cin)
    if a is not None:
        rep = lambda t: t.double().repeat_interleave(N // t.shape[0], 0)[:, None, None, None, :]
        v = v * rep(a) + rep(b)
        v = F_.silu(v) if act else v
    w4 = ws.double().reshape(128, 3, 3, Cin).permute(0, 3, 1, 2)
    t = F_.conv2d(v.reshape(N * 16, Hh, Ww, Cin).permute(0, 3, 1, 2), w4, bs.double(), padding=1)
    t = t.reshape(N, 16, 128, Hh * Ww).permute(0, 3, 2, 1).reshape(N * Hh * Ww, 128, 16)
    y = F_.conv1d(t, wt.double().reshape(128, 3, 128).permute(0, 2, 1), bt.double(), padding=1)
    want = y.reshape(N, Hh * Ww, 128, 16).permute(0, 3, 1, 2).reshape(-1, 128)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("name", ["3x8", "2x8-spike"])
def test_tattn_reference_is_torch(name):
    (x, wqkv, wproj, bqkv, bproj, gamma, beta, N, HW), _, _, _ = _tattn(name)
    ref, _, _ = Z.tattn_ref(x, wqkv, wproj, bqkv, bproj, gamma, beta, N, HW, rounded=False)
    C, ch = 256, 64
    xd = x.double().view(N, 16, HW, C)
    h = F_.group_norm(xd.permute(0, 2, 3, 1).reshape(N * HW, C, 16), 32, gamma.double(), beta.double(), eps=Z.GN_EPS)   # [(n pixel), C, f]
    qkv = h.permute(0, 2, 1) @ wqkv.double().t() + bqkv.double()                                                        # [(n pixel), f, 3C]
    q, k, v = (t.reshape(N * HW, 16, 4, ch).permute(0, 2, 1, 3) for t in qkv.split(C, dim=-1))
    o = (torch.softmax(q @ k.transpose(-1, -2) * ch ** -0.5, -1) @ v).permute(0, 2, 1, 3).reshape(N, HW, 16, C).permute(0, 2, 1, 3)
    want = (xd + o @ wproj.double().t() + bproj.double()).reshape(-1, C)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())


# --------------------------------------------------------------------------- clean emulations: zero violations
@pytest.mark.parametrize("name,gn", VC)
def test_vconv_clean_emulation_is_inside_the_bound(name, gn):
    ops, ref, bound = _vconv(name, gn)
    y = Z.emu_vconv(*ops)
    ratio = E.check(y, ref, bound, pixels=ops[9] * ops[10], what=f"emulated vconv2d1d {name} gn={gn}")
    print(f"\nRATIO emulated vconv2d1d {name} gn={gn}: {ratio:.3f}  (store term / bound, median: {float((E.U16 * ref.abs() / bound).median()):.2f})")


@pytest.mark.parametrize("name", TA)
def test_tattn_clean_emulation_is_inside_the_bound(name):
    ops, ref, bound, validity = _tattn(name)
    assert validity < 0.5
    y = Z.emu_tattn(*ops)
    ratio = E.check(y, ref, bound, what=f"emulated tattn_block {name}")
    print(f"\nRATIO emulated tattn_block {name}: {ratio:.3f}  max sum p eta {validity:.3g}  (store term / bound, median: {float((E.U16 * ref.abs() / bound).median()):.2f})")


# --------------------------------------------------------------------------- seeded defects
def _vconv_applicable(defect, name, gn):
    _, N, Hh, Ww, Cin, S, _ = next(c for c in Z.VCONV_CASES if c[0] == name)
    if defect == "pad_normalised":
        return gn != "none"
    if defect == "affine_next_chunk":
        return gn != "none" and Cin >= 64
    if defect == "cross_sample":
        return N > 1
    return True


@pytest.mark.parametrize("defect", Z.VCONV_DEFECTS)
def test_vconv_defect_is_flagged(defect):
    hits, worst, tried = [], 0.0, 0
    for name, gn in VC:
        if not _vconv_applicable(defect, name, gn):
            continue
        ops, ref, bound = _vconv(name, gn)
        nbad, ratio, _ = E.violations(Z.emu_vconv(*ops, defect=defect), ref, bound)
        tried += 1
        worst = max(worst, ratio)
        if nbad:
            hits.append(f"{name}/{gn}:{nbad}")
    print(f"\nDEFECT vconv {defect}: worst error/bound {worst:.3g}, flagged on {len(hits)} of {tried} cases: {' '.join(hits)}")
    assert hits, f"vconv defect {defect} is not flagged on any case (worst ratio {worst:.3g})"
    if defect in ("pad_normalised", "zero_frame", "cross_sample", "affine_next_chunk"):
        assert len(hits) == tried                         # these touch every block of every launch they apply to


@pytest.mark.parametrize("defect", Z.TATTN_DEFECTS)
def test_tattn_defect_is_flagged(defect):
    hits, worst = [], 0.0
    for name in TA:
        ops, ref, bound, _ = _tattn(name)
        nbad, ratio, _ = E.violations(Z.emu_tattn(*ops, defect=defect), ref, bound)
        worst = max(worst, ratio)
        if nbad:
            hits.append(f"{name}:{nbad}")
    print(f"\nDEFECT tattn {defect}: worst error/bound {worst:.3g}, flagged on {len(hits)} of {len(TA)} cases: {' '.join(hits)}")
    if defect in Z.TATTN_BLIND:
        assert not hits, f"tattn defect {defect} is documented as a blind spot but is flagged: correct errbound_fused's docstring"
    else:
        assert hits, f"tattn defect {defect} is not flagged on any case (worst ratio {worst:.3g})"


# --------------------------------------------------------------------------- the stated blind spots
def test_double_rounding_of_an_intermediate_is_evaluated():
    """Evaluated, not hidden: per case the violations, the share of output elements whose bits differ from the clean emulation (the
    stand-in for the unfused path, which has the same rounding points) and the rel-L2 distance from it."""
    flagged = {}
    for what, keys, get, fn, defect in (("vconv T", [(n, g) for n, g in VC if g == "silu"], _vconv, Z.emu_vconv, "double_round_T"),
                                        ("tattn O", [(n,) for n in TA], _tattn, Z.emu_tattn, "double_round_O")):
        for key in keys:
            ops, ref, bound = get(*key)[:3]
            clean, bad = fn(*ops), fn(*ops, defect=defect)
            nbad, ratio, _ = E.violations(bad, ref, bound)
            moved = float((clean.view(torch.int16) != bad.view(torch.int16)).float().mean())
            dist = rel_l2(bad.double(), clean.double())
            flagged[(what, key[0])] = nbad
            print(f"\nBLIND SPOT {what} {'/'.join(key)}: {nbad} of {bad.numel()} elements outside the bound, worst ratio {ratio:.3f}, "
                  f"{100 * moved:.1f} % of the bits differ, rel-L2 {dist:.2e}")
            if what == "vconv T":
                assert moved > 0.03                       # test_vconv_vs_two_launch_path's "> 97 % bitwise equal" sees it on every case
    assert flagged[("vconv T", "1x4x4-c32")] > 0          # the metric itself sees it only where the bound is tightest (one chunk, K = 288)
    assert not any(n for (what, _), n in flagged.items() if what == "tattn O")
