"""The element-wise metric of tests/errbound_fwd.py (GroupNorm forward, layout-edge convolutions, resample, statistics records,
bilinear_concat), proven on the CPU.

1. The float64 references equal torch's own float64 operators (`F.group_norm` + FiLM + SiLU, `F.conv3d` with the tap list scattered into
   a dense kernel, `F.avg_pool2d`, nearest / bilinear `F.interpolate`) to 1e-12 on every shape of the case lists in tests/errbound_fwd.py
   (tests/test_elementwise_fwd_norm_gpu.py, tests/test_elementwise_fwd_edge_gpu.py and tests/test_elementwise_fwd_misc_gpu.py iterate
   over the same lists), the grid-stride shapes included in full.
2. A faithful emulation of each kernel - fp32 torch arithmetic, the sums in the kernel's own order where the bound depends on it
   (gn_small: the thread's chain, then the chain over the quads; gn_group: chain, 64-lane butterfly, LDS fold; records: a 256-term
   chain), one round-to-nearest store - has ZERO violating elements on every GPU shape.  That is the evidence that the bounds are not
   too tight; it held before anything ran on a GPU.
3. Seeded defects, each flagged by `check`.  DEFECT_LOG records for each whether the whole-tensor assertion of the kernel's existing
   GPU test would have passed the same emulated output (test_ops_gpu.py / test_round3_gpu.py: rel-L2 < 1e-2 bf16, 2e-5 fp32;
   test_round6_gpu.py::test_gn_group_one_launch: 4e-3 bf16, 2e-6 fp32; test_ops_gpu.py::test_gn_finalize_from_producer_statistics:
   rel-L2 of a, b < 1e-5; the records: max |err| / max |ref| < 2e-6; test_sr_gpu.py::test_bilinear_concat_kernel: allclose 1e-5 / 1e-6):

       defect                                                                  error     old tolerance
       gn_apply bf16: truncating store                                         3.4e-03   PASSES (1e-2)
       gn_apply bf16: SiLU of the bf16-rounded affine                          2.6e-03   PASSES (1e-2)
       gn_apply bf16: last row of a slice takes the next slice's affine        8.6e-03   PASSES (1e-2)
       gn_apply f32: channels >= 1024 take a / b of the first pass             2.1e-01   fails
       gn_small f32: unbiased variance                                         6.7e-03   fails
       gn_small bf16: count of 16 rows instead of Tn                           7.7e-01   fails
       gn_small f32: eps dropped                                               2.1e-06   PASSES (2e-5)
       gn_group bf16: unbiased variance                                        3.0e-03   PASSES (4e-3)
       gn_group f32: count of 16 rows instead of Tn                            3.3e-01   fails
       gn_group f32: eps dropped                                               1.7e-06   PASSES (2e-6) *
       gn_finalize_stats: last record of a slice dropped                       5.4e-02   fails
       gn_finalize_stats: fp32 E[x^2] - mean^2 at mean = 8 std                 2.2e-06   PASSES (1e-5)
       stem strip bf16: w = W - 1 tap of a strip's last pixel reads the next image row  9.6e-02   fails
       head strip f32: w = W - 1 tap of a strip's last pixel reads the next image row   2.2e-01   fails
       stem mfma bf16: df = +1 tap of the last frame reads the next sample     1.3e-01   fails
       head coop bf16: df = +1 tap of the last frame reads the next sample     2.1e-01   fails
       head coop f32: bias added by every lane of a row                        9.0e+00   fails
       head strip bf16: clamped taps of a partly filled group counted again    1.8e-01   fails
       resample bf16: the pool divides after a bf16 rounding of the sum        2.3e-03   PASSES (1e-2)
       records: a record misses its 64th row                                   3.1e-02   fails
       records: summed from the values before the store rounding               8.0e-04   fails
       resample f32: the upsample uses fh for both axes                        1.1e+00   fails
       bilinear: align_corners=True coordinates                                4.1e-01   fails
       bilinear: neighbour index not clamped at the last row                   9.4e-02   fails
   (the numbers of one run; the tests print them with -s; the labels are the strings of the code).  Eight of the twenty-four pass the
   tolerance their kernel is held to today: every rounding defect, the eps and cancellation defects, and one single-row border defect;
   test_defects_the_old_tolerances_pass asserts exactly this set.  (*) A narrow pass: gn_group's dropped eps sits only 15 % under its
   old tolerance, on one seeded input (group variance 2.3, so eps / (2 var) = 2.2e-6 relative on rstd); at a smaller variance it
   would fail the old tolerance, at a larger one it would drop under the bound's own fp32 budget.  It counts among the eight with
   that caveat.  No stem / head defect passes its old
   tolerance at these shapes: the frames are so small (5 x 8 pixels) that one border column is a fifth of the tensor; on the 64 x 64
   frames of test_ops_gpu.py the same defects touch 1 / 64 of the rows.  The same holds for the records and for bilinear_concat, whose
   old assertions are already element-wise.  (A pool that rounds its sum to bf16 before dividing by 4 is no defect at all: the division
   commutes with the rounding; it shows with the odd factor 3 only.)
4. Every kernel variant named in errbound_fwd.VARIANTS / EDGE_VARIANTS is reached by at least one case.
"""
import pytest
import torch
import torch.nn.functional as F_

import errbound as E
import errbound_bwd as B
import errbound_fwd as W
from helpers import rel_l2

BF, F32 = torch.bfloat16, torch.float32
DT = W.DT
DEFECT_LOG = {}


def _close12(a, b):
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def _log(name, got, ref, tol):
    r = rel_l2(got.double(), ref)
    DEFECT_LOG[name] = (r, r < tol)
    print(f"\nDEFECT {name}: rel-L2 {r:.2e} -> the old tolerance {tol:g} {'PASSES' if r < tol else 'fails'} it")


def _flagged(y, ref, bound):
    return E.violations(y, ref, bound)[0] > 0


def _torch_gn(x, gamma, beta, film, slices, act):
    """F.group_norm per slice in float64, FiLM and SiLU on top: [S, Tn, C]."""
    C = x.shape[1]
    xs = x.double()[slices]                                                           # [S, Tn, C]
    y = F_.group_norm(xs.permute(0, 2, 1), 32, gamma.double(), beta.double(), eps=W.GN_EPS).permute(0, 2, 1)
    if film is not None:
        y = y * (1 + film.double()[:, None, :C]) + film.double()[:, None, C:]
    return F_.silu(y) if act else y


# --------------------------------------------------------------------------- gn_apply
@pytest.mark.parametrize("case", W.apply_cases(), ids=lambda c: c[0])
def test_apply_reference_and_emulation(case):
    name, dt, C, kind, N, Tn, HW, big, strided = case
    x, a, b, slices, geom = W.apply_inputs(dt, C, kind, N, Tn, HW, big)
    xs = x[slices]
    for act in (False, True):
        ref, bound = W.apply_ref(xs, a, b, act, DT[dt])
        assert float(ref.abs().max()) < 40                                           # the validity range of the silu_f bound
        y = W.emu_apply(xs, a, b, act, DT[dt])
        E.check(y.flatten(0, 1), ref.flatten(0, 1), bound.flatten(0, 1), what=f"emulated gn_apply {name} act={act}")
    if Tn > 1:
        # float64 a, b in place of the stored ones: the GroupNorm of torch (Tn = 1, cpg = 1 has zero variance: rstd = eps**-0.5 amplifies the last bit)
        _, gamma, beta, film, _, _ = W.gn_inputs(dt, C, kind, N, Tn, HW, 20.0 if big else 0.0, 21)
        f = B.gn_fwd_ref(x, gamma, beta, film, slices)
        act = kind.startswith("per_sample")
        ref, _ = W.apply_ref(xs, f["a"], f["b"], act, DT[dt])
        want = _torch_gn(x, gamma, beta, film, slices, act)
        assert float((ref - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())) * (1 + (400.0 if big else 0.0))   # (mean / std)^2 conditioning of the big-mean inputs


def _apply_defect(dt, C, kind, Tn, defect, act, name):
    x, a, b, slices, _ = W.apply_inputs(dt, C, kind, 2, Tn, 3, False)
    xs = x[slices]
    ref, bound = W.apply_ref(xs, a, b, act, DT[dt])
    y = W.emu_apply(xs, a, b, act, DT[dt], defect)
    assert _flagged(y.flatten(0, 1), ref.flatten(0, 1), bound.flatten(0, 1)), name
    _log(name, y, ref, 1e-2 if dt == "bf16" else 2e-5)


def test_apply_defects_are_flagged():
    _apply_defect("bf16", 320, "per_sample", 30, "trunc", True, "gn_apply bf16: truncating store")
    _apply_defect("bf16", 320, "per_sample", 30, "double_round", True, "gn_apply bf16: SiLU of the bf16-rounded affine")
    _apply_defect("bf16", 320, "spatial", 30, "next_affine", False, "gn_apply bf16: last row of a slice takes the next slice's affine")
    _apply_defect("f32", 1056, "per_sample_film", 30, "first_pass_ab", True, "gn_apply f32: channels >= 1024 take a / b of the first pass")


# --------------------------------------------------------------------------- gn_small / gn_group
def _two_pass(kernel, dt, C, kind, N, Tn, HW, big, film, acts, name):
    x, gamma, beta, fl, slices, _ = W.gn_inputs(dt, C, kind, N, Tn, HW, big, 51, film=film)
    for act in acts:
        r = W.two_pass_ref(x, gamma, beta, fl, slices, act, DT[dt], kernel)
        assert float(r["y"].abs().max()) < 40
        _close12(r["y"][slices], _torch_gn(x, gamma, beta, fl, slices, act))
        e = W.emu_two_pass(x, gamma, beta, fl, slices, act, DT[dt], kernel)
        what = f"emulated gn_{kernel} {name} act={act}"
        E.check(e["y"], r["y"], r["e_y"], what=what + ": y")
        for k in ("a", "b", "mean", "rstd"):
            E.check(e[k], r[k], r["e_" + k], what=f"{what}: {k}")


@pytest.mark.parametrize("case", W.small_cases(), ids=lambda c: c[0])
def test_small_reference_and_emulation(case):
    name, dt, C, kind, N, Tn, HW, big = case
    _two_pass("small", dt, C, kind, N, Tn, HW, big, False, (False, True), name)


@pytest.mark.parametrize("case", W.group_cases(), ids=lambda c: c[0])
def test_group_reference_and_emulation(case):
    name, dt, C, kind, N, Tn, HW, big, film, act, mode, strided = case
    _two_pass("group", dt, C, kind, N, Tn, HW, big, film, (act,), name)


def _two_pass_defect(kernel, dt, C, Tn, defect, name, tol):
    x, gamma, beta, fl, slices, _ = W.gn_inputs(dt, C, "per_sample", 2, Tn, 1, 0.0, 51, film=False)
    r = W.two_pass_ref(x, gamma, beta, fl, slices, True, DT[dt], kernel)
    e = W.emu_two_pass(x, gamma, beta, fl, slices, True, DT[dt], kernel, defect)
    assert _flagged(e["y"], r["y"], r["e_y"]), name
    if kernel == "group":
        assert _flagged(e["a"], r["a"], r["e_a"]) and _flagged(e["rstd"], r["rstd"], r["e_rstd"]), name
    _log(name, e["y"], r["y"], tol)


def test_two_pass_defects_are_flagged():
    _two_pass_defect("small", "f32", 384, 5, "unbiased", "gn_small f32: unbiased variance", 2e-5)
    _two_pass_defect("small", "bf16", 384, 5, "count16", "gn_small bf16: count of 16 rows instead of Tn", 1e-2)
    _two_pass_defect("small", "f32", 128, 5, "no_eps", "gn_small f32: eps dropped", 2e-5)
    _two_pass_defect("group", "bf16", 128, 37, "unbiased", "gn_group bf16: unbiased variance", 4e-3)
    _two_pass_defect("group", "f32", 128, 37, "count16", "gn_group f32: count of 16 rows instead of Tn", 2e-6)
    _two_pass_defect("group", "f32", 128, 37, "no_eps", "gn_group f32: eps dropped", 2e-6)


# --------------------------------------------------------------------------- gn_finalize_stats
def _explicit_gn_from_moments(rec, C, S, Tn, gamma, beta, film):
    """The affine from the record sums, written independently of finalize_ref: per-channel loops over groups in float64."""
    cpg = C // 32
    r = rec.double().reshape(S, Tn // 64, C // 4, 2).sum(1)                            # [S, C / 4, 2]
    a, b = torch.empty(S, C, dtype=torch.float64), torch.empty(S, C, dtype=torch.float64)
    for g in range(32):
        q = r[:, g * cpg // 4:(g + 1) * cpg // 4].sum(1) / (Tn * cpg)
        mean, var = q[:, 0], q[:, 1] - q[:, 0] ** 2
        rstd = 1 / torch.sqrt(var + W.GN_EPS)
        for c in range(g * cpg, (g + 1) * cpg):
            sc = 1 + film[:, c].double() if film is not None else 1.0
            sh = film[:, C + c].double() if film is not None else 0.0
            a[:, c] = rstd * gamma[c].double() * sc
            b[:, c] = (beta[c].double() - mean * rstd * gamma[c].double()) * sc + sh
    return a, b


@pytest.mark.parametrize("case", W.finalize_cases(), ids=lambda c: c[0])
def test_finalize_reference_and_emulation(case):
    name, C, S, nrec, ratio, film, strided = case
    rec, gamma, beta, fl = W.finalize_inputs(C, S, nrec, ratio, film)
    r = W.finalize_ref(rec, C, S, nrec * 64, gamma, beta, fl)
    a, b = _explicit_gn_from_moments(rec, C, S, nrec * 64, gamma, beta, fl)
    _close12(r["a"], a)
    assert float((r["b"] - b).abs().max()) <= 1e-12 * (1 + ratio) ** 2 * max(1.0, float(b.abs().max()))
    assert abs(float((r["mean"] * r["rstd"]).median()) - ratio) < 0.35 * max(1.0, ratio)          # the inputs have the stated mean / std
    e = W.emu_finalize(rec, C, S, nrec * 64, gamma, beta, fl)
    for k in ("a", "b", "mean", "rstd"):
        E.check(e[k], r[k], r["e_" + k], what=f"emulated gn_finalize_stats {name}: {k}")


def test_finalize_defects_are_flagged():
    for cname, defect, name in (("strided", "drop_last_record", "gn_finalize_stats: last record of a slice dropped"),
                                ("mean-8-std", "fp32_var", "gn_finalize_stats: fp32 E[x^2] - mean^2 at mean = 8 std")):
        _, C, S, nrec, ratio, film, _ = next(c for c in W.finalize_cases() if c[0] == cname)
        rec, gamma, beta, fl = W.finalize_inputs(C, S, nrec, ratio, film)
        r = W.finalize_ref(rec, C, S, nrec * 64, gamma, beta, fl)
        e = W.emu_finalize(rec, C, S, nrec * 64, gamma, beta, fl, defect)
        assert _flagged(e["a"], r["a"], r["e_a"]) and _flagged(e["rstd"], r["rstd"], r["e_rstd"]), name
        _log(name, e["a"], r["a"], 1e-5)


# --------------------------------------------------------------------------- add_rowbias
@pytest.mark.parametrize("case", W.ROWBIAS_CASES, ids=str)
def test_rowbias_reference_and_emulation(case):
    dt, N, rps, C, strided = case
    x, e = W.rowbias_inputs(dt, N, rps, C)
    ref, bound = W.rowbias_ref(x, e, rps, DT[dt])
    _close12(ref.reshape(N, rps, C), x.double().reshape(N, rps, C) + e.double()[:, None])
    E.check(W.emu_rowbias(x, e, rps), ref, bound, what=f"emulated add_rowbias {case}")
    if dt == "bf16":
        assert _flagged(W._trunc_bf16(x.float() + e.repeat_interleave(rps, 0)), ref, bound)
    if N > 1:
        assert _flagged(W.emu_rowbias(x, e.roll(1, 0), rps), ref, bound)                # the bias of the neighbouring sample


# --------------------------------------------------------------------------- stem / head convolutions
def _torch_conv(x5, w, bias, taps):
    """F.conv3d in float64 with the tap list scattered into a dense kernel: x5 [N, F, Cin, H, W], w packed [ntaps, Cin, Cout] -> rows."""
    r = [max(abs(t[i]) for t in taps) for i in range(3)]
    k = torch.zeros(w.shape[2], w.shape[1], 2 * r[0] + 1, 2 * r[1] + 1, 2 * r[2] + 1, dtype=torch.float64)
    for t, (a, b, c) in enumerate(taps):
        k[:, :, a + r[0], b + r[1], c + r[2]] = w[t].double().t()
    y = F_.conv3d(x5.double().permute(0, 2, 1, 3, 4), k, None if bias is None else bias.double(), padding=r)     # [N, Cout, F, H, W]
    return W.api_to_rows(y.permute(0, 2, 1, 3, 4))


def _edge_operands(c):
    x, w, bias = W.edge_inputs(c)
    dims = (c["F"], c["H"], c["W"])
    if "Cout" in c:
        return W.api_to_rows(x), x, w, bias, dims, DT[c["dt"]]
    return x, W.rows_to_api(x, c["N"], c["F"], c["H"], c["W"]), w, bias, dims, F32


@pytest.mark.parametrize("c", W.stem_cases() + W.head_cases(), ids=lambda c: c["name"])
def test_edge_reference_and_emulation(c):
    rows, x5, w, bias, dims, odt = _edge_operands(c)
    taps = W.TAPS[c["taps"]]
    ref, bound = W.edge_ref(rows, w, bias, taps, dims, odt)
    _close12(ref, _torch_conv(x5, w, bias, taps))
    E.check(W.emu_edge(rows, w, bias, taps, dims, odt), ref, bound, what=f"emulated {c['name']}")


def _edge_defect(cases, cname, defect, name, tol):
    c = next(c for c in cases if c["name"] == cname)
    rows, _, w, bias, dims, odt = _edge_operands(c)
    taps = W.TAPS[c["taps"]]
    ref, bound = W.edge_ref(rows, w, bias, taps, dims, odt)
    y = W.emu_edge(rows, w, bias, taps, dims, odt, defect, lpr=c.get("lpr", 1))
    assert _flagged(y, ref, bound), name
    _log(name, y, ref, tol)


def test_edge_defects_are_flagged():
    _edge_defect(W.stem_cases(), "strip-2x3x12-bf16", "next_row", "stem strip bf16: w = W - 1 tap of a strip's last pixel reads the next image row", 1e-2)
    _edge_defect(W.head_cases(), "strip-l4-3x5x8-o3-27-f32", "next_row", "head strip f32: w = W - 1 tap of a strip's last pixel reads the next image row", 2e-5)
    _edge_defect(W.stem_cases(), "mfma-4x2x32-t3-bf16", "next_sample", "stem mfma bf16: df = +1 tap of the last frame reads the next sample", 1e-2)
    _edge_defect(W.head_cases(), "coop-o4-27-bf16", "next_sample", "head coop bf16: df = +1 tap of the last frame reads the next sample", 2e-5)
    _edge_defect(W.head_cases(), "coop-w6-27-f32", "bias_per_lane", "head coop f32: bias added by every lane of a row", 2e-5)
    _edge_defect(W.head_cases(), "strip-l8-2x3x8-o2-5-bf16", "tap_group", "head strip bf16: clamped taps of a partly filled group counted again", 2e-5)


def test_every_edge_variant_is_reached():
    missing = set(W.EDGE_VARIANTS) - W.edge_variants_reached()
    assert not missing, missing
    T = W.TAPS
    assert W.stem_variant("bf16", 1, 32, 32, T["5"], 32) == "strip" and W.stem_variant("bf16", 1, 32, 32, T["a3"], 32) == "mfma"    # offsets of +-2
    assert W.stem_variant("bf16", 3, 32, 64, T["27"], 64) == "strip" and W.stem_variant("f32", 3, 32, 64, T["9"], 64) == "strip"    # K = 81; fp32
    assert W.stem_variant("bf16", 3, 32, 64, T["9"], 68) == "strip"                                                                  # ldy % 8
    assert W.head_variant("bf16", 128, 3, 27, 64) == ("strip", 16, 3) and W.head_variant("bf16", 128, 3, 27, 64, False) == ("coop", 16, 4)
    assert W.head_variant("bf16", 256, 6, 27, 8) is None and W.head_variant("f32", 48, 3, 27, 8) == ("plain", 12, 4)


# --------------------------------------------------------------------------- resample, records, bilinear
def _torch_resample(x, NF, Hh, Ww, fh, fw, mode, scale):
    v = x.double().reshape(NF, Hh, Ww, -1).permute(0, 3, 1, 2)                                  # [NF, C, H, W]
    y = F_.avg_pool2d(v, (fh, fw)) if mode == 0 else F_.interpolate(v, scale_factor=(fh, fw), mode="nearest")
    return (y * scale).permute(0, 2, 3, 1).reshape(-1, x.shape[1])


@pytest.mark.parametrize("case", W.resample_cases(), ids=lambda c: c[0])
def test_resample_reference_and_emulation(case):
    name, dt, NF, Hh, Ww, C, fh, fw, mode, scale, strided, stats = case
    x = W.resample_inputs(NF, Hh, Ww, C, dt)
    ref, bound = W.resample_ref(x, NF, Hh, Ww, fh, fw, mode, scale, DT[dt])
    _close12(ref, _torch_resample(x, NF, Hh, Ww, fh, fw, mode, scale))
    y = W.emu_resample(x, NF, Hh, Ww, fh, fw, mode, scale)
    E.check(y, ref, bound, what=f"emulated resample {name}")
    if stats:
        assert ref.shape[0] % 64 == 0 and scale == 1.0 and dt == "bf16"
        vals = W.record_values(y)
        r, _ = W.records_ref(vals)
        _close12(r[..., 0].sum(0), y.double().reshape(-1, C // 4, 4).sum((0, 2)))
        W.check_records(W.emu_records(vals), vals, f"emulated records {name}")


def test_resample_and_record_defects_are_flagged():
    name, dt, NF, Hh, Ww, C, fh, fw, mode, scale, _, _ = next(c for c in W.resample_cases() if c[0] == "pool2x2-bf16")
    x = W.resample_inputs(NF, Hh, Ww, C, dt)
    ref, bound = W.resample_ref(x, NF, Hh, Ww, fh, fw, mode, scale, DT[dt])
    assert not _flagged(W.emu_resample(x, NF, Hh, Ww, fh, fw, mode, scale, "bf16_sum"), ref, bound)      # a division by 4 commutes with the rounding: no defect to see
    c3 = next(c for c in W.resample_cases() if c[0] == "pool1x3-bf16")
    x3 = W.resample_inputs(*c3[2:6], "bf16")
    ref3, bound3 = W.resample_ref(x3, *c3[2:5], *c3[6:10], BF)
    y = W.emu_resample(x3, *c3[2:5], *c3[6:10], "bf16_sum")
    assert _flagged(y, ref3, bound3)
    _log("resample bf16: the pool divides after a bf16 rounding of the sum", y, ref3, 1e-2)
    good = W.emu_resample(x, NF, Hh, Ww, fh, fw, mode, scale)
    vals, rref = W.record_values(good), None
    rref, rb = W.records_ref(vals)
    for defect, label, pre in (("miss_row", "records: a record misses its 64th row", None),
                               ("prestore", "records: summed from the values before the store rounding", W.record_values(W.emu_resample(x, NF, Hh, Ww, fh, fw, mode, scale, prestore=True)))):
        rec = W.emu_records(vals, defect, pre)
        assert _flagged(rec.flatten(1), rref.flatten(1), rb.flatten(1)), label
        r = float((rec.double() - rref).abs().max() / rref.abs().max())
        DEFECT_LOG[label] = (r, r < 2e-6)
        print(f"\nDEFECT {label}: max |err| / max |ref| {r:.2e} -> the old tolerance 2e-06 {'PASSES' if r < 2e-6 else 'fails'} it")
    name, dt, NF, Hh, Ww, C, fh, fw, mode, scale, _, _ = next(c for c in W.resample_cases() if c[0] == "up1x3-f32")
    x = W.resample_inputs(NF, Hh, Ww, C, dt)
    ref, bound = W.resample_ref(x, NF, Hh, Ww, fh, fw, mode, scale, DT[dt])
    y = W.emu_resample(x, NF, Hh, Ww, fh, fw, mode, scale, "fh_both")
    assert _flagged(y, ref, bound)
    _log("resample f32: the upsample uses fh for both axes", y, ref, 2e-5)


@pytest.mark.parametrize("case", W.BILINEAR_CASES, ids=str)
def test_bilinear_reference_and_emulation(case):
    N, C, Hh, Ww, h, w = case
    _, low = W.bilinear_inputs(*case)
    ref, bound = W.bilinear_ref(low, Hh, Ww)
    _close12(ref, F_.interpolate(low.double(), (Hh, Ww), mode="bilinear", align_corners=False))
    flat = lambda t: t.reshape(-1, Ww)
    E.check(flat(W.emu_bilinear(low, Hh, Ww)), flat(ref), flat(bound), what=f"emulated bilinear {case}")
    E.check(flat(W.emu_bilinear(low, Hh, Ww).to(BF)), flat(ref), flat(E.U16 * (ref.abs() + bound) + bound), what=f"emulated bilinear rows bf16 {case}")


def test_bilinear_defects_are_flagged():
    case = W.BILINEAR_CASES[0]
    _, low = W.bilinear_inputs(*case)
    ref, bound = W.bilinear_ref(low, case[2], case[3])
    flat = lambda t: t.reshape(-1, case[3])
    for defect, label in (("align_corners", "bilinear: align_corners=True coordinates"), ("no_clamp", "bilinear: neighbour index not clamped at the last row")):
        y = W.emu_bilinear(low, case[2], case[3], defect)
        assert _flagged(flat(y), flat(ref), flat(bound)), label
        _log(label, y, ref, 1e-6)                                                       # test_sr_gpu.py holds it to F.interpolate


def test_chain_reference_emulation_and_threshold():
    """producer -> records -> gn_finalize_stats: the float64 affine of chain_ref normalises like F.group_norm; records summed in fp32
    and finalized in double stay inside its bound at means of 0.6 and 5 std; the stated mean^2 / var at which the bound on `a` passes
    half a bf16 ulp follows from the bound's own formula."""
    for m in (0.6, 5.0):
        g = torch.Generator().manual_seed(int(10 * m))
        S, Tn, C = 2, 256, 256
        y = (torch.randn(S * Tn, C, generator=g) + m).to(BF)
        gamma, beta, film = 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g), 0.3 * torch.randn(S, 2 * C, generator=g)
        r = W.chain_ref(y, gamma, beta, film, S)
        sl = torch.arange(S * Tn).reshape(S, Tn)
        want = _torch_gn(y, gamma, beta, film, sl, False)
        got = y.double().reshape(S, Tn, C) * r["a"][:, None] + r["b"][:, None]
        assert float((got - want).abs().max()) <= 1e-12 * (1 + m * m) * max(1.0, float(want.abs().max()))
        rec = W.emu_records(W.record_values(y))
        e = W.emu_finalize(rec, C, S, Tn, gamma, beta, film)
        for k in ("a", "b", "mean", "rstd"):
            E.check(e[k], r[k], r["e_" + k], what=f"emulated chain mean {m}: {k}")
        bad = W.emu_finalize(W.emu_records(W.record_values(y), "miss_row"), C, S, Tn, gamma, beta, film)
        assert _flagged(bad["a"], r["a"], r["e_a"])
    rr = W.CHAIN_RATIO_AT_HALF_ULP
    rel = (256 * (1 + rr) + 510 * (rr * (1 + rr)) ** 0.5) * E.U32 / 2
    assert abs(rel / 2.0 ** -9 - 1) < 0.02 and 80 < rr < 90




# --------------------------------------------------------------------------- head_gemm + head_gather
@pytest.mark.parametrize("case", W.HEAD_GEMM_CASES[:-1] + [("o1-27-cut", 1, "27", 9, 2, 8, 8, 9)], ids=lambda c: c[0])
def test_head_gemm_reference_and_emulation(case):
    """P and y against torch's own float64 operators (the 1025-group shape cut to 9 groups: the same rows per slice), the emulation inside
    all three bounds, and the stated blind spot: a dropped lo half stays inside the bound on P."""
    name, Co, tk, N, Fr, Hh, Ww, S = case
    taps, dims = W.TAPS[tk], (Fr, Hh, Ww)
    x, a, b, w, bias = W.head_gemm_inputs(Co, tk, N, Fr, Hh, Ww, S)
    M, NO = x.shape[0], len(taps) * Co
    xs = x.view(S, M // S, 128)
    hilo = W.host_head_gemm_pack(w)
    assert float((W.head_weight_rows(w).double() - hilo[0, :NO].double() - hilo[1, :NO].double()).abs().max()) <= 2.0 ** -17 * float(w.abs().max())
    Pref, eP = W.head_gemm_ref(xs, a, b, True, w, hilo)
    s = F_.silu(xs.double() * a.double()[:, None] + b.double()[:, None]).reshape(M, 128)
    _close12(Pref, W.head_weight_rows(w).double() @ s.t())
    yref, ey = W.head_gather_ref(Pref, bias, Co, taps, dims, eP)
    _close12(yref, _torch_conv(W.rows_to_api(s, N, Fr, Hh, Ww), w, bias, taps))
    P = W.emu_head_gemm(xs, a, b, True, hilo, NO)
    E.check(P, Pref, eP, what=f"emulated head_gemm {name}")
    y = W.emu_head_gather(P, bias, Co, taps, dims)
    E.check(y, *W.head_gather_ref(P, bias, Co, taps, dims), what=f"emulated head_gather {name}")
    E.check(y, yref, ey, what=f"emulated head_gemm + head_gather {name}")
    unmasked = W.emu_head_gather(P, bias, Co, taps, (1, 1, M))                          # a gather that ignores the frame borders
    assert _flagged(unmasked, *W.head_gather_ref(P, bias, Co, taps, dims))
    assert _flagged(W.emu_head_gemm(xs, a.roll(1, 0), b.roll(1, 0), True, hilo, NO), Pref, eP)      # the affine of the neighbouring slice
    assert not _flagged(W.emu_head_gemm(xs, a, b, True, hilo, NO, drop_lo=True), Pref, eP)          # the blind spot, as stated


# --------------------------------------------------------------------------- coverage of the kernel variants, summary
def test_every_variant_is_reached():
    missing = set(W.VARIANTS) - W.variants_reached()
    assert not missing, missing


def test_selection_rules():
    assert W.thread_shape("bf16", 96) == (1, 21, 4) and W.thread_shape("f32", 1056) == (2, 1, 0) and W.thread_shape("bf16", 2048) == (1, 1, 0)
    assert W.gn_apply_R("bf16", 256, 4100, 5) == (4096, 7) and W.gn_apply_R("bf16", 256, 6, 5) == (32, 0)
    assert W.gn_small_spb("bf16", 384) == (5, 16) and W.gn_small_spb("f32", 1024) == (1, 0)
    assert W.nchunks("bf16", 2048, 257) == 65 and W.nchunks("bf16", 32, 257) == 2 and W.nchunks("f32", 96, 30) == 1
    assert not W.gn_small_ok("f32", 2048, 16) and not W.gn_group_ok(2048, 257, 2048) and not W.gn_group_ok(128, 37, 170)


PASSES_OLD_TOLERANCE = {"gn_apply bf16: truncating store", "gn_apply bf16: SiLU of the bf16-rounded affine",
                        "gn_apply bf16: last row of a slice takes the next slice's affine", "gn_small f32: eps dropped",
                        "gn_group bf16: unbiased variance", "gn_group f32: eps dropped",
                        "gn_finalize_stats: fp32 E[x^2] - mean^2 at mean = 8 std",
                        "resample bf16: the pool divides after a bf16 rounding of the sum"}


def test_defects_the_old_tolerances_pass():
    """Exactly the eight defects of the module docstring's table pass the whole-tensor tolerance their kernel is held to today: the
    roundings, the eps and cancellation defects and one single-row border defect; the sixteen others do not.  The log is computed
    here, whatever ran before."""
    DEFECT_LOG.clear()
    for t in (test_apply_defects_are_flagged, test_two_pass_defects_are_flagged, test_finalize_defects_are_flagged, test_edge_defects_are_flagged,
              test_resample_and_record_defects_are_flagged, test_bilinear_defects_are_flagged):
        t()
    assert len(DEFECT_LOG) == 24, sorted(DEFECT_LOG)
    assert {k for k, (_, ok) in DEFECT_LOG.items() if ok} == PASSES_OLD_TOLERANCE, DEFECT_LOG
