"""CPU-side checks of DDIM inversion: the C ABI of mmd_slerp / mmd_slerp_ws_bytes, the float64 slerp of tests/ddim_invert_ref.py against
an independent numpy form, the restated kernel (its fp32 / fp64 emulation keeps the element-wise bound on every GPU shape, every seeded
defect breaks it), the level arithmetic of ddim_encode_loop / ddim_decode_loop, and every refused argument by its name."""
import os
import re

import numpy as np
import pytest
import torch

import ddim_invert_ref as R
from conftest import ROOT
from helpers import flags

NEW = ("mmd_slerp", "mmd_slerp_ws_bytes")


# ----------------------------------------------------------------------------- C ABI
def test_symbols_in_header_binding_and_library():
    from mm_diffusion import _hip, ops
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(_hip.lib(), name), name
    assert callable(ops.slerp) and callable(ops.slerp_workspace)


def test_workspace_size_depends_on_per_alone_per_row():
    from mm_diffusion import _hip
    ws = _hip.lib().mmd_slerp_ws_bytes
    for per in (1, 5, 2048, 2049, 196608, 2048 * 256, 2048 * 256 + 1, 1 << 31):
        one = ws(1, per)
        assert one > 0 and one % 24 == 0 and one <= 256 * 24, per
        assert ws(3, per) == 3 * one and ws(7, per) == 7 * one, per
    assert ws(1, 196608) == 96 * 24          # the base model's video latent: 96 workgroups per sample
    assert ws(0, 8) == 0 and ws(1, 0) == 0 and ws(-1, 8) == 0


def test_bad_arguments_return_codes_and_name_the_entry():
    from mm_diffusion import _hip
    lib = _hip.lib()
    # non-NULL pointers that are never dereferenced (the checks run before any launch), far enough apart not to overlap
    a, b, lam, out, ws = (1 << 20) * 1, (1 << 20) * 2, (1 << 20) * 3, (1 << 20) * 4, (1 << 20) * 5

    def refused(word, *args):
        assert lib.mmd_slerp(*args, None) < 0
        msg = lib.mmd_last_error()
        assert b"slerp:" in msg and word in msg, msg
    refused(b"needs a", None, b, lam, out, ws, 1, 8)
    refused(b"needs a", a, None, lam, out, ws, 1, 8)
    refused(b"lam", a, b, None, out, ws, 1, 8)
    refused(b"out", a, b, lam, None, ws, 1, 8)
    refused(b"ws", a, b, lam, out, None, 1, 8)
    refused(b"N", a, b, lam, out, ws, 0, 8)
    refused(b"N", a, b, lam, out, ws, -3, 8)
    refused(b"per", a, b, lam, out, ws, 1, 0)
    refused(b"per", a, b, lam, out, ws, 1, -1)
    refused(b"overlap", a, b, lam, a, ws, 1, 8)
    refused(b"overlap", a, b, lam, b, ws, 1, 8)
    refused(b"overlap", a, b, lam, a + 28, ws, 1, 8)          # out starts inside a's last element
    refused(b"overlap", a, b, lam, b - 4 * 15, ws, 2, 8)       # out ends inside b's first
    refused(b"overlap", a, a, lam, a, ws, 1, 8)


def test_cpu_tensors_and_shapes_raise_in_ops_slerp():
    from mm_diffusion import ops
    from mm_diffusion._hip import MMDError
    a, lam = torch.zeros(2, 8), torch.zeros(2)
    with pytest.raises(MMDError, match="CPU tensor"):
        ops.slerp(a, a.clone(), lam)


# ----------------------------------------------------------------------------- the float64 form and the bound
def _independent_slerp(a, b, lam):
    """slerp through unit vectors and the half-angle arctangent, no arccos: theta = 2 atan2(|a^ - b^|, |a^ + b^|), and the weights of a^, b^
    scaled back (the interpolation of mmd_slerp is that of the raw rows: w_a a + w_b b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty_like(a)
    for n in range(a.shape[0]):
        ah, bh = a[n] / np.linalg.norm(a[n]), b[n] / np.linalg.norm(b[n])
        theta = 2.0 * np.arctan2(np.linalg.norm(ah - bh), np.linalg.norm(ah + bh))
        l = float(lam[n])
        out[n] = (np.sin((1 - l) * theta) * a[n] + np.sin(l * theta) * b[n]) / np.sin(theta)
    return out


@pytest.mark.parametrize("per", [p for p in R.PERS if p > 1])
def test_float64_slerp_matches_an_independent_form(per):
    a, b, lam = R.slerp_case(3, per)
    y, wa, wb = R.slerp64(a, b, lam)
    want = _independent_slerp(a, b, lam)
    assert np.abs(y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # |slerp| interpolates the norms' geometry: on unit rows the result is a unit row
    ah = a.astype(np.float64) / np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True)
    bh = b.astype(np.float64) / np.linalg.norm(b.astype(np.float64), axis=1, keepdims=True)
    yh, _, _ = R.slerp64(ah, bh, lam)
    assert np.abs(np.linalg.norm(yh, axis=1) - 1.0).max() <= 1e-12


def test_float64_slerp_endpoints_and_chord_cases():
    a, b, _ = R.slerp_case(3, 1025)
    for l, want in ((0.0, a), (1.0, b)):
        y, wa, wb = R.slerp64(a, b, np.full(3, l, np.float32))
        assert np.array_equal(wa, np.full(3, 1.0 - l)) and np.array_equal(wb, np.full(3, l))
        assert np.array_equal(y, want.astype(np.float64))
    lam = np.array([0.25, 0.5, 0.75], np.float32)
    for kind in ("same", "opposite", "zero"):
        a, b, _ = R.slerp_case(3, 768, kind)
        y, wa, wb = R.slerp64(a, b, lam)
        rows = slice(0, 1) if kind == "zero" else slice(None)
        assert np.array_equal(wa[rows], 1.0 - lam.astype(np.float64)[rows]) and np.array_equal(wb[rows], lam.astype(np.float64)[rows]), kind


ALL_CASES = [(N, per, kind) for N in R.NS for per in R.PERS for kind in ("random", "same", "opposite", "zero")]


@pytest.mark.parametrize("N,per,kind", ALL_CASES)
def test_emulated_kernel_keeps_the_bound_on_every_gpu_shape(N, per, kind):
    a, b, lam = R.slerp_case(N, per, kind)
    assert R.branch_margin_ok(a, b), "the case sits near the 0.9995 switch"
    y, wa, wb = R.slerp64(a, b, lam)
    bound = R.combine_bound(a, b, wa, wb, y)
    assert R.violations(R.emulate(a, b, lam), y, bound) == 0
    for l, want in ((0.0, a), (1.0, b)):          # the endpoints are the inputs, bit for bit
        got = R.emulate(a, b, np.full(N, l, np.float32))
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), l


def test_the_bound_is_tight_enough_to_matter():
    a, b, lam = R.slerp_case(3, 1025)
    y, wa, wb = R.slerp64(a, b, lam)
    bound = R.combine_bound(a, b, wa, wb, y)
    scale = np.abs(wa[:, None] * a) + np.abs(wb[:, None] * b)
    assert (bound <= 4.1 * R.U * scale + R.TINY).all()          # a few fp32 roundings of the terms, no more


@pytest.mark.parametrize("defect", ["range", "no_guard", "swap", "tail"])
def test_seeded_defects_break_the_bound(defect):
    flagged = 0
    for N in R.NS:
        for per in (1023, 1024, 1025, 768):
            for kind in (("same", "opposite") if defect == "no_guard" else ("random",)):
                a, b, lam = R.slerp_case(N, per, kind)
                y, wa, wb = R.slerp64(a, b, lam)
                bound = R.combine_bound(a, b, wa, wb, y)
                assert R.violations(R.emulate(a, b, lam), y, bound) == 0
                bad = R.violations(R.emulate(a, b, lam, defect=defect, prefill=-12345.0), y, bound)
                if defect == "no_guard":          # acos of a quotient that rounding may or may not have pushed past 1: some rows, not all
                    flagged += bad > 0
                else:
                    assert bad > 0, (N, per)
                    flagged += 1
    assert flagged > 0


def test_the_clamp_alone_is_redundant_behind_the_chord_test():
    for kind in ("random", "same", "opposite"):
        a, b, lam = R.slerp_case(3, 1025, kind)
        assert np.array_equal(R.emulate(a, b, lam).view(np.int32), R.emulate(a, b, lam, defect="no_clamp").view(np.int32)), kind


# ----------------------------------------------------------------------------- levels
def _diffusion(T, respacing=""):
    from mm_diffusion import multimodal_script_util as msu
    return msu.create_gaussian_diffusion(steps=T, noise_schedule="linear" if T >= 100 else "cosine", timestep_respacing=respacing)      # (linear betas pass 1 below T = 20)


@pytest.mark.parametrize("T,respacing", [(4, ""), (8, ""), (1000, ""), (1000, "8"), (1000, "4")])
def test_level_arithmetic(T, respacing):
    from mm_diffusion._hip import MMDError
    d = _diffusion(T, respacing)
    Tl = d.num_timesteps
    assert Tl == (int(respacing) if respacing else T)
    assert d.ddim_encode_indices() == R.encode_indices(Tl) == list(range(Tl - 1))
    assert d.ddim_decode_indices() == R.decode_indices(Tl) == list(range(Tl - 1, -1, -1)) == d._indices(False)
    for lvl in sorted({1, 2, Tl // 2, Tl - 1} - {0}):
        up, down = d.ddim_encode_indices(lvl), d.ddim_decode_indices(lvl)
        assert up == R.encode_indices(Tl, lvl) and down == R.decode_indices(Tl, lvl)
        assert len(up) == lvl and len(down) == lvl + 1
        # encode step i evaluates the model at level i and lands on i + 1; decode step i at level i and lands on i - 1: the encode
        # visits levels 0 ... l-1, the decode l ... 0, and the last table entry an encode step reads is alphas_cumprod[l], never the 0 pad
        assert [i + 1 for i in up][-1] == lvl == down[0] and down[-1] == 0 and up[0] == 0
        assert all(d.alphas_cumprod_next[i] == d.alphas_cumprod[i + 1] > 0 for i in up)
    assert d.alphas_cumprod_next[Tl - 1] == 0.0
    assert d.ddim_decode_indices(0) == [0]
    for bad in (0, -1, Tl, Tl + 1):
        with pytest.raises(MMDError, match="to_level"):
            d.ddim_encode_indices(bad)
    with pytest.raises(MMDError, match="alphas_cumprod_next"):
        d.ddim_encode_indices(Tl)
    for bad in (-1, Tl, Tl + 5):
        with pytest.raises(MMDError, match="from_level"):
            d.ddim_decode_indices(bad)
    for bad in (1.5, True, "3"):
        with pytest.raises(MMDError, match="to_level"):
            d.ddim_encode_indices(bad)


# ----------------------------------------------------------------------------- refusals
_TINY = {}


def _tiny():
    """the tiny model on the CPU (never run) and its respaced diffusion"""
    if not _TINY:
        from mm_diffusion import logger, multimodal_script_util as msu
        logger.set_quiet(True)
        fl = flags("tiny", timestep_respacing="8")
        _TINY["v"] = (fl,) + tuple(msu.create_model_and_diffusion(**fl))
    return _TINY["v"]


def _clip(fl, B=2, video=None, audio=None):
    return {"video": torch.zeros(B, *(video or fl["video_size"])), "audio": torch.zeros(B, *(audio or fl["audio_size"]))}


def _loops(diff, model, x):
    """every public inversion entry point as (label, the name of its state argument, call(**kw))"""
    return [("ddim_encode_loop", lambda **kw: diff.ddim_encode_loop(model, x, **kw)),
            ("ddim_encode_loop", lambda **kw: diff.ddim_encode_loop_progressive(model, x, **kw)),
            ("ddim_decode_loop", lambda **kw: diff.ddim_decode_loop(model, x, **kw)),
            ("ddim_decode_loop", lambda **kw: diff.ddim_decode_loop_progressive(model, x, **kw)),
            ("ddim_interpolate", lambda **kw: diff.ddim_interpolate(model, x, x, [0.5], **kw))]


def test_cpu_tensors_are_refused_by_name():
    from mm_diffusion._hip import MMDError
    fl, model, diff = _tiny()
    for who, call in _loops(diff, model, _clip(fl)):
        with pytest.raises(MMDError, match=who + r".*CPU tensor"):
            call()


def test_levels_out_of_range_are_refused_by_name():
    from mm_diffusion._hip import MMDError
    fl, model, diff = _tiny()
    x = _clip(fl)
    T = diff.num_timesteps
    assert T == 8
    for bad in (0, -2, T + 1):
        with pytest.raises(MMDError, match=r"ddim_encode_loop: to_level"):
            diff.ddim_encode_loop(model, x, bad)
        with pytest.raises(MMDError, match=r"ddim_interpolate: level"):
            diff.ddim_interpolate(model, x, x, [0.5], bad)
    for bad in (-1, T, T + 1):
        with pytest.raises(MMDError, match=r"ddim_decode_loop: from_level"):
            diff.ddim_decode_loop(model, x, bad)
    with pytest.raises(MMDError, match=r"to_level = 8 = T.*alphas_cumprod_next\[T-1\] is 0.*eps"):
        diff.ddim_encode_loop_progressive(model, x, T)
    with pytest.raises(MMDError, match=r"ddim_interpolate: level = 8 = T"):
        diff.ddim_interpolate(model, x, x, [0.5], T)


def test_eta_and_host_callables_are_refused_by_name():
    from mm_diffusion._hip import MMDError
    fl, model, diff = _tiny()
    x = _clip(fl)
    with pytest.raises(MMDError, match=r"ddim_encode_loop: eta"):
        diff.ddim_encode_loop(model, x, eta=0.5)
    with pytest.raises(MMDError, match=r"ddim_encode_loop: eta"):
        diff.ddim_encode_loop_progressive(model, x, 3, eta=1.0)
    for who, call in _loops(diff, model, x):
        with pytest.raises(MMDError, match=who + ": denoised_fn"):
            call(denoised_fn=lambda t: t)
        with pytest.raises(MMDError, match=who + ": cond_fn"):
            call(cond_fn=lambda *a, **k: None)


def test_shapes_that_do_not_match_the_model_are_refused_by_name():
    from mm_diffusion._hip import MMDError
    fl, model, diff = _tiny()
    F, C, Hh, Ww = fl["video_size"]
    wrong = [_clip(fl, video=[F, C, Hh, Ww + 1]), _clip(fl, video=[F + 1, C, Hh, Ww]), _clip(fl, audio=[1, fl["audio_size"][1] - 1]),
             {"video": torch.zeros(2, *fl["video_size"]), "audio": torch.zeros(3, *fl["audio_size"])},
             {"video": torch.zeros(2, *fl["video_size"])}, {"video": torch.zeros(2, C, Hh, Ww), "audio": torch.zeros(2, *fl["audio_size"])}]
    for x in wrong:
        for (who, call), name in zip(_loops(diff, model, x), ("x_start", "x_start", "latent", "latent", "a")):
            with pytest.raises(MMDError, match=who + ": " + name):
                call()
    good = _clip(fl)
    with pytest.raises(MMDError, match="ddim_interpolate: b"):
        diff.ddim_interpolate(model, good, wrong[0], [0.5])
    with pytest.raises(MMDError, match="ddim_interpolate: weights"):
        diff.ddim_interpolate(model, good, good, [])
    with pytest.raises(MMDError, match="ddim_interpolate: weights"):
        diff.ddim_interpolate(model, good, good, [0.5, float("nan")])


def test_the_sr_stage_raises_instead_of_inheriting_the_loops():
    from mm_diffusion import script_util as su
    from mm_diffusion._hip import MMDError
    from mm_diffusion.gaussian_diffusion import GaussianDiffusion
    from mm_diffusion.respace import SpacedDiffusion
    diff = su.create_gaussian_diffusion(diffusion_steps=1000,noise_schedule="linear", timestep_respacing="ddim4")
    assert isinstance(diff, GaussianDiffusion) and isinstance(diff, SpacedDiffusion)
    x = torch.zeros(1, 3, 8, 8)
    for fn in ("ddim_encode_loop", "ddim_encode_loop_progressive", "ddim_decode_loop", "ddim_decode_loop_progressive"):
        with pytest.raises(MMDError, match="SR stage"):
            getattr(diff, fn)(None, x)
    with pytest.raises(MMDError, match="SR stage"):
        diff.ddim_interpolate(None, x, x, [0.5])


def test_graph_stepper_refuses_cond_and_jump_length_by_name():
    from mm_diffusion._hip import MMDError
    from mm_diffusion.sampler import GraphStepper
    _, _, diff = _tiny()
    with pytest.raises(MMDError, match="jump_length.*ddim_reverse"):
        GraphStepper(diff, None, 2, "cuda", update="ddim_reverse", jump_length=2)
    with pytest.raises(MMDError, match="cond.*ddim_reverse"):
        GraphStepper(diff, None, 2, "cuda", update="ddim_reverse", cond={"video": object()})
    with pytest.raises(MMDError, match="ddim_reverse"):
        GraphStepper(diff, None, 2, "cuda", update="ddim_backward")


def test_timing_tool_parses_its_arguments():
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ddim_invert_bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 0 and b"--repeats" in p.stdout and b"--out" in p.stdout, p.stdout
