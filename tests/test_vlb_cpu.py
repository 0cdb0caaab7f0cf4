"""CPU-side checks of the variational-bound surface (bits / dim): the C ABI of the new entry points, the host methods with the reference's
names on both diffusion classes and both respacing wrappers, the KL loss types of the SR stage's training_losses, the tool, and the
self-consistency of the fixtures tools/gen_golden.py (group `vlb`) captured from the reference (tests/golden/README_vlb.md)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import gold

NEW_SYMBOLS = ("mmd_vlb_workspace_bytes", "mmd_vlb_terms", "mmd_vlb_terms_bwd")
METHODS = ("_vb_terms_bpd", "_prior_bpd", "calc_bpd_loop")
LN2 = np.log(2.0)


def test_new_entry_points_are_declared_exported_and_bound():
    from mm_diffusion import _hip
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    lib = _hip.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    # three doubles per (sample, chunk); the chunk count is the loss reduction's
    assert lib.mmd_vlb_workspace_bytes(4) * 2 == lib.mmd_loss_workspace_bytes(4) * 3
    # argument errors come back as codes with a message, before any launch
    assert lib.mmd_vlb_terms(None, None, None, None, None, None, 4, 1, 1, 1, 1, 0, None, None, None, 0, None, None, None) < 0
    assert b"vlb_terms" in lib.mmd_last_error()
    one = torch.zeros(8)
    p = one.data_ptr()
    # the clipped x0 prediction is not differentiable: refused, not ignored
    assert lib.mmd_vlb_terms_bwd(p, p, p, p, p, 4, 1, 1, 1, 1, 1, p, p, None) < 0 and b"clip" in lib.mmd_last_error()
    # eps_mse without the noise tensor; a result row shorter than the table
    assert lib.mmd_vlb_terms(p, p, None, p, p, p, 4, 1, 1, 1, 1, 0, p, p, p, 0, None, p, None) < 0 and b"noise" in lib.mmd_last_error()
    assert lib.mmd_vlb_terms(p, p, None, p, p, p, 4, 1, 1, 1, 1, 0, p, p, None, 3, None, p, None) < 0 and b"timesteps" in lib.mmd_last_error()


def test_both_classes_and_both_wrappers_have_the_bound_methods():
    from mm_diffusion import gaussian_diffusion as gd, multimodal_gaussian_diffusion as mgd, multimodal_respace, respace
    import inspect
    for cls in (gd.GaussianDiffusion, mgd.GaussianDiffusion, respace.SpacedDiffusion, multimodal_respace.SpacedDiffusion):
        for m in METHODS:
            assert callable(getattr(cls, m, None)), (cls, m)
        assert list(inspect.signature(cls._vb_terms_bpd).parameters)[:7] == ["self", "model", "x_start", "x_t", "t", "clip_denoised", "model_kwargs"]
        assert list(inspect.signature(cls.calc_bpd_loop).parameters)[:5] == ["self", "model", "x_start", "clip_denoised", "model_kwargs"]
        assert inspect.signature(cls.calc_bpd_loop).parameters["clip_denoised"].default is True
    from mm_diffusion.sampler import GraphStepper
    from mm_diffusion._hip import MMDError
    with pytest.raises(MMDError):          # the stepper knows ddpm, ddim and vlb; anything else is refused before an engine is built
        GraphStepper(None, None, 2, "cpu", update="nonsense")


def _sr_diffusion(**over):
    from mm_diffusion import script_util as su
    return su.create_gaussian_diffusion(diffusion_steps=1000, learn_sigma=True, timestep_respacing="4", **over)


def test_sr_kl_training_on_cpu_tensors_raises_mmderror_not_notimplemented():
    from mm_diffusion._hip import MMDError
    from mm_diffusion.multimodal_gaussian_diffusion import LossType
    diff = _sr_diffusion(use_kl=True)
    assert diff.loss_type == LossType.RESCALED_KL
    x0 = torch.zeros(2, 3, 8, 8)
    with pytest.raises(MMDError):
        diff.training_losses(lambda x, t, **kw: torch.zeros(2, 6, 8, 8), x0, torch.tensor([0, 3]))
    with pytest.raises(MMDError):
        diff.calc_bpd_loop(lambda x, t, **kw: torch.zeros(2, 6, 8, 8), x0)
    with pytest.raises(MMDError):
        diff._prior_bpd(x0)


def test_multimodal_kl_training_still_raises():
    from mm_diffusion import multimodal_script_util as msu
    diff = msu.create_gaussian_diffusion(steps=1000, learn_sigma=True, use_kl=True, timestep_respacing="4")
    x0 = {"video": torch.zeros(1, 2, 3, 4, 4), "audio": torch.zeros(1, 1, 16)}
    with pytest.raises(NotImplementedError):
        diff.multimodal_training_losses(None, x0, torch.tensor([1]))


# ------------------------------------------------------------------ fixtures: self-consistency (guards the generator)
def _prior_fp64(x0, ac_last):
    """normal_kl(sqrt(ac) x0, log(1 - ac), 0, 0) averaged per sample, in bits - fp64 from the schedule."""
    x0 = x0.astype(np.float64).reshape(x0.shape[0], -1)
    lv = np.log(1.0 - ac_last)
    return (0.5 * (-1.0 - lv + np.exp(lv) + ac_last * x0 ** 2)).mean(axis=1) / LN2


def _streams(tag):
    g = gold(tag)
    if tag.startswith("sr_"):
        return g, [("", g["x0"], {k: g[k] for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")})]
    return g, [(k, g[f"x0_{k}"], {n: g[f"{n}_{k}"] for n in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")}) for k in ("video", "audio")]


@pytest.mark.parametrize("tag", ["tiny_bpd", "tiny_ls_bpd", "sr_tiny_bpd"])
def test_bound_fixtures_are_self_consistent(tag):
    g, streams = _streams(tag)
    T = len(g["timestep_map"])
    assert g["alphas_cumprod"].shape == (T,) and g["alphas_cumprod"].dtype == np.float64
    for key, x0, r in streams:
        B = x0.shape[0]
        assert r["vb"].shape == r["xstart_mse"].shape == r["mse"].shape == (B, T) and r["total_bpd"].shape == r["prior_bpd"].shape == (B,)
        assert all(np.isfinite(v).all() for v in r.values())
        np.testing.assert_allclose(r["total_bpd"], r["vb"].sum(axis=1) + r["prior_bpd"], rtol=1e-6)
        # the reference evaluates 0.5 (-1 - lv + exp(lv) + mean^2) in fp32: O(1) terms cancel to ~1e-5, so the error is absolute - four
        # roundings of half an fp32 ulp of 1 (6e-8), halved, over ln 2: 1.7e-7 bits at worst, whatever the value
        np.testing.assert_allclose(r["prior_bpd"], _prior_fp64(x0, g["alphas_cumprod"][-1]), rtol=1e-5, atol=2e-7)
        assert (np.abs(x0) > 0.999).any() and np.abs(x0).max() <= 1.0        # both edge branches of the decoder NLL are in the data
        assert (r["vb"] >= 0).all() and (r["xstart_mse"] >= 0).all() and (r["mse"] >= 0).all()


def _decoder_nll_fp64(x0, mean, logvar):
    """-discretized_gaussian_log_likelihood (the tanh CDF approximation and the 1e-12 clamps are part of the definition), per-sample mean, bits."""
    x0, mean, logvar = (np.asarray(a, dtype=np.float64) for a in (x0, mean, logvar))
    cdf = lambda u: 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (u + 0.044715 * u ** 3)))       # noqa: E731
    cx, inv = x0 - mean, np.exp(-0.5 * logvar)
    cp, cm = cdf(inv * (cx + 1.0 / 255.0)), cdf(inv * (cx - 1.0 / 255.0))
    lp = np.where(x0 < -0.999, np.log(np.maximum(cp, 1e-12)),
                  np.where(x0 > 0.999, np.log(np.maximum(1.0 - cm, 1e-12)), np.log(np.maximum(cp - cm, 1e-12))))
    return (-lp).reshape(lp.shape[0], -1).mean(axis=1) / LN2


def test_fixed_variance_term_at_t0_is_the_decoder_nll_of_the_stored_arrays():
    """tiny_bpd (fixed large variance): sample 0 of the single-term call sits at t = 0; its posterior mean follows from the stored clipped
    pred_xstart and x_t through the schedule, its log-variance is the fixed one - everything the decoder NLL needs is in the file."""
    g = gold("tiny_bpd")
    assert int(g["term_t"][0]) == 0
    ac = g["alphas_cumprod"]
    betas = 1.0 - ac / np.append(1.0, ac[:-1])
    post_var = betas * (1.0 - np.append(1.0, ac[:-1])) / (1.0 - ac)
    c1 = betas[0] * 1.0 / (1.0 - ac[0])                      # sqrt(alphas_cumprod_prev[0]) = 1
    c2 = 0.0                                                  # (1 - alphas_cumprod_prev[0]) = 0
    logvar0 = np.log(post_var[1])                             # FIXED_LARGE at t = 0: log(posterior_variance[1])
    for key in ("video", "audio"):
        px0 = g[f"term_pred_xstart_{key}_clip1"][:1].astype(np.float64)
        mean = c1 * px0 + c2 * g[f"term_xt_{key}"][:1]
        want = _decoder_nll_fp64(g[f"x0_{key}"][:1], mean, np.full_like(mean, logvar0))
        got = g[f"term_output_{key}_clip1"][:1]
        print(f"{key}: decoder NLL at t=0 fixture {got} fp64 {want}")
        np.testing.assert_allclose(got, want, rtol=2e-3)       # the fixture is fp32 torch: tanh-CDF differences lose digits


def test_kl_training_fixture_follows_the_training_protocol():
    g, h = gold("sr_tiny_kl_train_grads"), gold("sr_tiny_train_grads")
    assert "loss" in g.files and "mse" not in g.files and "vb" not in g.files           # KL: terms["loss"] only
    assert list(g["names"]) == list(h["names"]) and list(g["t"]) == [0, 977] and g["loss"].shape == (2,)
    assert g["sub_off"][-1] == g["sub"].shape[0] and np.isfinite(g["sub"]).all() and (g["loss"] > 0).all()


def test_bpd_eval_tool_imports_and_prints_help_without_a_gpu():
    tool = os.path.join(ROOT, "tools", "bpd_eval.py")
    for extra in ([], ["--sr"]):
        out = subprocess.run([sys.executable, tool, *extra, "--help"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "--bench" in out.stdout and "--weights" in out.stdout and ("--sr_learn_sigma" if extra else "--video_size") in out.stdout
