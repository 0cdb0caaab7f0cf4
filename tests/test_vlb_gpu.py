"""The variational bound (bits / dim) on the HIP path: the mmd_vlb_terms / mmd_vlb_terms_bwd kernels against an fp64 restatement of
normal_kl / the discretized-Gaussian likelihood / the posterior written here, the host methods (_vb_terms_bpd, _prior_bpd, calc_bpd_loop)
against fixtures captured from the reference (tests/golden/README_vlb.md), graph replay against the eager path, and KL training.

Kernel tolerances are not fixed numbers: the decoder NLL subtracts two CDFs and is ill-conditioned, so each case evaluates the SAME formulas
with torch in fp32 on the CPU, measures that result's error against fp64, and allows the kernel twice that, per output (the factor covers
expf / tanhf / logf differing from the host's in the last bits)."""
import math

import numpy as np
import pytest
import torch

from helpers import gold, rel_l2

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)


# ------------------------------------------------------------------ the restatement (any dtype, autograd-friendly)
def cdf(u):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))


def terms_ref(x0, xt, noise, mo, tab, t, flags, dt):
    """-> vb [N], xstart_mse [N], eps_mse [N], pred_xstart, all in dtype `dt` on the CPU.  API layout [N, F, C(m), HW]; `tab` is the
    fp32 [7, T] device table (both precisions start from the same rounded coefficients)."""
    x0, xt, noise, tab = (a.detach().cpu().to(dt) for a in (x0, xt, noise, tab))
    mo = mo.to(dt)                                         # possibly a leaf of that dtype already (backward test): stays in the graph
    C = x0.shape[2]
    row = lambda r: tab[r][t.cpu()].view(-1, 1, 1, 1)      # noqa: E731
    cr, crm1, c1, c2, fixed, min_log, max_log = (row(r) for r in range(7))
    o = mo[:, :, :C]
    if flags & 4:
        frac = (mo[:, :, C:] + 1.0) / 2.0
        logvar = frac * max_log + (1.0 - frac) * min_log
    else:
        logvar = fixed.expand_as(x0)
    px0 = o if flags & 2 else cr * xt - crm1 * o
    if flags & 1:
        px0 = px0.clamp(-1.0, 1.0)
    mean, tmean = c1 * px0 + c2 * xt, c1 * x0 + c2 * xt
    kl = 0.5 * (-1.0 + logvar - min_log + torch.exp(min_log - logvar) + (tmean - mean) ** 2 * torch.exp(-logvar))
    cx, inv = x0 - mean, torch.exp(-0.5 * logvar)
    cp, cm = cdf(inv * (cx + 1.0 / 255.0)), cdf(inv * (cx - 1.0 / 255.0))
    lp = torch.where(x0 < -0.999, torch.log(cp.clamp(min=1e-12)),
                     torch.where(x0 > 0.999, torch.log((1.0 - cm).clamp(min=1e-12)), torch.log((cp - cm).clamp(min=1e-12))))
    mf = lambda a: a.flatten(1).mean(dim=1)                # noqa: E731
    vb = torch.where(t.cpu() == 0, mf(-lp), mf(kl)) / LN2
    eps = (cr * xt - px0) / crm1
    return vb, mf((px0 - x0) ** 2), mf((eps - noise) ** 2), px0


def diffusion(predict_xstart, var):
    from mm_diffusion import multimodal_script_util as msu
    return msu.create_gaussian_diffusion(steps=1000, learn_sigma=(var == "learned"), sigma_small=(var == "small"), predict_xstart=predict_xstart)


def case_inputs(diff, geom, predict_xstart, learned, seed):
    """Batch of 16 with t = 0, 1, middle, T-1 four times; x0 uniform in [-1, 1] with exact -1 / +1 entries (the |x| > 0.999 branches).
    The model output is a prediction of realistic quality: eps-prediction = noise + 20 %, x0-prediction = x0 + 30 % of the noise level
    of its timestep (at t = 0 the decoder's standard deviation is ~0.007: a prediction many deviations off would leave every likelihood
    on its 1e-12 clamp, where neither precision says anything)."""
    F, C, HW = geom
    g = torch.Generator().manual_seed(seed)
    N, T = 16, diff.num_timesteps
    t = torch.tensor([0, 1, T // 2, T - 1] * 4)
    x0 = torch.rand(N, F, C, HW, generator=g) * 2 - 1
    x0.view(-1)[::53] = -1.0
    x0.view(-1)[29::53] = 1.0
    noise = torch.randn(N, F, C, HW, generator=g)
    sa = torch.from_numpy(diff.sqrt_alphas_cumprod)[t].view(-1, 1, 1, 1)
    sb = torch.from_numpy(diff.sqrt_one_minus_alphas_cumprod)[t].view(-1, 1, 1, 1)
    xt = (sa * x0.double() + sb * noise.double()).float()
    pred = (x0 + 0.3 * sb.float() * torch.randn(N, F, C, HW, generator=g)) if predict_xstart else (noise + 0.2 * torch.randn(N, F, C, HW, generator=g))
    mo = torch.cat([pred, 0.6 * torch.randn(N, F, C, HW, generator=g)], dim=2) if learned else pred
    return x0, xt, noise, mo.contiguous(), t


def run_kernel(diff, x0, xt, noise, mo, t, geom, flags):
    from mm_diffusion import ops
    tab, _ = diff.device_tables(torch.device("cuda"))
    N = x0.shape[0]
    vb, xs, em = (torch.full((N,), float("nan"), device="cuda") for _ in range(3))
    px0 = torch.empty_like(x0, device="cuda")
    ops.vlb_terms(x0.cuda(), xt.cuda(), mo.cuda(), tab, t.cuda(), *geom, flags, vb, xstart_mse=xs, eps_mse=em, noise=noise.cuda(), pred_xstart=px0)
    torch.cuda.synchronize()
    return (vb.cpu(), xs.cpu(), em.cpu(), px0.cpu()), tab


GEOMS = {"video": (4, 3, 256), "audio": (1, 1, 2000)}


def worst(a, ref):
    """Largest error over the samples, relative to the largest fp64 value among them (vectors); rel-L2 for the pred_xstart tensor.  Not
    per-sample relative: with a good prediction the KL of a late timestep is a sum of O(1) terms that cancel to ~1e-6, and its rounding
    error is absolute."""
    if a.dim() > 1:
        return rel_l2(a, ref)
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("var", ["small", "large", "learned"])
@pytest.mark.parametrize("predict_xstart", [False, True])
@pytest.mark.parametrize("stream", ["video", "audio"])
def test_vlb_terms_kernel_against_fp64(stream, predict_xstart, var, clip):
    diff = diffusion(predict_xstart, var)
    geom = GEOMS[stream]
    flags = diff._flags(clip)
    assert flags == (1 if clip else 0) | (2 if predict_xstart else 0) | (4 if var == "learned" else 0)
    x0, xt, noise, mo, t = case_inputs(diff, geom, predict_xstart, var == "learned", seed=len(stream) + 2 * predict_xstart + 7 * clip)
    assert (x0.abs() > 0.999).any()
    got, tab = run_kernel(diff, x0, xt, noise, mo, t, geom, flags)
    ref64 = terms_ref(x0, xt, noise, mo, tab, t, flags, torch.float64)
    ref32 = terms_ref(x0, xt, noise, mo, tab, t, flags, torch.float32)
    assert all(torch.isfinite(r).all() for r in ref64)
    fails = []
    for name, g_, r32, r64 in zip(("vb", "xstart_mse", "eps_mse", "pred_xstart"), got, ref32, ref64):
        # the decoder-NLL samples (t = 0) and the KL samples apart: the former would hide the latter
        groups = [("all", slice(None))] if g_.dim() > 1 else [("t=0", t == 0), ("t>0", t != 0)]
        for gname, rows in groups:
            e_k, e_y = worst(g_[rows], r64[rows]), worst(r32[rows], r64[rows])
            print(f"{stream} x0-pred={predict_xstart} var={var} clip={clip} {name} {gname}: kernel {e_k:.3e}  fp32-on-CPU yardstick {e_y:.3e}")
            if not (torch.isfinite(g_).all() and e_k <= 2 * e_y):
                fails.append((name, gname, e_k, e_y))
    assert not fails, fails


def test_vlb_terms_is_bitwise_repeatable_and_tables_land_at_column_t():
    from mm_diffusion import ops
    diff = diffusion(False, "learned")
    geom = GEOMS["video"]
    x0, xt, noise, mo, t = case_inputs(diff, geom, False, True, seed=3)
    a, tab = run_kernel(diff, x0, xt, noise, mo, t, geom, 5)
    b, _ = run_kernel(diff, x0, xt, noise, mo, t, geom, 5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # result tables: sample n writes column t[n] of row n and nothing else; noise = None skips eps_mse
    T = diff.num_timesteps
    tabs = [torch.full((16, T), -7.0, device="cuda") for _ in range(2)]
    ops.vlb_terms(x0.cuda(), xt.cuda(), mo.cuda(), tab, t.cuda(), *geom, 5, tabs[0], xstart_mse=tabs[1])
    torch.cuda.synchronize()
    for k, full in enumerate(tabs):
        full = full.cpu()
        assert torch.equal(full[torch.arange(16), t], a[k])
        full[torch.arange(16), t] = -7.0
        assert bool((full == -7.0).all())


@pytest.mark.parametrize("predict_xstart", [False, True])
@pytest.mark.parametrize("stream", ["video", "audio"])
def test_vb_agrees_with_the_training_loss_vb(stream, predict_xstart):
    """Learned-range variance, clip off: mmd_loss_terms evaluates the same device function in fp32 (the reference's training precision),
    mmd_vlb_terms in double, so the two are not bitwise equal.  Bound: every element of the fp32 evaluation passes through at most three
    libm calls of <= 2 ulp and about ten roundings of half an ulp on O(1) intermediates; if none of that averaged out over the sample the
    mean would be ~11 ulp off - 16 fp32 ulps (2^-23 each) of the largest value among the compared samples."""
    from mm_diffusion import ops
    diff = diffusion(predict_xstart, "learned")
    geom = GEOMS[stream]
    x0, xt, noise, mo, t = case_inputs(diff, geom, predict_xstart, True, seed=11)
    flags = diff._flags(False)
    got, tab = run_kernel(diff, x0, xt, noise, mo, t, geom, flags)
    _, vb = ops.loss_terms(mo.cuda(), noise.cuda(), tab, t.cuda(), *geom, flags, x0=x0.cuda(), xt=xt.cuda(), vb_scale=1.0)
    for gname, rows in (("t=0", t == 0), ("t>0", t != 0)):
        e = worst(vb.cpu()[rows], got[0][rows].double())
        print(f"{stream} x0-pred={predict_xstart} {gname}: loss_terms vb against vlb_terms vb {e:.3e}")
        assert e <= 16 * 2.0 ** -23


@pytest.mark.parametrize("var", ["large", "learned"])
@pytest.mark.parametrize("predict_xstart", [False, True])
@pytest.mark.parametrize("stream", ["video", "audio"])
def test_vlb_terms_backward_against_fp64_autograd(stream, predict_xstart, var):
    """d(sum dvb vb)/d model_out, mean and variance channels, the t = 0 (decoder NLL) and the t > 0 (KL) samples apart."""
    from mm_diffusion import ops
    diff = diffusion(predict_xstart, var)
    geom = GEOMS[stream]
    C = geom[1]
    flags = diff._flags(False)
    x0, xt, noise, mo, t = case_inputs(diff, geom, predict_xstart, var == "learned", seed=17)
    dvb = torch.linspace(0.5, 1.5, 16)
    tab, _ = diff.device_tables(torch.device("cuda"))
    g = torch.full_like(mo, float("nan"), device="cuda")
    ops.vlb_terms_bwd(x0.cuda(), xt.cuda(), mo.cuda(), tab, t.cuda(), *geom, flags, dvb.cuda(), g)
    torch.cuda.synchronize()
    g = g.cpu()
    refs = {}
    for dt in (torch.float64, torch.float32):
        leaf = mo.to(dt).requires_grad_()
        vb = terms_ref(x0, xt, noise, leaf, tab, t, flags, dt)[0]
        (vb * dvb.to(dt)).sum().backward()
        refs[dt] = leaf.grad
    assert torch.isfinite(g).all()
    fails = []
    groups = [("mean", slice(0, C))] + ([("variance", slice(C, 2 * C))] if var == "learned" else [])
    for cname, cs in groups:
        for tname, rows in (("t=0", t == 0), ("t>0", t != 0)):
            r64 = refs[torch.float64][rows][:, :, cs]
            e_k, e_y = rel_l2(g[rows][:, :, cs], r64), rel_l2(refs[torch.float32][rows][:, :, cs], r64)
            print(f"{stream} x0-pred={predict_xstart} var={var} {cname} {tname}: kernel {e_k:.3e}  fp32 autograd yardstick {e_y:.3e}")
            assert float(r64.norm()) > 0
            if not e_k <= 2 * e_y:
                fails.append((cname, tname, e_k, e_y))
    assert not fails, fails
    with pytest.raises(Exception, match="clip"):
        ops.vlb_terms_bwd(x0.cuda(), xt.cuda(), mo.cuda(), tab, t.cuda(), *geom, flags | 1, dvb.cuda(), torch.empty_like(mo, device="cuda"))


# ------------------------------------------------------------------ host methods against the reference's fixtures
# fp32 bounds: the loop bounds test_model_gpu.py (LOOP_TOL fp32 = 1e-4) and test_sr_gpu.py (5e-4) already apply.
# bf16 bounds: twice the rel-L2 measured against the fixture on the MI355X (the tables below; tests/golden/README_vlb.md), never above the
# bf16 bound of the sampling-loop test of the same model: tiny, 4 steps -> tiny_psample4 3e-2; tiny with learned sigma -> tiny_ls_psample2
# 1.2e-1 (test_model_gpu.py LOOP_TOL_BF16); SR -> 1e-1 (test_sr_gpu.py).  The outputs are bitwise repeatable: the factor is room for kernel
# changes, not for noise.  The prior term does not see the model: it keeps the fp32 bound in both modes.
# The largest entries are the pred_xstart tensors of the single-term call, whose second sample sits at the top timestep (t = 999 of the
# base process): the eps -> x0 map multiplies the model's bf16 error by sqrt(1 / abar_t - 1) ~ 157 before the clamp.
MM_FP32, SR_FP32 = 1e-4, 5e-4
MM_BF16_CAP = {"tiny_bpd": 3e-2, "tiny_ls_bpd": 1.2e-1}
SR_BF16_CAP = 1e-1
MM_BF16_MEASURED = {
    "tiny_bpd": {"total_bpd_video": 8.63e-05, "vb_video": 1.01e-04, "xstart_mse_video": 5.49e-04, "mse_video": 7.72e-04,
                 "total_bpd_audio": 1.48e-04, "vb_audio": 1.66e-04, "xstart_mse_audio": 2.02e-03, "mse_audio": 9.39e-04,
                 "term_output_video_clip1": 4.15e-04, "term_pred_xstart_video_clip1": 1.96e-02, "term_output_audio_clip1": 5.35e-04,
                 "term_pred_xstart_audio_clip1": 1.11e-02, "term_output_video_clip0": 2.21e-04, "term_pred_xstart_video_clip0": 7.15e-03,
                 "term_output_audio_clip0": 3.00e-04, "term_pred_xstart_audio_clip0": 5.60e-03},
    "tiny_ls_bpd": {"total_bpd_video": 2.02e-02, "vb_video": 2.02e-02, "xstart_mse_video": 9.19e-04, "mse_video": 5.12e-04,
                    "total_bpd_audio": 3.47e-03, "vb_audio": 3.50e-03, "xstart_mse_audio": 1.88e-03, "mse_audio": 2.07e-03,
                    "term_output_video_clip1": 3.15e-04, "term_pred_xstart_video_clip1": 5.50e-02, "term_output_audio_clip1": 3.02e-04,
                    "term_pred_xstart_audio_clip1": 2.52e-02, "term_output_video_clip0": 6.89e-04, "term_pred_xstart_video_clip0": 7.49e-03,
                    "term_output_audio_clip0": 2.62e-04, "term_pred_xstart_audio_clip0": 6.88e-03},
}
SR_BF16_MEASURED = {"total_bpd": 1.05e-02, "vb": 1.05e-02, "xstart_mse": 2.51e-04, "mse": 1.24e-04, "term_output": 9.62e-05,
                    "term_pred_xstart": 1.59e-02}
NAMES = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")


def _bound(measured, cap, fp32, key, dt):
    if dt == torch.float32 or "prior_bpd" in key:
        return fp32
    return min(2 * measured[key], cap)


def _mm(tag, dt):
    import test_model_gpu as tm
    ls = tag == "tiny_ls_bpd"
    g = gold(tag)
    fl, model, diff = tm.build("tiny", "tiny_learn_sigma" if ls else "tiny", dt, timestep_respacing="4", **(dict(learn_sigma=True) if ls else {}))
    assert diff.timestep_map == list(g["timestep_map"])
    x0 = {k: torch.from_numpy(g[f"x0_{k}"]).cuda() for k in ("video", "audio")}
    return tm, g, model, diff, x0


def _mm_loop(tm, g, model, diff, x0, **kw):
    tm.replay(model, g["shifts"])
    diff.noise_source = tm.cpu_noise_source()
    torch.manual_seed(int(g["seed"]))
    out = diff.calc_bpd_loop(model, x0, clip_denoised=True, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tag", ["tiny_bpd", "tiny_ls_bpd"])
def test_multimodal_bound_matches_the_reference_fixture(tag, dt):
    tm, g, model, diff, x0 = _mm(tag, dt)
    fails = []

    def check(name, got, want):
        e = rel_l2(got.float().cpu(), want)
        bound = _bound(MM_BF16_MEASURED[tag], MM_BF16_CAP[tag], MM_FP32, name, dt)
        print(f"{tag} {dt} {name}: rel-L2 {e:.3e} (bound {bound:.1e})")
        if not (np.isfinite(e) and e < bound):
            fails.append((name, e, bound))

    out = _mm_loop(tm, g, model, diff, x0)
    for k in ("video", "audio"):
        assert out["vb"][k].shape == g[f"vb_{k}"].shape
        for name in NAMES:
            check(f"{name}_{k}", out[name][k], g[f"{name}_{k}"])
        check(f"_prior_bpd_{k}", diff._prior_bpd(x0[k]), g[f"prior_bpd_{k}"])
    # one term at t = [0, k], clip on and off
    t = torch.from_numpy(g["term_t"]).cuda()
    xt = {k: torch.from_numpy(g[f"term_xt_{k}"]).cuda() for k in ("video", "audio")}
    for clip in (1, 0):
        tm.replay(model, g[f"term_shifts_clip{clip}"])
        with torch.no_grad():
            r = diff._vb_terms_bpd(model, x0, xt, t, clip_denoised=bool(clip))
        assert sorted(r) == ["output", "pred_xstart"]
        for k in ("video", "audio"):
            check(f"term_output_{k}_clip{clip}", r["output"][k], g[f"term_output_{k}_clip{clip}"])
            check(f"term_pred_xstart_{k}_clip{clip}", r["pred_xstart"][k], g[f"term_pred_xstart_{k}_clip{clip}"])
    assert not fails, fails


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_multimodal_bound_graph_replay_equals_eager_and_lanes_agree(dt):
    tm, g, model, diff, x0 = _mm("tiny_ls_bpd", dt)
    runs = {"graph": _mm_loop(tm, g, model, diff, x0), "eager": _mm_loop(tm, g, model, diff, x0, use_graph=False),
            "lanes1": _mm_loop(tm, g, model, diff, x0, lanes=1), "lanes2": _mm_loop(tm, g, model, diff, x0, lanes=2)}
    for other in ("eager", "lanes1", "lanes2"):
        for name in NAMES:
            for k in ("video", "audio"):
                assert torch.equal(runs["graph"][name][k], runs[other][name][k]), (other, name, k)


def _sr(dt, **over):
    import test_sr_gpu as ts
    g = gold("sr_tiny_bpd")
    model, diff = ts.build(dt, sr_timestep_respacing="4", **over)
    assert diff.timestep_map == list(g["timestep_map"])
    return g, model, diff, torch.from_numpy(g["x0"]).cuda(), torch.from_numpy(g["low"]).cuda()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_sr_bound_matches_the_reference_fixture(dt):
    g, model, diff, x0, low = _sr(dt)
    fails = []

    def check(name, got, want):
        e = rel_l2(got.float().cpu(), want)
        bound = _bound(SR_BF16_MEASURED, SR_BF16_CAP, SR_FP32, name, dt)
        print(f"sr_tiny_bpd {dt} {name}: rel-L2 {e:.3e} (bound {bound:.1e})")
        if not (np.isfinite(e) and e < bound):
            fails.append((name, e, bound))

    diff.noise_source = lambda like: torch.randn(like.shape).to(like.device)
    torch.manual_seed(int(g["seed"]))
    out = diff.calc_bpd_loop(model, x0, clip_denoised=True, model_kwargs={"low_res": low})
    assert sorted(out) == sorted(NAMES)
    for name in NAMES:
        assert tuple(out[name].shape) == g[name].shape
        check(name, out[name], g[name])
    check("_prior_bpd", diff._prior_bpd(x0), g["prior_bpd"])
    with torch.no_grad():
        r = diff._vb_terms_bpd(model, x0, torch.from_numpy(g["term_xt"]).cuda(), torch.from_numpy(g["term_t"]).cuda(), clip_denoised=True,
                               model_kwargs={"low_res": low})
    check("term_output", r["output"], g["term_output"])
    check("term_pred_xstart", r["pred_xstart"], g["term_pred_xstart"])
    assert not fails, fails


# ------------------------------------------------------------------ KL training (SR stage)
def test_sr_kl_training_matches_the_reference_fixture_and_accumulates():
    """use_kl=True (LossType.RESCALED_KL): the loss and EVERY parameter gradient against sr_tiny_kl_train_grads.npz with the comparison and
    the bounds of test_sr_train_gpu.py; a second backward accumulates into the same gradients."""
    import test_sr_train_gpu as srt
    g = gold("sr_tiny_kl_train_grads")
    for dt in (torch.float32, torch.bfloat16):
        d, model, diff = srt.sr_build("sr_tiny", dt, use_kl=True)
        x0, low, noise, t = srt.sr_inputs(g, d)
        terms = diff.training_losses(model, x0, t, model_kwargs={"low_res": low}, noise=noise)
        assert sorted(terms) == ["loss"] and terms["loss"].grad_fn is not None
        loss = terms["loss"].detach().float().cpu().numpy()
        terms["loss"].mean().backward()
        torch.cuda.synchronize()
        tol_loss, tol = (5e-4, srt.GRAD_FP32) if dt == torch.float32 else (3e-2, srt.GRAD_BF16)
        print(f"sr_tiny_kl {dt} loss: {loss} reference {g['loss']}")
        stride, names = int(g["stride"]), [str(n) for n in g["names"]]
        params = dict(model.named_parameters())
        assert names == list(params) and all(params[k].grad is not None for k in names)
        sub = torch.cat([params[k].grad.detach().float().flatten()[::stride] for k in names]).cpu()
        norms = np.asarray([float(params[k].grad.detach().double().norm()) for k in names])
        e_sub = rel_l2(sub, g["sub"])
        big = g["norms"] > srt.NORM_FLOOR * g["norms"].max()
        ratio = np.abs(norms / np.maximum(g["norms"], 1e-30) - 1)
        e_norm = float(ratio[big].max())
        wi = int(np.argmax(np.where(big, ratio, 0)))
        print(f"sr_tiny_kl gradients vs the reference ({dt}): subsample rel-L2 {e_sub:.3e}, worst per-tensor norm error {e_norm:.3e} ({names[wi]}); "
              f"{int(big.sum())} of {len(names)} tensors above the norm floor")
        assert big.mean() >= 0.9
        np.testing.assert_allclose(loss, g["loss"], rtol=tol_loss)
        assert torch.isfinite(sub).all() and e_sub < tol and e_norm < tol
        if dt == torch.float32:
            first = {k: params[k].grad.detach().clone() for k in names}
            diff.training_losses(model, x0, t, model_kwargs={"low_res": low}, noise=noise)["loss"].mean().backward()
            torch.cuda.synchronize()
            # (the tensors above the norm floor: below it a gradient is rounding residue of the atomics' order, different every call)
            e_acc = max(rel_l2(params[k].grad.cpu(), 2 * first[k].cpu()) for k, b in zip(names, big) if b)
            print(f"second backward: worst rel-L2 of grad against twice the first {e_acc:.3e}")
            assert e_acc < srt.GRAD_FP32
        del model
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ a bound that cannot be differentiated is never handed out as a loss
def test_bound_of_a_model_output_that_requires_grad_raises_unless_differentiable():
    """With autograd on and a model output that requires grad: the multimodal _vb_terms_bpd (no backward built) and the tensor-valued one
    with the clamp raise; the tensor-valued one with clip_denoised=False is the differentiable training form; under no_grad all evaluate."""
    from mm_diffusion._hip import MMDError
    from mm_diffusion import script_util as su
    g = torch.Generator().manual_seed(5)
    t = torch.tensor([1, 2]).cuda()
    mm = diffusion(False, "learned")
    x0 = {"video": torch.rand(2, 2, 3, 4, 4, generator=g).cuda(), "audio": torch.rand(2, 1, 32, generator=g).cuda()}
    outs = (torch.randn(2, 2, 6, 4, 4, generator=g).cuda().requires_grad_(), torch.randn(2, 2, 32, generator=g).cuda().requires_grad_())
    with pytest.raises(MMDError, match="no_grad"):
        mm._vb_terms_bpd(lambda v, a, ts: outs, x0, x0, t)
    with torch.no_grad():
        r = mm._vb_terms_bpd(lambda v, a, ts: outs, x0, x0, t)
    assert all(torch.isfinite(r["output"][k]).all() and not r["output"][k].requires_grad for k in ("video", "audio"))
    sr = su.create_gaussian_diffusion(diffusion_steps=1000, learn_sigma=True, timestep_respacing="4")
    img = torch.rand(2, 3, 8, 8, generator=g).cuda()
    mo = torch.randn(2, 6, 8, 8, generator=g).cuda().requires_grad_()
    with pytest.raises(NotImplementedError, match="no_grad"):
        sr._vb_terms_bpd(lambda x, ts: mo, img, img, t)
    live = sr._vb_terms_bpd(lambda x, ts: mo, img, img, t, clip_denoised=False)["output"]
    live.sum().backward()
    assert torch.isfinite(mo.grad).all() and float(mo.grad.abs().max()) > 0
    with torch.no_grad():
        held = sr._vb_terms_bpd(lambda x, ts: mo, img, img, t)["output"]
    assert torch.isfinite(held).all() and not held.requires_grad
