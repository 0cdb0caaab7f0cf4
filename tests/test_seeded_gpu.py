"""Seeded, addressable samples on the device: mmd_ctr_fill against the numpy restatement (words bitwise, normals element by element), the
fused update kernels against fill + memory kernel (bitwise), batch invariance at the kernel and at the loop level, and the moments."""
import random

import numpy as np
import pytest
import torch

import seeded_ref as R
from helpers import flags, synth_sd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
X_T = R.X_T

# |z - z64| <= K 2^-24 |z64|, element by element.  The ROCm installation the library is built with states no ulp figures for its device
# logf / sqrtf / sincospif (neither its headers nor its documents do), so K is not the 8 that 1 / 1 / 2 ulp would give through
#   z = sqrt(-2 ln u_a) cos(2 pi u_b):  (1 ulp of logf) / 2 + 1 ulp of sqrtf + 2 ulp of sincospif + 1/2 ulp of the product, 1 ulp <= 2 * 2^-24 relative
# but the measured fallback: the largest ratio seen on the first MI355X run over the 6 * 2^20 values below (4.098; per block 3.88 ... 4.10),
# doubled (DESIGN.md section 2 has both numbers).
K_MEASURED = 4.098
K = 2.0 * K_MEASURED


def _src(seed=42, **kw):
    from mm_diffusion.seeded import CounterNoise
    return CounterNoise(seed, **kw)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------- 1. words, bitwise
@pytest.mark.parametrize("ids", [[0], [7, 2 ** 32 - 1, 8], [9, 2, 5]])
def test_words_match_numpy_bitwise(ids):
    src = _src(0x0123456789ABCDEF, sample_ids=ids)
    seed = src.seed
    for per in (1, 3, 4, 5, 210, 1601, 6144):
        for draw in (0, 3, X_T):
            for tag in range(4):
                got = _u32(src.words((len(ids), per), tag, draw, DEV))
                want = np.stack([R.words(seed, sid, draw, tag, per) for sid in ids])
                assert np.array_equal(got, want), (per, draw, tag)


def test_ids_outside_32_bits_are_an_error():
    from mm_diffusion._hip import MMDError
    with pytest.raises(MMDError):
        _src(sample_ids=[2 ** 32]).words((1, 8), 0, 0, DEV)
    with pytest.raises(MMDError):
        _src(first_sample=2 ** 32 - 1).words((2, 8), 0, 0, DEV)
    with pytest.raises(MMDError):          # one id per row
        _src(sample_ids=[1, 2]).randn((3, 8), 0, 0, DEV)


# ----------------------------------------------------------------------------- 2. / 5. normals: element by element, and their moments
@pytest.fixture(scope="module")
def blocks():
    """{block: fp32 device normals as a float64 numpy array [2^20]} for R.BLOCKS + R.PARTNERS, drawn once."""
    out = {}
    for b in R.BLOCKS + R.PARTNERS:
        seed, sid, draw, tag = b
        out[b] = _src(seed, sample_ids=[sid]).randn((1, R.NBLOCK), tag, draw, DEV).cpu().numpy().reshape(-1)
    return out


def test_normals_match_float64_box_muller_element_by_element(blocks):
    worst = 0.0
    for b, z in blocks.items():
        assert z.dtype == np.float32
        z64 = R.normals(*b, R.NBLOCK)
        ratio = np.abs(z.astype(np.float64) - z64) / (2.0 ** -24 * np.abs(z64))
        worst = max(worst, float(ratio.max()))
        print(b, "largest |z - z64| / (2^-24 |z64|):", float(ratio.max()), "violations of K:", int((ratio > K).sum()))
    print("largest ratio over all blocks:", worst, "K:", K)
    for b, z in blocks.items():
        z64 = R.normals(*b, R.NBLOCK)
        assert int((np.abs(z.astype(np.float64) - z64) > K * 2.0 ** -24 * np.abs(z64)).sum()) == 0, b
    # a ragged sample: the words past its end are dropped, the values before it are those of the full quads
    for per in (1, 3, 5, 210, 1601):
        z = _src(42, sample_ids=[7]).randn((1, per), 1, 3, DEV).cpu().numpy().reshape(-1)
        assert np.array_equal(z, blocks[(42, 7, 3, 1)][:per])


def test_moments_on_device(blocks):
    n = R.NBLOCK
    for b in R.BLOCKS:
        z = blocks[b].astype(np.float64)
        print(b, "mean", z.mean(), "var", z.var())
        assert abs(z.mean()) <= 5.0 / np.sqrt(n)
        assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
        assert np.abs(z).max() <= 5.77
    for a, b in zip(R.BLOCKS, R.PARTNERS):          # other tag, id k + 1, draw i + 1
        c = float((blocks[a].astype(np.float64) * blocks[b].astype(np.float64)).mean())
        print(a, b, "corr", c)
        assert abs(c) <= 5.0 / np.sqrt(n)


# ----------------------------------------------------------------------------- 3. fused = fill + memory kernel
def _diffusion(learn_sigma, resp="8"):
    from mm_diffusion import multimodal_script_util as msu
    return msu.create_gaussian_diffusion(steps=1000, learn_sigma=learn_sigma, timestep_respacing=resp)


def _case(shape, learn_sigma, seed):
    N, F, C, HW = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, F, C, HW, generator=g).to(DEV)
    mo = (0.7 * torch.randn(N, F, 2 * C if learn_sigma else C, HW, generator=g)).to(DEV)
    return x, mo


IDS = [7, 2 ** 32 - 1, 8]
T_VEC = [0, 5, 2]


def _noise_rows(shape, tag, ids, t):
    """The memory form's noise: mmd_ctr_fill(kind 0) per sample at draw t[n]."""
    return torch.cat([_src(42, sample_ids=[sid]).randn((1,) + tuple(shape[1:]), tag, tn, DEV) for sid, tn in zip(ids, t)])


@pytest.mark.parametrize("shape,tag", [((3, 2, 3, 35), 0), ((3, 1, 1, 1601), 1)])
@pytest.mark.parametrize("learn_sigma", [False, True])
@pytest.mark.parametrize("clip", [False, True])
def test_fused_ddpm_update_is_fill_plus_memory_kernel(shape, tag, learn_sigma, clip):
    from mm_diffusion import ops
    diff = _diffusion(learn_sigma)
    tab, _ = diff.device_tables(DEV)
    N, F, C, HW = shape
    x, mo = _case(shape, learn_sigma, 3)
    t = torch.tensor(T_VEC, device=DEV)
    src = _src(42, sample_ids=IDS)
    noise = _noise_rows(shape, tag, IDS, T_VEC)
    fl = diff._flags(clip)
    assert bool(fl & 4) == learn_sigma
    a = [torch.full_like(x, 9.0) for _ in range(4)]
    b = [torch.full_like(x, 7.0) for _ in range(4)]
    ops.ddpm_update(x, mo, noise, a[0], tab, t, F, C, HW, fl, x0_out=a[1], mean_out=a[2], logvar_out=a[3])
    ops.ddpm_update_ctr(x, mo, src.key(DEV), src.ids(N, DEV), tag, b[0], tab, t, F, C, HW, fl, x0_out=b[1], mean_out=b[2], logvar_out=b[3])
    for name, u, v in zip(("sample", "x0", "mean", "logvar"), a, b):
        assert torch.equal(u, v), name
    assert torch.equal(a[0][0], a[2][0])                  # t == 0: no noise
    assert not torch.equal(a[0][1], a[2][1])              # t != 0: noise went in
    # the sample alone (the steppers' form), in place
    xin = x.clone()
    ops.ddpm_update_ctr(xin, mo, src.key(DEV), src.ids(N, DEV), tag, xin, tab, t, F, C, HW, fl)
    assert torch.equal(xin, a[0])


@pytest.mark.parametrize("shape,tag", [((3, 2, 3, 35), 0), ((3, 1, 1, 1601), 1)])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_fused_ddim_update_is_fill_plus_memory_kernel(shape, tag, eta):
    from mm_diffusion import ops
    for learn_sigma, clip in ((False, True), (True, False)):
        diff = _diffusion(learn_sigma)
        tab, _ = diff.device_tables(DEV)
        tab3 = diff.ddim_tables(DEV)
        N, F, C, HW = shape
        x, mo = _case(shape, learn_sigma, 4)
        t = torch.tensor(T_VEC, device=DEV)
        src = _src(42, sample_ids=IDS)
        noise = _noise_rows(shape, tag, IDS, T_VEC)
        fl = diff._flags(clip)
        a = [torch.full_like(x, 9.0) for _ in range(2)]
        b = [torch.full_like(x, 7.0) for _ in range(2)]
        ops.ddim_update(x, mo, noise, a[0], tab, tab3, t, F, C, HW, fl, eta, x0_out=a[1])
        ops.ddim_update_ctr(x, mo, src.key(DEV), src.ids(N, DEV), tag, b[0], tab, tab3, t, F, C, HW, fl, eta, x0_out=b[1])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (learn_sigma, clip)
        # the reverse ODE (flag 8) draws nothing
        ops.ddim_update(x, mo, None, a[0], tab, tab3, t, F, C, HW, fl | 8, 0.0)
        ops.ddim_update_ctr(x, mo, src.key(DEV), src.ids(N, DEV), tag, b[0], tab, tab3, t, F, C, HW, fl | 8, 0.0)
        assert torch.equal(a[0], b[0])


# ----------------------------------------------------------------------------- 4. kernel-level batch invariance
def test_kernel_rows_do_not_depend_on_the_batch():
    from mm_diffusion import ops
    diff = _diffusion(False)
    tab, _ = diff.device_tables(DEV)
    shape = (4, 2, 3, 35)
    N, F, C, HW = shape
    x, mo = _case(shape, False, 5)
    ids = [7, 8, 9, 10]
    t = torch.tensor([3] * N, device=DEV)

    def run(rows):
        src = _src(42, sample_ids=[ids[r] for r in rows])
        out = torch.empty(len(rows), F, C, HW, device=DEV)
        ops.ddpm_update_ctr(x[rows].contiguous(), mo[rows].contiguous(), src.key(DEV), src.ids(len(rows), DEV), 0, out, tab, t[:len(rows)].contiguous(),
                            F, C, HW, 1)
        fill = src.randn((len(rows), F, C, HW), 0, 3, DEV)
        return out, fill
    whole, wfill = run([0, 1, 2, 3])
    assert len({whole[r].cpu().numpy().tobytes() for r in range(4)}) == 4
    for r in range(4):
        one, ofill = run([r])
        assert torch.equal(one[0], whole[r]) and torch.equal(ofill[0], wfill[r]), r
    perm = [2, 0, 3, 1]
    p, pfill = run(perm)
    for k, r in enumerate(perm):
        assert torch.equal(p[k], whole[r]) and torch.equal(pfill[k], wfill[r]), r
    # first_sample addresses the same ids
    assert torch.equal(_src(42, first_sample=7).randn((4, F, C, HW), 0, 3, DEV), wfill)


# ----------------------------------------------------------------------------- 6. end to end, tiny model
_MODELS = {}


def _model(dt):
    if dt not in _MODELS:
        from mm_diffusion import logger, multimodal_script_util as msu
        logger.set_quiet(True)
        fl = flags("tiny", timestep_respacing="4", use_fp16=(dt == torch.bfloat16))
        model, diff = msu.create_model_and_diffusion(**fl)
        model.load_state_dict(synth_sd("tiny"))
        model.cuda().eval()
        assert diff.noise_source is None
        g = torch.Generator().manual_seed(11)
        cond = (0.5 * torch.randn(4, *fl["video_size"], generator=g)).to(DEV)
        _MODELS[dt] = fl, model, diff, cond
    return _MODELS[dt]


def _loop(dt, kind, B, first, seed=42, use_graph=True):
    """Rows first ... first + B - 1 of seed `seed` through one sampling loop -> [B, video + audio values]."""
    fl, model, diff, cond = _model(dt)
    diff.noise_source = _src(seed, first_sample=first)
    shape = {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}
    try:
        if kind == "ddpm" and use_graph:
            final = diff.p_sample_loop(model, shape, device=DEV, progress=False)
        elif kind == "ddim" and use_graph:
            final = diff.ddim_sample_loop(model, shape, device=DEV, progress=False, eta=0.5)
        else:
            if kind == "ddpm":
                gen = diff.p_sample_loop_progressive(model, shape, device=DEV, use_graph=use_graph)
            elif kind == "ddim":
                gen = diff.ddim_sample_loop_progressive(model, shape, device=DEV, eta=0.5, use_graph=use_graph)
            else:
                gen = diff.conditional_p_sample_loop_progressive_unscale(model, shape, False, model_kwargs={"video": cond[first:first + B].clone()},
                                                                         device=DEV, use_graph=use_graph)
            for final in gen:
                pass
    finally:
        diff.noise_source = None
    torch.cuda.synchronize()
    return torch.cat([final["video"].float().flatten(1), final["audio"].float().flatten(1)], dim=1).clone()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "replace"])
def test_sample_k_is_the_same_in_any_batch_lane_count_and_path(dt, kind, monkeypatch):
    from mm_diffusion.sampler import default_lanes
    monkeypatch.delenv("MMD_LANES", raising=False)
    assert default_lanes(4) == 2
    ref = _loop(dt, kind, 4, 0)
    assert torch.isfinite(ref).all()
    assert len({ref[r].cpu().numpy().tobytes() for r in range(4)}) == 4          # sample 3 differs from sample 2, and so on
    assert torch.equal(torch.cat([_loop(dt, kind, 2, 0), _loop(dt, kind, 2, 2)]), ref), "batch 2 + batch 2"
    assert torch.equal(torch.cat([_loop(dt, kind, 1, k) for k in range(4)]), ref), "four batch-1 runs"
    assert torch.equal(_loop(dt, kind, 4, 0, use_graph=False), ref), "eager launches"
    monkeypatch.setenv("MMD_LANES", "1")
    assert default_lanes(4) == 1
    assert torch.equal(_loop(dt, kind, 4, 0), ref), "one lane"
    monkeypatch.delenv("MMD_LANES")
    torch.randn(1000)
    torch.randn(1000, device=DEV)
    random.seed(99)
    [random.randint(0, 7) for _ in range(17)]
    assert torch.equal(_loop(dt, kind, 4, 0), ref), "after unrelated draws"
    other = _loop(dt, kind, 1, 2, seed=43)
    assert not torch.equal(other[0], ref[2]), "another seed"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fn", ["p_sample_loop", "ddim_sample_loop"])
def test_sr_sample_k_is_the_same_in_any_batch(dt, fn):
    from test_sr_gpu import build
    model, diff = build(dt, sr_timestep_respacing="3")
    assert diff.noise_source is None
    g = torch.Generator().manual_seed(13)
    low = (0.5 * torch.randn(4, 3, 16, 16, generator=g)).to(DEV)

    def run(B, first, seed=42):
        diff.noise_source = _src(seed, first_sample=first)
        kw = dict(eta=0.5) if fn == "ddim_sample_loop" else {}
        out = getattr(diff, fn)(model, (B, 3, 64, 64), clip_denoised=True, model_kwargs={"low_res": low[first:first + B].clone()}, noise=None,
                                device=DEV, progress=False, **kw)
        diff.noise_source = None
        return out.float().clone()
    ref = run(4, 0)
    assert torch.isfinite(ref).all() and len({ref[r].cpu().numpy().tobytes() for r in range(4)}) == 4
    assert torch.equal(torch.cat([run(2, 0), run(2, 2)]), ref), "batch 2 + batch 2"
    assert torch.equal(torch.cat([run(1, k) for k in range(4)]), ref), "four batch-1 runs"
    torch.randn(1000)
    torch.randn(1000, device=DEV)
    assert torch.equal(run(4, 0), ref), "after unrelated draws"
    assert not torch.equal(run(1, 2, seed=43)[0], ref[2]), "another seed"


def test_sr_loop_with_a_noise_tensor_keeps_the_reference_behaviour():
    """noise= handed in: that tensor is x_T and the per-step noise of every step (memory kernel), whatever the noise source is."""
    from test_sr_gpu import build
    model, diff = build(torch.float32, sr_timestep_respacing="3")
    g = torch.Generator().manual_seed(14)
    low, noise = (0.5 * torch.randn(2, 3, 16, 16, generator=g)).to(DEV), torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    outs = []
    for src in (None, _src(42)):
        diff.noise_source = src
        outs.append(diff.p_sample_loop(model, (2, 3, 64, 64), model_kwargs={"low_res": low}, noise=noise.clone(), device=DEV, progress=False))
    assert torch.equal(outs[0], outs[1])


# ----------------------------------------------------------------------------- 7. nothing moved
def test_stepper_without_a_counter_source_is_unchanged():
    from mm_diffusion.sampler import GraphStepper
    fl, model, diff, _ = _model(torch.float32)
    names = lambda st: [op[2] for plan in st.update_plans for op in plan if op[0] is not None]      # noqa: E731
    for update, mem, ctr in (("ddpm", "mmd_ddpm_update", "mmd_ddpm_update_ctr"), ("ddim", "mmd_ddim_update", "mmd_ddim_update_ctr")):
        assert diff.noise_source is None
        st = GraphStepper(diff, model, 2, DEV, update=update, eta=0.5)
        assert st.noise_v.shape == (2, *fl["video_size"]) and st.noise_a.shape == (2, *fl["audio_size"])
        assert names(st) == [mem, mem]
        st.close()
        diff.noise_source = _src(42)
        try:
            st = GraphStepper(diff, model, 2, DEV, update=update, eta=0.5)
            assert st.noise_v is None and st.noise_a is None and names(st) == [ctr, ctr]
            st.close()
            st = GraphStepper(diff, model, 2, DEV, update="vlb")          # out of scope: its noise stays in memory
            assert st.noise_v is not None and "mmd_vlb_terms" in names(st)
            st.close()
        finally:
            diff.noise_source = None


def test_steps_need_uniform_timesteps_with_a_counter_source():
    from mm_diffusion._hip import MMDError
    fl, model, diff, _ = _model(torch.float32)
    x = {"video": torch.zeros(2, *fl["video_size"], device=DEV), "audio": torch.zeros(2, *fl["audio_size"], device=DEV)}
    diff.noise_source = _src(42)
    try:
        for step in (diff.p_sample, diff.ddim_sample):
            with pytest.raises(MMDError):
                with torch.no_grad():
                    step(model, x, torch.tensor([3, 2], device=DEV))
    finally:
        diff.noise_source = None
