"""The graph-replayed stochastic multistep solver (SDE-DPM-Solver++) on the GPU.  Kernel level: mmd_dpmpp_sde_update bitwise against the
launches the eager method composes it from (mmd_clamp_scale, mmd_lincomb twice) and element by element against the float64 restatement
(tests/dpm_sde_ref.py has the bound), the counter form bitwise against mmd_ctr_fill(draw = k) + the memory form, rows against batch-1
calls, a k outside the table, refused overlaps, and the marginal a perfect data prediction must keep.  Loop level:
DPM_Solver.sample_graph_sde bitwise against sample(method="multistep_sde"), across launch modes and lane counts, CounterNoise
addressability, partial masks against the host composition, and the kept stepper."""
import random

import numpy as np
import pytest
import torch

import dpm_sde_ref as R
from helpers import rel_l2

pytestmark = pytest.mark.gpu

GUARD = 64


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _guarded(t, shift=0):
    """a device copy of t with GUARD sentinel floats on either side -> (whole buffer, view of t's shape); shift = 1 starts the view 4 bytes
    off a multiple of 16"""
    buf = torch.full((t.numel() + 2 * GUARD + shift,), -12345.0, device="cuda")
    buf[GUARD + shift:GUARD + shift + t.numel()] = t.reshape(-1)
    return buf, buf[GUARD + shift:GUARD + shift + t.numel()].view(t.shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == -12345.0).all()) and bool((buf[-GUARD:] == -12345.0).all())


_CASES = {}


def _case(cmf, with_s):
    """The device tensors of one kernel case (made once, never modified)."""
    if (cmf, with_s) not in _CASES:
        c = R.make_case(cmf, with_s)
        sh = (R.N, R.F, R.C, R.HW)
        d = dict(c, x_d=torch.from_numpy(c["x"]).cuda().view(sh), m1_d=torch.from_numpy(c["m1"]).cuda().view(sh), mo_d=torch.from_numpy(c["mo"]).cuda(),
                 tab_d=torch.from_numpy(c["tab"]).cuda(), cz_d=torch.from_numpy(c["cz"]).cuda(),
                 s_d=None if c["s"] is None else torch.from_numpy(c["s"]).cuda(), Cm=R.C * cmf)
        _CASES[(cmf, with_s)] = d
    return _CASES[(cmf, with_s)]


def _key_ids(seed=R.SEED, ids=R.IDS):
    key = torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32).view(np.int32)).cuda()
    return key, torch.tensor(list(ids), dtype=torch.int64, device="cuda")


def _k(k):
    return torch.tensor(list(k), dtype=torch.int64, device="cuda")


def _fill(k, tag, seed=R.SEED, ids=R.IDS):
    """mmd_ctr_fill(kind 0) per sample at draw k[n] -> fp32 [N, F, C, HW]"""
    from mm_diffusion import ops
    key, idt = _key_ids(seed, ids)
    out = torch.empty(len(ids), R.F, R.C, R.HW, device="cuda")
    for n, kn in enumerate(k):
        ops.ctr_fill(out[n:n + 1], 0, key, idt[n:n + 1].contiguous(), int(kn), tag)
    return out


def _composition(c, k, z):
    """What the eager method launches, sample by sample at row k[n]: clamp_scale + lincomb(x, c0, m0, c1[, M1, c2]) + lincomb(v, 1, z, cz)
    -> (x out, m0); a k outside the table leaves x."""
    from mm_diffusion import ops
    m0 = c["mo_d"][:, :, :R.C].clone().contiguous()          # a copy also where the slice is the whole tensor: clamp_scale_ works in place
    if c["s_d"] is not None:
        ops.clamp_scale_(m0, c["s_d"], c["max_val"])
    out = c["x_d"].clone()
    for n, kn in enumerate(k):
        if not 0 <= kn < R.ROWS:
            continue
        c0, c1, c2, kind = (float(c["tab"][j, kn]) for j in (2, 3, 4, 5))
        xn, mn, zn = (t[n:n + 1].contiguous() for t in (c["x_d"], m0, z))
        if int(kind) == R.DENOISE:
            out[n:n + 1] = mn
            continue
        v = ops.lincomb(xn, c0, mn, c1, c["m1_d"][n:n + 1].contiguous(), c2) if int(kind) == R.SECOND else ops.lincomb(xn, c0, mn, c1)
        out[n:n + 1] = ops.lincomb(v, 1.0, zn, float(c["cz"][kn]))
    return out, m0


# ----------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("cmf,with_s", R.CASES)
def test_memory_form_is_bitwise_the_composition_and_within_the_float64_bound(cmf, with_s):
    from mm_diffusion import ops
    c = _case(cmf, with_s)
    worst = 0.0
    for k in R.K_CASES:
        z = torch.from_numpy(R.counter_noise64(k, 0).astype(np.float32)).cuda().view(R.N, R.F, R.C, R.HW)
        want, m0 = _composition(c, k, z)
        (bx, x), (bm, m1), (bo, mov), (bz, zv) = _guarded(c["x_d"]), _guarded(c["m1_d"]), _guarded(c["mo_d"]), _guarded(z)
        ops.dpmpp_sde_update(x, mov, m1, c["tab_d"], c["cz_d"], _k(k), R.F, R.C, c["Cm"], R.HW, noise=zv, s=c["s_d"], max_val=c["max_val"])
        assert same(x, want), k
        assert same(m1, m0), "M1 must be the clamp-scaled m0"
        assert same(mov, c["mo_d"]) and same(zv, z) and all(_guards_intact(b) for b in (bx, bm, bo, bz))
        y, mw, by, bmw = R.update64(c["x"], c["m0raw"], c["m1"], z.cpu().numpy().reshape(R.N, R.PER), c["tab"], c["cz"], k, c["s"], c["max_val"])
        gx, gm = x.cpu().numpy().reshape(R.N, R.PER), m1.cpu().numpy().reshape(R.N, R.PER)
        worst = max(worst, float((np.abs(gx.astype(np.float64) - y) / np.maximum(by, 1e-300)).max()))
        assert R.violations(gx, y, by) == 0 and R.violations(gm, mw, bmw) == 0, k
    print(f"Cm {cmf}C s {with_s}: largest error / bound {worst:.3f}")
    # buffers that do not start on 16 bytes take the element path: the same bits
    for shift_x, shift_o in ((1, 0), (0, 1)):
        (bx, x), (bm, m1), (bo, mov), (bz, zv) = _guarded(c["x_d"], shift_x), _guarded(c["m1_d"], shift_x), _guarded(c["mo_d"], shift_o), _guarded(z, shift_x)
        ops.dpmpp_sde_update(x, mov, m1, c["tab_d"], c["cz_d"], _k(k), R.F, R.C, c["Cm"], R.HW, noise=zv, s=c["s_d"], max_val=c["max_val"])
        assert same(x, want) and same(m1, m0) and all(_guards_intact(b) for b in (bx, bm, bo, bz)), (shift_x, shift_o)
    # first-order and denoise rows do not read M1: NaN there must not reach x (0 * NaN would)
    for row in (0, 2):
        k = (row,) * R.N
        x, m1 = c["x_d"].clone(), torch.full_like(c["x_d"], float("nan"))
        ops.dpmpp_sde_update(x, c["mo_d"], m1, c["tab_d"], c["cz_d"], _k(k), R.F, R.C, c["Cm"], R.HW, noise=z, s=c["s_d"], max_val=c["max_val"])
        assert same(x, _composition(c, k, z)[0]), row


@pytest.mark.parametrize("cmf,with_s", R.CASES)
def test_counter_form_is_bitwise_fill_plus_memory_form(cmf, with_s):
    from mm_diffusion import ops
    c = _case(cmf, with_s)
    key, ids = _key_ids()
    geom = (R.F, R.C, c["Cm"], R.HW)
    for tag in (0, 1):
        for k in R.K_CASES:
            z = _fill(k, tag)
            xm, mm = c["x_d"].clone(), c["m1_d"].clone()
            ops.dpmpp_sde_update(xm, c["mo_d"], mm, c["tab_d"], c["cz_d"], _k(k), *geom, noise=z, s=c["s_d"], max_val=c["max_val"])
            (bx, x), (bm, m1) = _guarded(c["x_d"]), _guarded(c["m1_d"])
            ops.dpmpp_sde_update(x, c["mo_d"], m1, c["tab_d"], c["cz_d"], _k(k), *geom, ctr=(key, ids, tag), s=c["s_d"], max_val=c["max_val"])
            assert same(x, xm) and same(m1, mm), (tag, k)
            assert _guards_intact(bx) and _guards_intact(bm)
            if any(int(c["tab"][5, kn]) != R.DENOISE for kn in k):
                assert not same(x, _composition(c, k, torch.zeros_like(z))[0]), "the noise term is there"
        # the two streams draw different noise
        assert not same(_fill((0, 0, 0), 0), _fill((0, 0, 0), 1))
    # a row does not depend on the batch: sample id 7 alone is what it is as row 2 of 3
    assert R.IDS[2] == 7
    for k in ((1, 0, 3), (0, 0, 0)):
        x, m1 = c["x_d"].clone(), c["m1_d"].clone()
        ops.dpmpp_sde_update(x, c["mo_d"], m1, c["tab_d"], c["cz_d"], _k(k), *geom, ctr=(key, ids, 1), s=c["s_d"], max_val=c["max_val"])
        x1, m11 = c["x_d"][2:3].clone(), c["m1_d"][2:3].clone()
        ops.dpmpp_sde_update(x1, c["mo_d"][2:3].contiguous(), m11, c["tab_d"], c["cz_d"], _k(k[2:]), *geom, ctr=(key, ids[2:3].contiguous(), 1),
                             s=None if c["s_d"] is None else c["s_d"][2:3].contiguous(), max_val=c["max_val"])
        assert same(x1, x[2:3]) and same(m11, m1[2:3]), k


def test_a_step_number_outside_the_table_writes_nothing():
    from mm_diffusion import ops
    c = _case(2, True)
    key, ids = _key_ids()
    k = (4, 0, -2)
    z = _fill((0, 0, 0), 0)
    for src in (dict(noise=z), dict(ctr=(key, ids, 0))):
        (bx, x), (bm, m1) = _guarded(c["x_d"]), _guarded(c["m1_d"])
        ops.dpmpp_sde_update(x, c["mo_d"], m1, c["tab_d"], c["cz_d"], _k(k), R.F, R.C, c["Cm"], R.HW, s=c["s_d"], max_val=c["max_val"], **src)
        for n in (0, 2):
            assert same(x[n], c["x_d"][n]) and same(m1[n], c["m1_d"][n]), n
        assert not same(x[1], c["x_d"][1]) and not same(m1[1], c["m1_d"][1])
        assert _guards_intact(bx) and _guards_intact(bm)


def test_overlapping_arguments_are_refused_and_x_is_unwritten():
    from mm_diffusion import ops
    from mm_diffusion._hip import MMDError
    c = _case(1, False)
    key, ids = _key_ids()
    k = _k((0, 0, 0))
    geom = (R.F, R.C, c["Cm"], R.HW)
    big = torch.cat([c["x_d"].reshape(-1), c["m1_d"].reshape(-1)]).clone()
    x = big[:c["x_d"].numel()].view(c["x_d"].shape)
    inside = big[4:4 + c["x_d"].numel()].view(c["x_d"].shape)          # starts 16 bytes into x
    z = torch.zeros_like(c["x_d"])
    keep = big.clone()
    for m1, src in ((x, dict(noise=z)), (inside, dict(noise=z)), (c["m1_d"].clone(), dict(noise=x)), (c["m1_d"].clone(), dict(noise=inside)),
                    (x, dict(ctr=(key, ids, 0))), (inside, dict(ctr=(key, ids, 0)))):
        with pytest.raises(MMDError, match="overlap"):
            ops.dpmpp_sde_update(x, c["mo_d"], m1, c["tab_d"], c["cz_d"], k, *geom, **src)
        assert same(big, keep)
    zs = c["m1_d"].clone()
    with pytest.raises(MMDError, match="overlap"):
        ops.dpmpp_sde_update(x, c["mo_d"], zs, c["tab_d"], c["cz_d"], k, *geom, noise=zs)
    assert same(big, keep) and same(zs, c["m1_d"])


def test_a_perfect_data_prediction_keeps_the_marginal():
    """8 first-order rows of a logSNR grid through mmd_dpmpp_sde_update_ctr with m0 = mu at every row: element by element the float64
    emulation with the float64 Box-Muller normals within the carried bound (dpm_sde_ref.marginal_case), and the mean and variance of
    x - alpha_t mu within 5 standard errors of 0 and sigma_t^2 (the convention of test_seeded_gpu.py; tests/test_dpm_sde_cpu.py holds
    the float64 emulation to the same check for this seed)."""
    from mm_diffusion import ops
    m = R.marginal_case()
    sh = (R.M_N, R.F, R.C, R.HW)
    x = torch.from_numpy(m["x0"]).cuda().view(sh)
    mu = torch.from_numpy(m["mu"]).cuda().view(sh)
    m1 = torch.zeros_like(x)
    tab = torch.from_numpy(m["tab"]).cuda()
    cz = torch.from_numpy(m["cz"]).cuda()
    key, ids = _key_ids(R.M_SEED, R.M_IDS)
    for i in range(R.M_ROWS):
        ops.dpmpp_sde_update(x, mu, m1, tab, cz, torch.full((R.M_N,), i, dtype=torch.int64, device="cuda"), R.F, R.C, R.C, R.HW,
                             ctr=(key, ids, R.M_TAG))
    got = x.cpu().numpy().reshape(R.M_N, R.PER)
    err = np.abs(got.astype(np.float64) - m["want"])
    zm, zv = R.marginal_scores(got, m["mu"], m["alpha_t"], m["sigma_t"])
    print(f"largest error / carried bound {float((err / m['bound']).max()):.3f}; mean off by {zm:.2f} se, variance by {zv:.2f} se")
    assert R.violations(got, m["want"], m["bound"]) == 0
    assert zm <= 5.0 and zv <= 5.0
    assert same(m1, mu)


# ----------------------------------------------------------------------------- the loop
_MODELS = {}


def _model(dt):
    from test_model_gpu import build
    if dt not in _MODELS:
        _MODELS[dt] = build("tiny", "tiny", dt)
    return _MODELS[dt]


def _solver(dt=torch.float32, thresholding=True):
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    fl, model, diff = _model(dt)
    return fl, model, DPM_Solver(model=model, alphas_cumprod=torch.tensor(diff.alphas_cumprod, dtype=torch.float32), predict_x0=True,
                                 thresholding=thresholding)


def _replay(model, seed):
    rng = random.Random(seed)
    model.shift_source = lambda lo, hi: rng.randint(lo, hi)


def _x_T(fl, B, seed):
    torch.manual_seed(seed)
    return {"video": torch.randn(B, *fl["video_size"]).cuda(), "audio": torch.randn(B, *fl["audio_size"]).cuda()}


def _shape(fl, B):
    return {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}


def _clone(x):
    return {k: v.clone() for k, v in x.items()}


def _same_streams(a, b):
    return all(same(a[k], b[k]) for k in ("video", "audio"))


# (order, skip_type, thresholding, denoise, steps, dtype)
LOOPS = [
    (2, "logSNR", True, True, 6, torch.float32),
    (1, "time_uniform", False, False, 4, torch.float32),
    (2, "time_quadratic", False, True, 5, torch.float32),
    (1, "logSNR", True, True, 5, torch.float32),
    (2, "time_uniform", True, False, 4, torch.float32),
    (2, "logSNR", True, True, 5, torch.bfloat16),
]


@pytest.mark.parametrize("order,skip,thr,denoise,steps,dt", LOOPS)
def test_sample_graph_sde_is_bitwise_the_eager_method(order, skip, thr, denoise, steps, dt):
    fl, model, solver = _solver(dt, thr)
    try:
        x_T = _x_T(fl, 2, 11)
        kw = dict(steps=steps, order=order, skip_type=skip, denoise=denoise)
        _replay(model, 3)
        torch.manual_seed(77)
        want = solver.sample(_clone(x_T), method="multistep_sde", **kw)
        _replay(model, 3)
        torch.manual_seed(77)
        got = solver.sample_graph_sde(_clone(x_T), **kw)
        for k in ("video", "audio"):
            assert torch.isfinite(want[k]).all()
            assert same(got[k], want[k]), (k, rel_l2(got[k].cpu(), want[k].cpu()))
    finally:
        model.shift_source = None


def test_graph_and_eager_launch_and_lane_counts_agree_and_the_noise_is_used():
    fl, model, solver = _solver()
    x_T = _x_T(fl, 4, 5)
    kw = dict(steps=4, order=2, skip_type="logSNR", denoise=True)
    outs = []
    try:
        for use_graph, lanes in ((True, 1), (False, 1), (True, 2), (False, 2)):
            _replay(model, 9)
            torch.manual_seed(123)
            outs.append(solver.sample_graph_sde(_clone(x_T), use_graph=use_graph, lanes=lanes, **kw))
        _replay(model, 9)
        torch.manual_seed(124)
        other = solver.sample_graph_sde(_clone(x_T), use_graph=True, lanes=2, **kw)
        _replay(model, 9)
        det = solver.sample_graph(_clone(x_T), **kw)
    finally:
        model.shift_source = None
    for o in outs[1:]:
        assert _same_streams(o, outs[0])
    for k in ("video", "audio"):
        assert torch.isfinite(outs[0][k]).all()
        assert not same(other[k], outs[0][k]), "another torch seed gives another sample"
        assert not same(det[k], outs[0][k]), "the stochastic loop is not the deterministic one"


def test_counter_noise_samples_are_addressable():
    from mm_diffusion.seeded import CounterNoise, TAG_AUDIO, TAG_VIDEO, X_T
    fl, model, solver = _solver()
    assert model.shift_source is None
    kw = dict(steps=4, order=2, skip_type="logSNR", denoise=True)
    full = solver.sample_graph_sde(shape=_shape(fl, 4), noise_source=CounterNoise(1234), **kw)
    st = solver._stepper[1]
    assert st.noise is None, "with a counter there are no noise buffers"
    assert [name for _, _, name, *_ in st.update_plans[0]].count("mmd_dpmpp_sde_update_ctr") == 2
    torch.randn(1000, device="cuda")          # unrelated draws in between
    random.random()
    halves = [solver.sample_graph_sde(shape=_shape(fl, 2), noise_source=CounterNoise(1234, first_sample=f), **kw) for f in (0, 2)]
    for k in ("video", "audio"):
        assert torch.isfinite(full[k]).all()
        assert same(torch.cat([h[k] for h in halves]), full[k]), k
    for i in (1, 3):
        one = solver.sample_graph_sde(shape=_shape(fl, 1), noise_source=CounterNoise(1234, sample_ids=[i]), **kw)
        for k in ("video", "audio"):
            assert same(one[k][0], full[k][i]), (i, k)
    for use_graph, lanes in ((True, 1), (False, 2)):
        o = solver.sample_graph_sde(shape=_shape(fl, 4), noise_source=CounterNoise(1234), use_graph=use_graph, lanes=lanes, **kw)
        assert _same_streams(o, full), (use_graph, lanes)
    # the eager method on the counter's x_T draw
    ctr = CounterNoise(1234)
    sh = _shape(fl, 4)
    x_T = {"video": ctr.randn(sh["video"], TAG_VIDEO, X_T, "cuda"), "audio": ctr.randn(sh["audio"], TAG_AUDIO, X_T, "cuda")}
    eager = solver.sample(x_T, method="multistep_sde", noise_source=ctr, **kw)
    assert _same_streams(eager, full)
    assert model.shift_source is None
    other = solver.sample_graph_sde(shape=_shape(fl, 1), noise_source=CounterNoise(1235, sample_ids=[0]), **kw)
    assert not same(other["video"][0], full["video"][0]) and not same(other["audio"][0], full["audio"][0])
    with pytest.raises(Exception, match="x_T must be None"):
        solver.sample_graph_sde(_x_T(fl, 2, 1), noise_source=CounterNoise(1), **kw)


def _masks(fl, B, seed):
    g = torch.Generator().manual_seed(seed)
    F, C, Hh, Ww = fl["video_size"]
    L = fl["audio_size"][1]
    known = {"video": (torch.randn(B, F, C, Hh, Ww, generator=g) * 0.5).cuda(), "audio": (torch.randn(B, 1, L, generator=g) * 0.5).cuda()}
    mv = torch.rand(B, F, Hh, Ww, generator=g) < 0.4          # per-sample cells
    ma = torch.zeros(L, dtype=torch.bool)
    ma[:L // 3 + 1] = True                                       # one row for the batch
    return known, {"video": mv, "audio": ma}


@pytest.mark.parametrize("thr,order", [(True, 2), (False, 1)])
def test_partial_mask_is_the_host_composition(thr, order):
    from mm_diffusion import masking, ops
    fl, model, solver = _solver(torch.float32, thr)
    B, steps = 2, 4
    x_T = _x_T(fl, B, 21)
    known, mask = _masks(fl, B, 2)
    kw = dict(steps=steps, order=order, skip_type="logSNR", denoise=True)
    try:
        _replay(model, 4)
        torch.manual_seed(31)
        got = solver.sample_graph_sde(_clone(x_T), known=known, mask=mask, **kw)
        _replay(model, 4)
        torch.manual_seed(31)
        raw = solver.sample_graph_sde(_clone(x_T), known=known, mask=mask, paste_known=False, **kw)
        # the host composition: cond_replace before every evaluation + the eager update
        _replay(model, 4)
        torch.manual_seed(31)
        cond = masking.normalize(known, mask, {k: tuple(v.shape) for k, v in x_T.items()})
        tabs = solver.sde_tables(steps, order, "logSNR", True, device="cuda")
        qtab = torch.from_numpy(tabs["tab2"]).cuda()
        ts = tabs["timesteps"]
        grid = solver.get_time_steps("logSNR", solver.noise_schedule.T, 1. / solver.noise_schedule.total_N, steps, "cpu")

        def replace(x, i):
            x = _clone(x)
            for k, c in cond.items():
                ops.cond_replace(x[k], c.known, qtab, torch.full((B,), i, dtype=torch.int64, device="cuda"), mask=None if c.mask is None else c.mask.cuda(),
                                 noise=x_T[k])
            return x
        x, m1 = _clone(x_T), None
        with torch.no_grad():
            for i in range(steps):
                x = replace(x, i)
                m0 = solver.model_fn(x, ts[i].expand(B))
                second = order == 2 and i > 0
                coefs = solver._sde_coefs(grid[i - 1:i] if second else None, grid[i:i + 1], grid[i + 1:i + 2])
                z = {k: torch.randn(tuple(x[k].shape), device="cuda") for k in ("video", "audio")}
                x = solver.multistep_sde_update(x, m0, m1 if second else None, coefs, z)
                m1 = m0
            x = replace(x, steps)
            x = solver.denoise_fn(x, torch.ones((B,)) * (1. / solver.noise_schedule.total_N))
        for k in ("video", "audio"):
            assert torch.isfinite(raw[k]).all()
            assert same(raw[k], x[k]), (k, rel_l2(raw[k].cpu(), x[k].cpu()))
        for k, c in cond.items():
            ops.cond_replace(x[k], c.known, None, None, mask=None if c.mask is None else c.mask.cuda(), coef=(1.0, 0.0))
        for k in ("video", "audio"):
            assert same(got[k], x[k]), k
        # the known cells of the result are `known`, the others the raw result
        mv = mask["video"][:, :, None].expand(-1, -1, fl["video_size"][1], -1, -1).cuda()
        ma = mask["audio"][None, None].expand(B, 1, -1).cuda()
        for k, m in (("video", mv), ("audio", ma)):
            assert same(got[k][m], known[k][m]) and same(got[k][~m], raw[k][~m]) and not same(got[k][m], raw[k][m])
    finally:
        model.shift_source = None


def test_empty_mask_is_the_unconditional_loop():
    fl, model, solver = _solver()
    x_T = _x_T(fl, 2, 8)
    known, mask = _masks(fl, 2, 3)
    empty = {k: torch.zeros_like(m) for k, m in mask.items()}
    kw = dict(steps=4, order=2, skip_type="time_uniform", denoise=False)
    try:
        _replay(model, 6)
        torch.manual_seed(41)
        want = solver.sample_graph_sde(_clone(x_T), **kw)
        _replay(model, 6)
        torch.manual_seed(41)
        got = solver.sample_graph_sde(_clone(x_T), known=known, mask=empty, **kw)
    finally:
        model.shift_source = None
    assert _same_streams(got, want)


def test_kept_stepper_replays_on_another_grid_step_count_and_seed():
    from mm_diffusion.sampler import DpmppSdeStepper
    from mm_diffusion.seeded import CounterNoise
    fl, model, solver = _solver()
    calls = [(dict(steps=4, order=2, skip_type="time_uniform", denoise=True), 5), (dict(steps=6, order=1, skip_type="logSNR", denoise=False), 6)]
    got, kept, graphs = [], [], []
    for kw, seed in calls:
        got.append(solver.sample_graph_sde(shape=_shape(fl, 2), noise_source=CounterNoise(seed), **kw))
        kept.append(solver._stepper[1])
        graphs.append(list(kept[-1].graphs))
    assert isinstance(kept[0], DpmppSdeStepper) and kept[1] is kept[0], "the second call did not reuse the stepper"
    assert len(graphs[0]) == len(graphs[1]) and all(a is b for a, b in zip(graphs[0], graphs[1])), "the second call captured again"
    for (kw, seed), g in zip(calls, got):
        fresh = _solver()[2].sample_graph_sde(shape=_shape(fl, 2), noise_source=CounterNoise(seed), **kw)
        for k in ("video", "audio"):
            assert torch.isfinite(g[k]).all()
            assert same(g[k], fresh[k]), (kw, k, rel_l2(g[k].cpu(), fresh[k].cpu()))
    # the deterministic loop keeps a stepper of its own kind: the next call of the other kind builds one
    solver.sample_graph(shape=_shape(fl, 2), noise_source=CounterNoise(5), **calls[0][0])
    assert not isinstance(solver._stepper[1], DpmppSdeStepper)
