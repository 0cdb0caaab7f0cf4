"""The graph-replayed single-step DPM-Solver / DPM-Solver++ loop on the GPU: mmd_dpm_single_update bitwise against the launches it
replaces (mmd_lincomb, mmd_dpmpp_x0, mmd_clamp_scale), and DPM_Solver.sample_graph_singlestep bitwise against
sample(method="singlestep" / "singlestep_fixed").

Bounds.  Everything compared with the eager kernels is compared bit for bit.  The float64 check of a stage row allows three fp32
roundings (the product c0 XB and the two fmas), each relative to a partial sum that is no larger than |c0 XB| + |c1 MS| + |c2 m0|:
3 * 2^-24 of that total, on every element.  The loops against the reference fixtures keep the rel-L2 of 1e-4 that
test_dpm_solver_gpu.py applies to the eager loop on the same fixtures."""
import random

import numpy as np
import pytest
import torch

from helpers import gold, rel_l2

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- the kernel
GUARD = 64


def _guarded(t):
    """a copy of t with GUARD sentinel floats on either side -> (whole buffer, view of t's shape)"""
    buf = torch.full((t.numel() + 2 * GUARD,), -12345.0, device="cuda")
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    return buf, buf[GUARD:GUARD + t.numel()].view(t.shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == -12345.0).all()) and bool((buf[-GUARD:] == -12345.0).all())


# N, F, C, HW: one ragged block / many blocks with a sample boundary inside a block and a ragged tail
SHAPES = [(3, 2, 3, 5), (2, 1, 1, 70001)]
ROWS = 3      # row j has kind j


def _case(shape, Cm_factor, seed=0):
    N, F, C, HW = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, F, C, HW, generator=g).cuda()
    xb = torch.randn(N, F, C, HW, generator=g).cuda()
    ms = torch.randn(N, F, C, HW, generator=g).cuda()
    src = (torch.randn(N, F, C * Cm_factor, HW, generator=g) * 1.5).cuda()
    src[:, :, C:] = float("nan")          # the variance channels of a learned-sigma output are never read
    tab = torch.zeros(6, ROWS)
    tab[0], tab[1] = torch.tensor([1.7, 157.41, 1.0002]), torch.tensor([-1.3, -157.40, -0.017])
    tab[2], tab[3], tab[4] = torch.tensor([0.99, 2.6, 5.0]), torch.tensor([0.01, -2.4, 5.0]), torch.tensor([7.0, 0.81, 5.0])
    tab[5] = torch.tensor([0.0, 1.0, 2.0])
    return x, xb, ms, src, tab.cuda()


def _want(row, tab, x0, xb0, ms0, m0):
    """(x, XB, MS) after a row of kind `row`, from the eager loop's launches."""
    from mm_diffusion import ops
    c0, c1, c2 = (float(tab[j, row]) for j in (2, 3, 4))
    if row == 0:
        return ops.lincomb(x0, c0, m0, c1), x0, m0
    if row == 1:
        return ops.lincomb(xb0, c0, ms0, c1, m0, c2), xb0, ms0
    return m0, xb0, ms0


def _run(shape, Cm, tab, k, x0, xb0, ms0, src, **kw):
    """One guarded call: the buffers after it, all guards and the source checked."""
    from mm_diffusion import ops
    N, F, C, HW = shape
    (bx, x), (bb, xb), (bm, ms), (bs, sv) = _guarded(x0), _guarded(xb0), _guarded(ms0), _guarded(src)
    ops.dpm_single_update(x, sv, xb, ms, tab, k, F, C, Cm, HW, **kw)
    assert same(sv, src) and all(_guards_intact(b) for b in (bx, bb, bm, bs))
    return x.clone(), xb.clone(), ms.clone()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("Cm_factor", [1, 2])
def test_update_is_bitwise_the_launches_it_replaces(shape, Cm_factor):
    from mm_diffusion import ops
    N, F, C, HW = shape
    x0, xb0, ms0, src, tab = _case(shape, Cm_factor)
    eps = src[:, :, :C].contiguous()
    s = torch.tensor([0.4, 1.3, 2.9][:N], device="cuda")
    max_val = 1.5
    clamped = ops.clamp_scale_(eps.clone(), s, max_val)
    for row in range(ROWS):
        k = torch.full((N,), row, dtype=torch.int64, device="cuda")
        # form 0: m0 is the first C channels of the source
        got = _run(shape, C * Cm_factor, tab, k, x0, xb0, ms0, src)
        for g, w, what in zip(got, _want(row, tab, x0, xb0, ms0, eps), ("x", "XB", "MS")):
            assert same(g, w), (row, what)
        assert all(same(a, b) for a, b in zip(got, _run(shape, C * Cm_factor, tab, k, x0, xb0, ms0, src))), "two calls, two results"
        # form 1: the data prediction formed in the kernel = mmd_dpmpp_x0 followed by form 0
        x0raw = ops.dpmpp_x0(x0, src, torch.empty_like(x0), tab, k, F, C, C * Cm_factor, HW)
        assert same(x0raw, ops.lincomb(x0, float(tab[0, row]), eps, float(tab[1, row])))
        got = _run(shape, C * Cm_factor, tab, k, x0, xb0, ms0, src, form=1)
        two = _run(shape, C, tab, k, x0, xb0, ms0, x0raw)
        for g, t, w, what in zip(got, two, _want(row, tab, x0, xb0, ms0, x0raw), ("x", "XB", "MS")):
            assert same(g, t) and same(g, w), (row, what, "form 1")
        # s: the clamp of mmd_clamp_scale in front of the plain form; MS holds the clamped value
        got = _run(shape, C * Cm_factor, tab, k, x0, xb0, ms0, src, s=s, max_val=max_val)
        plain = _run(shape, C, tab, k, x0, xb0, ms0, clamped)
        for g, t, w, what in zip(got, plain, _want(row, tab, x0, xb0, ms0, clamped), ("x", "XB", "MS")):
            assert same(g, t) and same(g, w), (row, what, "s")
    # step numbers outside the table leave x, XB and MS alone; the sample next to them is written (N = 2: the boundary is inside a block)
    for ks in ([-2, 0, ROWS][:N], [ROWS, -2, 1][:N], [0, ROWS, -2][:N]):
        k = torch.tensor(ks, dtype=torch.int64, device="cuda")
        got = _run(shape, C * Cm_factor, tab, k, x0, xb0, ms0, src)
        for n, kn in enumerate(ks):
            if 0 <= kn < ROWS:
                for g, w in zip(got, _want(kn, tab, x0, xb0, ms0, eps)):
                    assert same(g[n], w[n]), (ks, n)
                assert not same(got[0][n], x0[n])
            else:
                assert same(got[0][n], x0[n]) and same(got[1][n], xb0[n]) and same(got[2][n], ms0[n]), (ks, n)


def test_stage_row_is_within_three_roundings_of_float64():
    shape = (2, 2, 3, 4099)
    N, F, C, HW = shape
    x0, xb0, ms0, src, tab = _case(shape, 1, seed=4)
    k = torch.ones(N, dtype=torch.int64, device="cuda")
    got = _run(shape, C, tab, k, x0, xb0, ms0, src)[0].double().cpu()
    c0, c1, c2 = (float(tab[j, 1]) for j in (2, 3, 4))          # the fp32 table values, exactly
    terms = [c0 * xb0.double().cpu(), c1 * ms0.double().cpu(), c2 * src.double().cpu()]
    want, scale = terms[0] + terms[1] + terms[2], terms[0].abs() + terms[1].abs() + terms[2].abs()
    excess = ((got - want).abs() - 3 * 2.0 ** -24 * scale).max()
    print(f"worst |got - want| / scale = {((got - want).abs() / scale).max():.3e} (bound {3 * 2.0 ** -24:.3e})")
    assert float(excess) <= 0.0


# ----------------------------------------------------------------------------- the loop
_MODELS = {}


def _model(dt):
    from test_model_gpu import build
    if dt not in _MODELS:
        _MODELS[dt] = build("tiny", "tiny", dt)
    return _MODELS[dt]


def _solver(dt, predict_x0, thresholding):
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    fl, model, diff = _model(dt)
    return fl, model, DPM_Solver(model=model, alphas_cumprod=torch.tensor(diff.alphas_cumprod, dtype=torch.float32), predict_x0=predict_x0,
                                 thresholding=thresholding)


def _replay(model, seed):
    rng = random.Random(seed)
    model.shift_source = lambda lo, hi: rng.randint(lo, hi)


def _x_T(fl, B, seed):
    torch.manual_seed(seed)
    return {"video": torch.randn(B, *fl["video_size"]).cuda(), "audio": torch.randn(B, *fl["audio_size"]).cuda()}


def _clone(x):
    return {k: v.clone() for k, v in x.items()}


# (order, method, steps, skip_type, predict_x0, thresholding, denoise, solver_type, dtype)
LOOPS = [
    (3, "singlestep", 4, "logSNR", False, False, False, "dpm_solver", torch.float32),
    (3, "singlestep", 5, "logSNR", True, True, True, "dpm_solver", torch.float32),
    (3, "singlestep", 6, "time_uniform", True, False, True, "dpm_solver", torch.float32),
    (2, "singlestep", 3, "time_quadratic", False, False, True, "dpm_solver", torch.float32),
    (2, "singlestep", 4, "logSNR", True, True, False, "taylor", torch.float32),
    (2, "singlestep", 4, "time_uniform", False, True, True, "taylor", torch.float32),
    (1, "singlestep", 2, "logSNR", False, False, False, "dpm_solver", torch.float32),
    (3, "singlestep_fixed", 7, "logSNR", True, False, False, "dpm_solver", torch.float32),
    (3, "singlestep", 5, "logSNR", False, False, True, "dpm_solver", torch.bfloat16),
    (3, "singlestep", 4, "logSNR", True, True, True, "dpm_solver", torch.bfloat16),
]


@pytest.mark.parametrize("order,method,steps,skip,px,thr,denoise,st,dt", LOOPS)
def test_sample_graph_singlestep_is_bitwise_the_eager_loop(order, method, steps, skip, px, thr, denoise, st, dt):
    """sample() runs under torch.no_grad() here, as a sampling script runs it: its closing denoise evaluation is the one call it makes
    outside its own no_grad block (test_dpmpp_gpu.py has the measurement)."""
    fl, model, solver = _solver(dt, px, thr)
    try:
        x_T = _x_T(fl, 2, 11)
        kw = dict(steps=steps, order=order, skip_type=skip, method=method, denoise=denoise, solver_type=st)
        rows = solver.singlestep_tables(**kw)["rows"]
        _replay(model, 3)
        with torch.no_grad():
            want = solver.sample(_clone(x_T), **kw)
        nfe_eager, solver.nfe = solver.nfe, 0
        _replay(model, 3)
        got = solver.sample_graph_singlestep(_clone(x_T), **kw)
        assert solver.nfe == rows == nfe_eager, (solver.nfe, rows, nfe_eager)
        for k in ("video", "audio"):
            assert torch.isfinite(want[k]).all()
            assert same(got[k], want[k]), (k, rel_l2(got[k].cpu(), want[k].cpu()))
    finally:
        model.shift_source = None


@pytest.mark.parametrize("tag,kw", [
    ("tiny_dpm_singlestep3", dict(steps=20, order=3, skip_type="logSNR", method="singlestep")),
    ("tiny_dpm_singlestep2", dict(steps=7, order=2, skip_type="time_quadratic", method="singlestep")),
])
def test_sample_graph_singlestep_matches_the_reference_fixtures(tag, kw):
    g = gold(tag)
    fl, model, solver = _solver(torch.float32, False, False)
    it = iter(int(s) for s in g["shifts"])
    model.shift_source = lambda lo, hi: next(it)
    try:
        B = int(g["B"])
        torch.manual_seed(int(g["seed"]))
        x_T = {"video": torch.randn(B, *fl["video_size"]).cuda(), "audio": torch.randn(B, *fl["audio_size"]).cuda()}
        out = solver.sample_graph_singlestep(x_T, **kw)
    finally:
        model.shift_source = None
    ev, ea = rel_l2(out["video"].cpu(), g["video"]), rel_l2(out["audio"].cpu(), g["audio"])
    print(f"{tag}: rel-L2 video {ev:.3e} audio {ea:.3e}")
    assert next(it, None) is None, "different number of network evaluations than the reference"
    assert ev < 1e-4 and ea < 1e-4


def test_graph_and_eager_launch_and_lane_counts_agree():
    fl, model, solver = _solver(torch.float32, True, True)
    x_T = _x_T(fl, 4, 5)
    kw = dict(steps=5, order=3, skip_type="logSNR", denoise=True)
    outs = []
    try:
        for use_graph, lanes in ((True, 1), (False, 1), (True, 2), (False, 2)):
            _replay(model, 9)
            outs.append(solver.sample_graph_singlestep(_clone(x_T), use_graph=use_graph, lanes=lanes, **kw))
        # with thresholding: mmd_dpmpp_x0 + the selection + the update per stream, then the join
        per_stream = ["mmd_dpmpp_x0", "mmd_dpmpp_select", "mmd_dpm_single_update"]
        assert [name for _, _, name, *_ in solver._stepper[1].update_plans[0]] == per_stream * 2 + ["sync"]
    finally:
        model.shift_source = None
    for o in outs[1:]:
        assert same(o["video"], outs[0]["video"]) and same(o["audio"], outs[0]["audio"])


def test_kept_stepper_replays_both_plan_sets_on_another_grid():
    """The noise-prediction solver with denoise=True launches two plan sets, the step and the closing data prediction ("final").  A second
    call with another grid, order and step count reuses the kept stepper - both sets' captured graphs against reloaded tables - and
    gives the bits of a fresh solver and of the eager loop; a sample_graph call in between (another kind of stepper) breaks neither."""
    from mm_diffusion.sampler import DpmppStepper, DpmSingleStepper
    fl, model, solver = _solver(torch.float32, False, False)
    x_T = _x_T(fl, 2, 7)
    calls = [dict(steps=4, order=3, skip_type="logSNR", denoise=True), dict(steps=5, order=2, skip_type="time_uniform", denoise=True)]
    multi = dict(steps=3, order=2, skip_type="logSNR", denoise=True)

    def run(fn, kw, **more):
        _replay(model, 13)
        with torch.no_grad():
            return fn(_clone(x_T), **kw, **more)

    def check(kw, g, eager_method, fresh_fn):
        fresh = run(getattr(_solver(torch.float32, False, False)[2], fresh_fn), kw)
        eager = run(solver.sample, kw, method=eager_method)
        for k in ("video", "audio"):
            assert torch.isfinite(g[k]).all()
            assert same(g[k], fresh[k]), (kw, k, "fresh solver", rel_l2(g[k].cpu(), fresh[k].cpu()))
            assert same(g[k], eager[k]), (kw, k, "eager loop", rel_l2(g[k].cpu(), eager[k].cpu()))
    try:
        got, kept = [], []
        for kw in calls:
            got.append(run(solver.sample_graph_singlestep, kw))
            kept.append(solver._stepper[1])
        assert kept[1] is kept[0] and isinstance(kept[0], DpmSingleStepper) and kept[0].final_plans
        assert all(ps.graphs is not None for ps in kept[0]._sets.values()), "both plan sets are captured"
        # without thresholding a stream's update is ONE launch in either solver form: per set two launches and the join
        assert [name for _, _, name, *_ in kept[0].update_plans[0]] == ["mmd_dpm_single_update"] * 2 + ["sync"]
        assert [name for _, _, name, *_ in kept[0].final_plans[0]] == ["mmd_dpm_single_update"] * 2 + ["sync"]
        for kw, g in zip(calls, got):
            check(kw, g, "singlestep", "sample_graph_singlestep")
        between = run(solver.sample_graph, multi)
        assert isinstance(solver._stepper[1], DpmppStepper)
        check(multi, between, "multistep", "sample_graph")
        after = run(solver.sample_graph_singlestep, calls[0])
        assert isinstance(solver._stepper[1], DpmSingleStepper) and solver._stepper[1] is not kept[0]
        for k in ("video", "audio"):
            assert same(after[k], got[0][k]), k
    finally:
        model.shift_source = None


def test_counter_noise_samples_are_addressable():
    """The reference script's call (noise prediction, order 3, logSNR, singlestep) at steps = 5."""
    from mm_diffusion.seeded import CounterNoise
    fl, model, solver = _solver(torch.float32, False, False)
    assert model.shift_source is None
    shape = lambda B: {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}      # noqa: E731
    kw = dict(steps=5)
    full = solver.sample_graph_singlestep(shape=shape(4), noise_source=CounterNoise(1234), **kw)
    halves = [solver.sample_graph_singlestep(shape=shape(2), noise_source=CounterNoise(1234, first_sample=f), **kw) for f in (0, 2)]
    for k in ("video", "audio"):
        assert torch.isfinite(full[k]).all()
        assert same(torch.cat([h[k] for h in halves]), full[k]), k
    for i in range(4):      # batch 1 is accepted
        one = solver.sample_graph_singlestep(shape=shape(1), noise_source=CounterNoise(1234, sample_ids=[i]), **kw)
        for k in ("video", "audio"):
            assert same(one[k][0], full[k][i]), (i, k)
    other = solver.sample_graph_singlestep(shape=shape(1), noise_source=CounterNoise(1235, sample_ids=[0]), **kw)
    assert not same(other["video"][0], full["video"][0])


def _masks(fl, B, seed):
    g = torch.Generator().manual_seed(seed)
    F, C, Hh, Ww = fl["video_size"]
    L = fl["audio_size"][1]
    known = {"video": (torch.randn(B, F, C, Hh, Ww, generator=g) * 0.5).cuda(), "audio": (torch.randn(B, 1, L, generator=g) * 0.5).cuda()}
    mv = torch.rand(B, F, Hh, Ww, generator=g) < 0.4          # per-sample cells
    ma = torch.zeros(L, dtype=torch.bool)
    ma[:L // 3 + 1] = True                                       # one row for the batch
    return known, {"video": mv, "audio": ma}


@pytest.mark.parametrize("px,order,steps", [(True, 3, 4), (False, 3, 4), (False, 2, 3)])
def test_partial_mask_is_the_host_composition(px, order, steps):
    """The host loop: ops.cond_replace before every model call (the stage evaluations at s1 and s2 too), solver.model_fn, and ops.lincomb
    with the table's coefficients for the state each row leaves."""
    from mm_diffusion import masking, ops
    fl, model, solver = _solver(torch.float32, px, False)
    B = 2
    x_T = _x_T(fl, B, 21)
    known, mask = _masks(fl, B, 2)
    kw = dict(steps=steps, order=order, skip_type="logSNR", denoise=True)
    try:
        _replay(model, 4)
        got = solver.sample_graph_singlestep(_clone(x_T), known=known, mask=mask, **kw)
        _replay(model, 4)
        raw = solver.sample_graph_singlestep(_clone(x_T), known=known, mask=mask, paste_known=False, **kw)
        _replay(model, 4)
        cond = masking.normalize(known, mask, {k: tuple(v.shape) for k, v in x_T.items()})
        tabs = solver.singlestep_tables(device="cuda", **kw)
        qtab = torch.from_numpy(tabs["tab2"]).cuda()
        assert tabs["rows"] == steps + 1

        def replace(x, j):
            x = _clone(x)
            for k, c in cond.items():
                ops.cond_replace(x[k], c.known, qtab, torch.full((B,), j, dtype=torch.int64, device="cuda"), mask=None if c.mask is None else c.mask.cuda(),
                                 noise=x_T[k])
            return x
        x = _clone(x_T)
        XB = MS = None
        with torch.no_grad():
            for j in range(tabs["rows"]):
                tau = tabs["timesteps"][j].expand(B)
                x = replace(x, j)
                row = {k: [float(v) for v in tabs["tab"][k][:, j]] for k in solver.KEYS}
                kind = int(row["video"][5])
                if kind == ops.DPM1_KIND_DENOISE:
                    x = solver.denoise_fn(x, tau)
                    continue
                m = solver.model_fn(x, tau)
                if kind == ops.DPM1_KIND_OPEN:
                    XB, MS = x, m
                    x = {k: ops.lincomb(XB[k], row[k][2], MS[k], row[k][3]) for k in solver.KEYS}
                else:
                    x = {k: ops.lincomb(XB[k], row[k][2], MS[k], row[k][3], m[k], row[k][4]) for k in solver.KEYS}
        for k in ("video", "audio"):
            assert same(raw[k], x[k]), k
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
    fl, model, solver = _solver(torch.float32, True, True)
    x_T = _x_T(fl, 2, 8)
    known, mask = _masks(fl, 2, 3)
    empty = {k: torch.zeros_like(m) for k, m in mask.items()}
    kw = dict(steps=4, order=3, skip_type="time_uniform", denoise=False)
    try:
        _replay(model, 6)
        want = solver.sample_graph_singlestep(_clone(x_T), **kw)
        _replay(model, 6)
        got = solver.sample_graph_singlestep(_clone(x_T), known=known, mask=empty, **kw)
    finally:
        model.shift_source = None
    assert same(got["video"], want["video"]) and same(got["audio"], want["audio"])
