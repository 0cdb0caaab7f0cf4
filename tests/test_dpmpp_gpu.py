"""The graph-replayed DPM-Solver / DPM-Solver++ multistep loop on the GPU: the new kernels bitwise against the kernels the eager loop
launches (mmd_lincomb, mmd_abs_quantile, mmd_clamp_scale), and DPM_Solver.sample_graph bitwise against sample(method="multistep").

Bounds.  Everything compared with the eager kernels is compared bit for bit.  The quantile against torch.quantile keeps the rtol of
1e-6 of test_dpm_solver_gpu.py; the loops against the reference fixtures keep its rel-L2 of 1e-4."""
import itertools
import random

import numpy as np
import pytest
import torch

import dpmpp_ref as R
from helpers import gold, rel_l2

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- selection
@pytest.mark.parametrize("per", R.PER_CASES)
def test_selection_is_bitwise_abs_quantile(per):
    """Bitwise against mmd_abs_quantile on every case; rtol 1e-6 against torch.quantile.

    torch.quantile is evaluated on the float64 copy of |x| at the fp32 q the C ABI receives.  On fp32 input it computes the rank
    q (per - 1) in fp32, whose rounding (up to (per - 1) 2^-24 of a rank) moves the interpolated value by more than the bound where the
    neighbours lie apart: measured at per = 4096, N(0, 0.3^2), q = 0.995: torch fp32 0.83366829, torch float64 0.83367059, float64 at the
    fp32 q 0.83367104, both kernels 0.83367103.
    Where one of the two wanted ranks is infinite (the "inf" inputs at 1 - 3 elements, or q = 1) both interpolation formulas leave the
    IEEE artefacts of inf - inf and 0 inf, and not the same ones (per = 3, q = 0.995: kernels inf, torch fp32 NaN; per = 3, q = 0.5, an
    infinite upper neighbour at weight 0: kernels NaN, torch the finite lower neighbour): there the kernels are compared with each other
    bit for bit, and their result must be non-finite."""
    from mm_diffusion import ops
    for N in (1, 3):
        ws = ops.dpmpp_workspace(N, "cuda")
        for kind, q in itertools.product(R.INPUT_KINDS, R.Q_CASES):
            xh = R.make_input(kind, N, per)
            x = torch.from_numpy(xh).cuda()
            old = ops.abs_quantile(x, q)
            new = ops.dpmpp_select(x, q, torch.empty(N, device="cuda"), ws)
            want = torch.quantile(x.abs().cpu().double(), float(np.float32(q)), dim=1).numpy().astype(np.float32)      # in the output's format
            got = new.cpu().numpy()
            print(f"per {per} N {N} {kind} q {q}: new {got} old {old.cpu().numpy()} torch {want}")
            assert same(new, old), (N, kind, q)
            assert int(ws.abs().max()) == 0, "the workspace must be zero again"
            lo, hi, _ = R.ranks(per, q)
            for n in range(N):
                if max(R.partition_bits(xh[n], lo), R.partition_bits(xh[n], hi)) < 0x7F800000:
                    np.testing.assert_allclose(got[n], want[n], rtol=1e-6, err_msg=f"{N} {kind} {q} sample {n}")
                else:
                    assert not np.isfinite(got[n]), (N, kind, q, n, got[n], want[n])


def _x0_case(Cm_factor, seed=0):
    N, F, C, HW = 3, 3, 3, 683            # 6147 elements a sample: one workgroup's chunk, and a second one of three elements
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, F, C, HW, generator=g).cuda()
    mo = (torch.randn(N, F, C * Cm_factor, HW, generator=g) * 1.5).cuda()
    tab = torch.zeros(6, 4)
    tab[0] = torch.tensor([1.7, 157.41, 1.0002, 3.0])
    tab[1] = torch.tensor([-1.3, -157.40, -0.017, 0.5])
    return N, F, C, HW, x, mo, tab.cuda()


@pytest.mark.parametrize("Cm_factor", [1, 2])
def test_x0_is_bitwise_lincomb_and_its_histogram_is_bincount(Cm_factor):
    from mm_diffusion import ops
    N, F, C, HW, x, mo, tab = _x0_case(Cm_factor)
    eps = mo[:, :, :C].contiguous()
    for row in range(4):
        k = torch.full((N,), row, dtype=torch.int64, device="cuda")
        want = ops.lincomb(x, float(tab[0, row]), eps, float(tab[1, row]))
        ws = ops.dpmpp_workspace(N, "cuda")
        got = ops.dpmpp_x0(x, mo, torch.full_like(x, 7.0), tab, k, F, C, C * Cm_factor, HW, hist=ws)
        assert same(got, want), row
        plain = ops.dpmpp_x0(x, mo, torch.full_like(x, 7.0), tab, k, F, C, C * Cm_factor, HW)
        assert same(plain, want), row
        w = ws.cpu().numpy().view(np.uint32).reshape(N, R.WS_WORDS)
        for n in range(N):
            np.testing.assert_array_equal(w[n, :R.L0_BINS], R.hist0(want[n].cpu().numpy()))
        assert not w[:, R.L0_BINS:].any()
        s = ops.dpmpp_select(got, 0.995, torch.empty(N, device="cuda"), ws, level0_done=True)
        assert same(s, ops.abs_quantile(want, 0.995))
        assert int(ws.abs().max()) == 0
    # a step number outside the table writes nothing
    k = torch.tensor([0, 4, -1], dtype=torch.int64, device="cuda")
    got = ops.dpmpp_x0(x, mo, torch.full_like(x, 7.0), tab, k, F, C, C * Cm_factor, HW)
    assert bool((got[1:] == 7.0).all()) and same(got[0], ops.lincomb(x, float(tab[0, 0]), eps, float(tab[1, 0]))[0])


GUARD = 64


def _guarded(t):
    """a copy of t with GUARD sentinel floats on either side -> (whole buffer, view of t's shape)"""
    buf = torch.full((t.numel() + 2 * GUARD,), -12345.0, device="cuda")
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
    return buf, buf[GUARD:GUARD + t.numel()].view(t.shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == -12345.0).all()) and bool((buf[-GUARD:] == -12345.0).all())


@pytest.mark.parametrize("Cm_factor", [1, 2])
@pytest.mark.parametrize("with_s", [True, False])
def test_update_is_bitwise_clamp_scale_and_lincomb(Cm_factor, with_s):
    from mm_diffusion import ops
    N, F, C, HW, x0, mo, _ = _x0_case(Cm_factor, seed=1)
    g = torch.Generator().manual_seed(5)
    m1_0 = torch.randn(N, F, C, HW, generator=g).cuda()
    tab = torch.zeros(6, 3)
    tab[2], tab[3], tab[4] = torch.tensor([0.99, 2.6, 5.0]), torch.tensor([0.01, -2.4, 5.0]), torch.tensor([0.0, 0.81, 5.0])
    tab[5] = torch.tensor([0.0, 1.0, 2.0])
    tab = tab.cuda()
    s = torch.tensor([0.4, 1.3, 2.9], device="cuda") if with_s else None
    max_val = 1.5
    m0 = mo[:, :, :C].clone()
    if with_s:
        ops.clamp_scale_(m0, s, max_val)
    for row in range(3):
        k = torch.full((N,), row, dtype=torch.int64, device="cuda")
        c0, c1, c2 = (float(tab[j, row]) for j in (2, 3, 4))
        want = (ops.lincomb(x0, c0, m0, c1), ops.lincomb(x0, c0, m0, c1, m1_0, c2), m0)[row]
        runs = []
        for _ in range(2):
            (bx, x), (bm, m1), (bo, mov) = _guarded(x0), _guarded(m1_0), _guarded(mo)
            ops.dpmpp_update(x, mov, m1, tab, k, F, C, C * Cm_factor, HW, s=s, max_val=max_val)
            assert same(x, want), row
            assert same(m1, m0), "M1 must be the clamped x0"
            assert same(mov, mo) and all(_guards_intact(b) for b in (bx, bm, bo))
            runs.append(x.clone())
        assert same(runs[0], runs[1])
        # a row does not depend on the batch: sample 1 alone
        x1, m11 = x0[1:2].clone(), m1_0[1:2].clone()
        ops.dpmpp_update(x1, mo[1:2].contiguous(), m11, tab, k[1:2].contiguous(), F, C, C * Cm_factor, HW, s=None if s is None else s[1:2].contiguous(),
                         max_val=max_val)
        assert same(x1, want[1:2]) and same(m11, m0[1:2])
    # first-order rows do not read M1: NaN there must not reach x (0 * NaN would)
    k = torch.zeros(N, dtype=torch.int64, device="cuda")
    x, m1 = x0.clone(), torch.full_like(x0, float("nan"))
    ops.dpmpp_update(x, mo, m1, tab, k, F, C, C * Cm_factor, HW, s=s, max_val=max_val)
    assert same(x, ops.lincomb(x0, float(tab[2, 0]), m0, float(tab[3, 0])))
    # a step number outside the table writes nothing
    k = torch.tensor([3, 0, -2], dtype=torch.int64, device="cuda")
    x, m1 = x0.clone(), m1_0.clone()
    ops.dpmpp_update(x, mo, m1, tab, k, F, C, C * Cm_factor, HW, s=s, max_val=max_val)
    assert same(x[0], x0[0]) and same(x[2], x0[2]) and same(m1[0], m1_0[0]) and not same(x[1], x0[1])


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


# (order, skip_type, predict_x0, thresholding, denoise, solver_type, steps, dtype)
LOOPS = [
    (2, "logSNR", True, True, True, "dpm_solver", 6, torch.float32),
    (2, "time_uniform", False, False, False, "dpm_solver", 6, torch.float32),
    (1, "time_quadratic", True, True, False, "dpm_solver", 5, torch.float32),
    (1, "logSNR", True, False, True, "dpm_solver", 4, torch.float32),
    (2, "time_quadratic", True, False, False, "taylor", 5, torch.float32),
    (2, "time_uniform", False, True, True, "dpm_solver", 5, torch.float32),
    (1, "time_uniform", False, False, False, "dpm_solver", 4, torch.float32),
    (2, "logSNR", True, True, True, "dpm_solver", 5, torch.bfloat16),
    (2, "time_quadratic", False, False, True, "dpm_solver", 4, torch.bfloat16),
]


@pytest.mark.parametrize("order,skip,px,thr,denoise,st,steps,dt", LOOPS)
def test_sample_graph_is_bitwise_the_eager_multistep_loop(order, skip, px, thr, denoise, st, steps, dt):
    """sample() runs under torch.no_grad() here, as a sampling script runs it.  With gradients enabled and trainable parameters its
    closing denoise evaluation - the one call it makes outside its own no_grad block - goes through the differentiable forward instead
    of the engine's launch plan, other kernels whose result differs from the plan's in the last bits (measured rel-L2 2e-7 on the
    result; the evaluations inside the loop are the plan's either way)."""
    fl, model, solver = _solver(dt, px, thr)
    try:
        x_T = _x_T(fl, 2, 11)
        kw = dict(steps=steps, order=order, skip_type=skip, denoise=denoise, solver_type=st)
        _replay(model, 3)
        with torch.no_grad():      # sample() takes its closing denoise evaluation outside its own no_grad block: see the docstring
            want = solver.sample({k: v.clone() for k, v in x_T.items()}, method="multistep", **kw)
        _replay(model, 3)
        got = solver.sample_graph({k: v.clone() for k, v in x_T.items()}, **kw)
        for k in ("video", "audio"):
            assert torch.isfinite(want[k]).all()
            assert same(got[k], want[k]), (k, rel_l2(got[k].cpu(), want[k].cpu()))
    finally:
        model.shift_source = None


@pytest.mark.parametrize("tag,px,thr,kw", [
    ("tiny_dpmpp_multistep2", True, True, dict(steps=10, order=2, skip_type="logSNR", denoise=True)),
    ("tiny_dpm_multistep2", False, False, dict(steps=10, order=2, skip_type="time_uniform")),
])
def test_sample_graph_matches_the_reference_fixtures(tag, px, thr, kw):
    g = gold(tag)
    fl, model, solver = _solver(torch.float32, px, thr)
    it = iter(int(s) for s in g["shifts"])
    model.shift_source = lambda lo, hi: next(it)
    try:
        B = int(g["B"])
        torch.manual_seed(int(g["seed"]))
        x_T = {"video": torch.randn(B, *fl["video_size"]).cuda(), "audio": torch.randn(B, *fl["audio_size"]).cuda()}
        out = solver.sample_graph(x_T, **kw)
    finally:
        model.shift_source = None
    ev, ea = rel_l2(out["video"].cpu(), g["video"]), rel_l2(out["audio"].cpu(), g["audio"])
    print(f"{tag}: rel-L2 video {ev:.3e} audio {ea:.3e}")
    assert next(it, None) is None, "different number of network evaluations than the reference"
    assert ev < 1e-4 and ea < 1e-4


def test_graph_and_eager_launch_and_lane_counts_agree():
    fl, model, solver = _solver(torch.float32, True, True)
    x_T = _x_T(fl, 4, 5)
    kw = dict(steps=4, order=2, skip_type="logSNR", denoise=True)
    outs = []
    try:
        for use_graph, lanes in ((True, 1), (False, 1), (True, 2), (False, 2)):
            _replay(model, 9)
            outs.append(solver.sample_graph({k: v.clone() for k, v in x_T.items()}, use_graph=use_graph, lanes=lanes, **kw))
    finally:
        model.shift_source = None
    for o in outs[1:]:
        assert same(o["video"], outs[0]["video"]) and same(o["audio"], outs[0]["audio"])


def test_kept_stepper_replays_both_plan_sets_on_another_grid():
    """The noise-prediction solver with denoise=True launches two plan sets, the step and the closing data prediction ("final"), each with
    graphs of its own.  A second call with another grid, order and step count reuses the kept stepper - both sets' captured graphs
    against reloaded tables - and must give the bits of a fresh solver and of the eager multistep loop (run under torch.no_grad(): see
    test_sample_graph_is_bitwise_the_eager_multistep_loop)."""
    fl, model, solver = _solver(torch.float32, False, False)
    x_T = _x_T(fl, 2, 7)
    calls = [dict(steps=4, order=2, skip_type="time_uniform", denoise=True), dict(steps=6, order=1, skip_type="logSNR", denoise=True)]

    def run(fn, kw, **more):
        _replay(model, 13)
        with torch.no_grad():
            return fn({k: v.clone() for k, v in x_T.items()}, **kw, **more)
    try:
        got, kept = [], []
        for kw in calls:
            got.append(run(solver.sample_graph, kw))
            kept.append(solver._stepper[1])
        assert kept[1] is kept[0] and kept[0].final_plans, "the second call did not reuse the stepper, or it has no final plan set"
        for kw, g in zip(calls, got):
            fresh = run(_solver(torch.float32, False, False)[2].sample_graph, kw)
            eager = run(solver.sample, kw, method="multistep")
            for k in ("video", "audio"):
                assert torch.isfinite(g[k]).all()
                assert same(g[k], fresh[k]), (kw, k, "fresh solver", rel_l2(g[k].cpu(), fresh[k].cpu()))
                assert same(g[k], eager[k]), (kw, k, "eager loop", rel_l2(g[k].cpu(), eager[k].cpu()))
    finally:
        model.shift_source = None


@pytest.mark.parametrize("px,thr", [(True, True), (False, False)])
def test_counter_noise_samples_are_addressable(px, thr):
    from mm_diffusion.seeded import CounterNoise
    fl, model, solver = _solver(torch.float32, px, thr)
    assert model.shift_source is None
    shape = lambda B: {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}      # noqa: E731
    kw = dict(steps=4, order=2, skip_type="logSNR", denoise=True)
    full = solver.sample_graph(shape=shape(4), noise_source=CounterNoise(1234), **kw)
    halves = [solver.sample_graph(shape=shape(2), noise_source=CounterNoise(1234, first_sample=f), **kw) for f in (0, 2)]
    for k in ("video", "audio"):
        assert same(torch.cat([h[k] for h in halves]), full[k]), k
    for i in range(4):
        one = solver.sample_graph(shape=shape(1), noise_source=CounterNoise(1234, sample_ids=[i]), **kw)
        for k in ("video", "audio"):
            assert same(one[k][0], full[k][i]), (i, k)
    other = solver.sample_graph(shape=shape(1), noise_source=CounterNoise(1235, sample_ids=[0]), **kw)
    assert not same(other["video"][0], full["video"][0])
    with pytest.raises(Exception, match="x_T must be None"):
        solver.sample_graph(_x_T(fl, 2, 1), noise_source=CounterNoise(1), **kw)


def _masks(fl, B, seed):
    g = torch.Generator().manual_seed(seed)
    F, C, Hh, Ww = fl["video_size"]
    L = fl["audio_size"][1]
    known = {"video": (torch.randn(B, F, C, Hh, Ww, generator=g) * 0.5).cuda(), "audio": (torch.randn(B, 1, L, generator=g) * 0.5).cuda()}
    mv = torch.rand(B, F, Hh, Ww, generator=g) < 0.4          # per-sample cells
    ma = torch.zeros(L, dtype=torch.bool)
    ma[:L // 3 + 1] = True                                       # one row for the batch
    return known, {"video": mv, "audio": ma}


@pytest.mark.parametrize("px,thr,order", [(True, True, 2), (False, False, 2), (True, False, 1)])
def test_partial_mask_is_the_host_composition(px, thr, order):
    from mm_diffusion import masking, ops
    fl, model, solver = _solver(torch.float32, px, thr)
    B, steps = 2, 4
    x_T = _x_T(fl, B, 21)
    known, mask = _masks(fl, B, 2)
    kw = dict(steps=steps, order=order, skip_type="logSNR", denoise=True)
    try:
        _replay(model, 4)
        got = solver.sample_graph({k: v.clone() for k, v in x_T.items()}, known=known, mask=mask, **kw)
        raw = None
        _replay(model, 4)
        raw = solver.sample_graph({k: v.clone() for k, v in x_T.items()}, known=known, mask=mask, paste_known=False, **kw)
        # the host composition
        _replay(model, 4)
        shape = {k: tuple(v.shape) for k, v in x_T.items()}
        cond = masking.normalize(known, mask, shape)
        tabs = solver.graph_tables(steps, order, "logSNR", "dpm_solver", True, device="cuda")
        qtab = torch.from_numpy(tabs["tab2"]).cuda()
        ts = tabs["timesteps"]

        def replace(x, i):
            x = {k: v.clone() for k, v in x.items()}
            for k, c in cond.items():
                ops.cond_replace(x[k], c.known, qtab, torch.full((B,), i, dtype=torch.int64, device="cuda"), mask=None if c.mask is None else c.mask.cuda(),
                                 noise=x_T[k])
            return x
        x = {k: v.clone() for k, v in x_T.items()}
        models, times = [], []
        with torch.no_grad():
            for i in range(steps):
                vec_t = ts[i].expand(B)
                x = replace(x, i)
                models.append(solver.model_fn(x, vec_t))
                times.append(vec_t)
                o = 1 if i == 0 or order == 1 else 2
                nxt = solver.get_time_steps("logSNR", solver.noise_schedule.T, 1. / solver.noise_schedule.total_N, steps, "cpu")[i + 1].expand(B)
                x = solver.multistep_dpm_solver_update(x, models[-o:], times[-o:], nxt, o)
            x = replace(x, steps)
            x = solver.denoise_fn(x, torch.ones((B,)) * (1. / solver.noise_schedule.total_N))
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
    kw = dict(steps=4, order=2, skip_type="time_uniform", denoise=False)
    try:
        _replay(model, 6)
        want = solver.sample_graph({k: v.clone() for k, v in x_T.items()}, **kw)
        _replay(model, 6)
        got = solver.sample_graph({k: v.clone() for k, v in x_T.items()}, known=known, mask=empty, **kw)
    finally:
        model.shift_source = None
    assert same(got["video"], want["video"]) and same(got["audio"], want["audio"])
