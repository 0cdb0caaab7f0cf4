"""Masked conditional sampling on the device.  Kernel level: mmd_cond_replace against mmd_q_sample (bitwise on the known cells), against
the untouched input (bitwise elsewhere, guard values around x), against the float64 restatement within its derived bound (masked_ref.py),
the counter form against mmd_ctr_fill + the memory form, rows against batch-1 calls, the paste, repeat runs and the refused arguments.
Loop level: masked_sample_loop against the reference's fixture and the project's own whole-stream loop, against a host-side composition
of q_sample / torch.where / p_sample / ddim_sample for partial masks, and its invariances (graph / eager, lanes, batch composition)."""
import random

import numpy as np
import pytest
import torch

import masked_ref as R
from helpers import flags, gold, rel_l2, synth_sd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GUARD, SENTINEL = 64, 12345.0
IDS = [7, 2 ** 32 - 1, 8]


def _src(seed=42, **kw):
    from mm_diffusion.seeded import CounterNoise
    return CounterNoise(seed, **kw)


_DIFF = {}


def _diffusion():
    """T = 1000: the timesteps 0, T - 1 and 7 are three different table columns"""
    if "d" not in _DIFF:
        from mm_diffusion import multimodal_script_util as msu
        _DIFF["d"] = msu.create_gaussian_diffusion(steps=1000, timestep_respacing="")
    return _DIFF["d"]


def _guarded(values):
    """float32 [N, per] -> (the whole buffer with GUARD sentinels on each side, the view of its middle)"""
    buf = torch.full((values.size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + values.size].view(values.shape)
    view.copy_(torch.from_numpy(values))
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _dev_case(shape, seed):
    """-> numpy x / known / eps [N, per], the same on the device as [N, F, C, HW], the timesteps (numpy, device) and the tables"""
    N, F, C, HW = shape
    x, known, eps = R.make_case(shape, seed)
    diff = _diffusion()
    _, qtab = diff.device_tables(DEV)
    t = R.timesteps(N, qtab.shape[1])
    dk, de = (torch.from_numpy(a).to(DEV).view(N, F, C, HW) for a in (known, eps))
    return x, known, eps, dk, de, t, torch.from_numpy(t).to(DEV), qtab


def _dev_mask(mask):
    return None if mask is None else torch.from_numpy(mask).to(DEV)


def _q_sample(dk, de, qtab, dt):
    from mm_diffusion import ops
    return ops.q_sample(dk, de, torch.empty_like(dk), qtab, dt).view(dk.shape[0], -1).cpu().numpy()


# ----------------------------------------------------------------------------- kernel level, memory form
@pytest.mark.parametrize("shape", R.SMALL)
def test_memory_form_against_q_sample_the_input_and_the_bound(shape):
    from mm_diffusion import ops
    N, F, C, HW = shape
    x, known, eps, dk, de, t, dt, qtab = _dev_case(shape, 1)
    q = _q_sample(dk, de, qtab, dt)
    tab = qtab.cpu().numpy()
    worst = 0.0
    for kind, per_sample in R.MASKS:
        mask, stride = R.make_mask(kind, per_sample, shape)
        buf, dx = _guarded(x)
        ops.cond_replace(dx.view(N, F, C, HW), dk, qtab, dt, noise=de, mask=_dev_mask(mask))
        got = dx.cpu().numpy()
        y, on, bound = R.replace64(x, known, eps, shape, mask, stride, tab[0][t], tab[1][t])
        case = (shape, kind, per_sample)
        assert _guards_intact(buf), case
        assert np.array_equal(got[on].view(np.uint32), q[on].view(np.uint32)), case          # known cells: mmd_q_sample's bits
        assert np.array_equal(got[~on].view(np.uint32), x[~on].view(np.uint32)), case        # the others: never written
        nv = R.violations(got, y, bound)
        ratio = float((np.abs(got.astype(np.float64) - y)[on] / bound[on]).max()) if on.any() and (bound[on] > 0).all() else 0.0
        worst = max(worst, ratio)
        print(case, "known", int(on.sum()), "of", on.size, "violations", nv, "largest |err| / bound", ratio)
        assert nv == 0, case
        # a second run writes the same bits
        buf2, dx2 = _guarded(x)
        ops.cond_replace(dx2.view(N, F, C, HW), dk, qtab, dt, noise=de, mask=_dev_mask(mask))
        assert torch.equal(buf, buf2), case
    print(shape, "largest |err| / bound:", worst)


def test_memory_form_past_the_grid_cap():
    from mm_diffusion import ops
    shape = R.BIG_MEMORY
    N, F, C, HW = shape
    assert N * F * C * HW > 4096 * 256
    x, known, eps, dk, de, t, dt, qtab = _dev_case(shape, 2)
    q = _q_sample(dk, de, qtab, dt)
    tab = qtab.cpu().numpy()
    mask, stride = R.make_mask("random", True, shape)
    buf, dx = _guarded(x)
    ops.cond_replace(dx.view(N, F, C, HW), dk, qtab, dt, noise=de, mask=_dev_mask(mask))
    got = dx.cpu().numpy()
    y, on, bound = R.replace64(x, known, eps, shape, mask, stride, tab[0][t], tab[1][t])
    assert _guards_intact(buf)
    assert np.array_equal(got[on].view(np.uint32), q[on].view(np.uint32))
    assert np.array_equal(got[~on].view(np.uint32), x[~on].view(np.uint32))
    assert R.violations(got, y, bound) == 0


def test_host_scalars_and_the_paste():
    from mm_diffusion import ops
    for shape in (R.VIDEO, R.AUDIO, (2, 1, 1, 5)):
        N, F, C, HW = shape
        x, known, eps, dk, de, t, dt, qtab = _dev_case(shape, 3)
        for kind, per_sample in (("null", False), ("random", False), ("random", True), ("last", True), ("zeros", False)):
            mask, stride = R.make_mask(kind, per_sample, shape)
            on = R.known_cells(shape, mask, stride)
            # the paste: no noise tensor, x = known on the known cells, bit for bit
            buf, dx = _guarded(x)
            ops.cond_replace(dx.view(N, F, C, HW), dk, None, None, mask=_dev_mask(mask), coef=(1.0, 0.0))
            got = dx.cpu().numpy()
            assert _guards_intact(buf)
            assert np.array_equal(got[on].view(np.uint32), known[on].view(np.uint32)), (shape, kind, per_sample)
            assert np.array_equal(got[~on].view(np.uint32), x[~on].view(np.uint32)), (shape, kind, per_sample)
            # host scalars = the table's values of one timestep: the bits of the table form with that timestep for every sample
            tab = qtab.cpu().numpy()
            ca, cb = float(tab[0][7]), float(tab[1][7])
            t7 = torch.full((N,), 7, dtype=torch.int64, device=DEV)
            buf_a, xa = _guarded(x)
            buf_b, xb = _guarded(x)
            ops.cond_replace(xa.view(N, F, C, HW), dk, None, None, noise=de, mask=_dev_mask(mask), coef=(ca, cb))
            ops.cond_replace(xb.view(N, F, C, HW), dk, qtab, t7, noise=de, mask=_dev_mask(mask))
            assert torch.equal(buf_a, buf_b), (shape, kind, per_sample)
            y, _, bound = R.replace64(x, known, eps, shape, mask, stride, np.full(N, tab[0][7]), np.full(N, tab[1][7]))
            assert R.violations(xa.cpu().numpy(), y, bound) == 0


# ----------------------------------------------------------------------------- kernel level, counter form
def _ctr_pair(shape, tag, ids, mask, seed=4, t=None, coef=None):
    """(counter form, mmd_ctr_fill at the x_T draw + memory form) on the same inputs -> two guarded buffers and the case"""
    from mm_diffusion import ops
    from mm_diffusion.seeded import X_T
    N, F, C, HW = shape
    x, known, eps, dk, de, tn, dt, qtab = _dev_case(shape, seed)
    src = _src(42, sample_ids=ids)
    fill = src.randn((N, F, C, HW), tag, X_T, DEV)
    tabs = (None, None) if coef is not None else (qtab, dt)
    buf_c, xc = _guarded(x)
    buf_m, xm = _guarded(x)
    ops.cond_replace(xc.view(N, F, C, HW), dk, *tabs, ctr=(src.key(DEV), src.ids(N, DEV), tag), mask=_dev_mask(mask), coef=coef)
    ops.cond_replace(xm.view(N, F, C, HW), dk, *tabs, noise=fill, mask=_dev_mask(mask), coef=coef)
    return buf_c, buf_m, xc, (x, known, fill.view(N, -1).cpu().numpy(), tn, qtab.cpu().numpy())


@pytest.mark.parametrize("shape", R.SMALL)
def test_counter_form_is_fill_plus_memory_form(shape):
    N, F, C, HW = shape
    tag = 0 if F > 1 else 1
    for kind, per_sample in R.MASKS:
        mask, stride = R.make_mask(kind, per_sample, shape)
        buf_c, buf_m, xc, (x, known, fill, t, tab) = _ctr_pair(shape, tag, IDS[:N], mask)
        case = (shape, kind, per_sample)
        assert _guards_intact(buf_c), case
        assert torch.equal(buf_c, buf_m), case
        got = xc.cpu().numpy()
        y, on, bound = R.replace64(x, known, fill, shape, mask, stride, tab[0][t], tab[1][t])
        assert np.array_equal(got[~on].view(np.uint32), x[~on].view(np.uint32)), case
        assert R.violations(got, y, bound) == 0, case
        if kind == "null" and on.size >= 100:          # the noise went in, and each sample drew its own
            assert not np.array_equal(got[1], (tab[0][t[1]] * known[1]).astype(np.float32))
            assert not np.array_equal(fill[0], fill[1])
    # host scalars with the counter's noise
    mask, _ = R.make_mask("random", True, shape)
    buf_c, buf_m, _, _ = _ctr_pair(shape, tag, IDS[:N], mask, coef=(0.75, 0.5))
    assert torch.equal(buf_c, buf_m)


def test_counter_form_past_the_grid_cap():
    shape = R.BIG_COUNTER
    N, F, C, HW = shape
    assert (HW + 3) // 4 * N > 4096 * 256
    mask, stride = R.make_mask("random", True, shape)
    buf_c, buf_m, xc, (x, known, fill, t, tab) = _ctr_pair(shape, 1, IDS[:N], mask)
    assert _guards_intact(buf_c)
    assert torch.equal(buf_c, buf_m)
    got = xc.cpu().numpy()
    y, on, bound = R.replace64(x, known, fill, shape, mask, stride, tab[0][t], tab[1][t])
    assert np.array_equal(got[~on].view(np.uint32), x[~on].view(np.uint32))
    assert R.violations(got, y, bound) == 0


@pytest.mark.parametrize("shape", [R.VIDEO, (3, 1, 1, 1603), (3, 1, 1, 5)])
def test_rows_do_not_depend_on_the_batch(shape):
    """N = 3 equals three N = 1 calls, both forms, per-sample masks, timesteps and ids"""
    from mm_diffusion import ops
    N, F, C, HW = shape
    tag = 0 if F > 1 else 1
    x, known, eps, dk, de, t, dt, qtab = _dev_case(shape, 5)
    mask, _ = R.make_mask("random", True, shape)
    dm = _dev_mask(mask)
    dx = torch.from_numpy(x).to(DEV).view(N, F, C, HW)
    src = _src(42, sample_ids=IDS)
    whole_m, whole_c = dx.clone(), dx.clone()
    ops.cond_replace(whole_m, dk, qtab, dt, noise=de, mask=dm)
    ops.cond_replace(whole_c, dk, qtab, dt, ctr=(src.key(DEV), src.ids(N, DEV), tag), mask=dm)
    assert not torch.equal(whole_m, dx) and not torch.equal(whole_c, whole_m)
    for r in range(N):
        one = _src(42, sample_ids=[IDS[r]])
        row_m, row_c = dx[r:r + 1].clone(), dx[r:r + 1].clone()
        ops.cond_replace(row_m, dk[r:r + 1], qtab, dt[r:r + 1], noise=de[r:r + 1], mask=dm[r:r + 1])
        ops.cond_replace(row_c, dk[r:r + 1], qtab, dt[r:r + 1], ctr=(one.key(DEV), one.ids(1, DEV), tag), mask=dm[r:r + 1])
        assert torch.equal(row_m[0], whole_m[r]) and torch.equal(row_c[0], whole_c[r]), r


def test_refused_arguments_return_their_error_without_a_launch():
    from mm_diffusion import _hip, ops
    from mm_diffusion._hip import MMDError
    lib = _hip.lib()
    N, F, C, HW = R.VIDEO
    x, known, eps, dk, de, t, dt, qtab = _dev_case(R.VIDEO, 6)
    dx = torch.from_numpy(x).to(DEV)
    before = dx.clone()
    m = torch.ones(N, F * HW, dtype=torch.uint8, device=DEV)
    src = _src(42, sample_ids=IDS)
    key, ids = src.key(DEV), src.ids(N, DEV)
    T = qtab.shape[1]
    P = lambda v: None if v is None else v.data_ptr()      # noqa: E731

    def mem(x=dx, known=dk, noise=de, mask=m, stride=F * HW, tab2=qtab, t=dt, ca=1.0, cb=0.0, T=T, N=N, F=F, C=C, HW=HW):
        return lib.mmd_cond_replace(P(x), P(known), P(noise), P(mask), stride, P(tab2), P(t), ca, cb, T, N, F, C, HW, None)

    def ctr(x=dx, known=dk, key=key, ids=ids, tag=0, mask=m, stride=F * HW, tab2=qtab, t=dt, ca=1.0, cb=0.0, T=T, N=N, F=F, C=C, HW=HW):
        return lib.mmd_cond_replace_ctr(P(x), P(known), P(key), P(ids), tag, P(mask), stride, P(tab2), P(t), ca, cb, T, N, F, C, HW, None)
    bad = [dict(x=None), dict(known=None), dict(tab2=None), dict(N=0), dict(F=0), dict(C=-1), dict(HW=0), dict(T=0), dict(stride=HW),
           dict(stride=F * HW + 1), dict(stride=-1)]
    for kw in bad:
        for fn in (mem, ctr):
            assert fn(**kw) == -1 and b"cond_replace" in lib.mmd_last_error(), kw
    assert mem(noise=None) == -1                                  # t given: the noise is needed
    assert mem(noise=None, t=None, tab2=None, cb=0.5) == -1       # host scalars with cb != 0 as well
    for kw in (dict(key=None), dict(ids=None), dict(tag=-1), dict(tag=4)):
        assert ctr(**kw) == -1 and b"cond_replace_ctr" in lib.mmd_last_error(), kw
    assert ctr(N=1, F=1, C=2 ** 20, HW=2 ** 15, stride=2 ** 15) == -1 and b"too large" in lib.mmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dx, before)                                # nothing ran
    # the op's own checks
    dx4 = dx.view(N, F, C, HW)
    for kw in (dict(noise=de.double()), dict(noise=de, mask=m.bool()), dict(noise=de, mask=m[:, :-1].contiguous()), dict(noise=de, ctr=(key, ids, 0)),
               dict(), dict(noise=de, coef=(1.0, 0.0)), dict(noise=de.cpu())):
        with pytest.raises(MMDError):
            ops.cond_replace(dx4, dk, qtab, dt, **kw)
    with pytest.raises(MMDError):
        ops.cond_replace(dx4, dk, None, None, coef=(1.0, 0.5))
    with pytest.raises(MMDError):
        ops.cond_replace(dx4, dk, qtab, dt.int(), noise=de)
    assert torch.equal(dx, before)


def test_a_plan_records_and_replays_the_op():
    from mm_diffusion import _hip as H, ops
    N, F, C, HW = R.VIDEO
    x, known, eps, dk, de, t, dt, qtab = _dev_case(R.VIDEO, 7)
    mask, _ = R.make_mask("random", True, R.VIDEO)
    dm = _dev_mask(mask)
    a, b = (torch.from_numpy(x).to(DEV).view(N, F, C, HW) for _ in range(2))
    ops.cond_replace(a, dk, qtab, dt, noise=de, mask=dm)
    plan = []
    with ops.recording(plan):
        ops.cond_replace(b, dk, qtab, dt, noise=de, mask=dm)
    assert [op[2] for op in plan] == ["mmd_cond_replace"] and not torch.equal(a, b)
    ops.run_plan(plan, H.stream_handle())
    assert torch.equal(a, b)


# ----------------------------------------------------------------------------- loop level, tiny model at timestep_respacing="4"
_MODELS = {}
DTYPES = [torch.float32, torch.bfloat16]


def _model(dt):
    if dt not in _MODELS:
        from mm_diffusion import logger, multimodal_script_util as msu
        logger.set_quiet(True)
        fl = flags("tiny", timestep_respacing="4", use_fp16=(dt == torch.bfloat16))
        model, diff = msu.create_model_and_diffusion(**fl)
        model.load_state_dict(synth_sd("tiny"))
        model.cuda().eval()
        assert model.dtype == dt and diff.noise_source is None
        g = torch.Generator().manual_seed(21)
        known = {"video": (0.5 * torch.randn(4, *fl["video_size"], generator=g)).to(DEV),
                 "audio": (0.5 * torch.randn(4, *fl["audio_size"], generator=g)).to(DEV)}
        _MODELS[dt] = fl, model, diff, known
    return _MODELS[dt]


def _shape(fl, B):
    return {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}


def _seed(model, diff, s=5):
    """The CPU noise source of the parity tests on a seeded generator; the window shifts a fixed sequence by call order."""
    calls = [0]

    def shift(lo, hi):
        calls[0] += 1
        return lo + (7 * calls[0] + 3) % (hi - lo + 1)
    model.shift_source = shift
    diff.noise_source = lambda like: torch.randn(like.shape).to(like.device)
    torch.manual_seed(s)


def _masks(fl, kind, B):
    from mm_diffusion import masking
    F, _, Hh, Ww = fl["video_size"]
    L = fl["audio_size"][1]
    g = torch.Generator().manual_seed(31)
    if kind == "prefix3":
        return masking.prefix_masks(fl["video_size"], fl["audio_size"], 3)
    if kind == "random":                # per sample, both streams; the last row's masks are empty
        m = {"video": torch.rand(B, F, Hh, Ww, generator=g) < 0.5, "audio": torch.rand(B, L, generator=g) < 0.5}
        m["video"][-1] = False
        m["audio"][-1] = False
        return m
    if kind == "audio":                 # video free, the first 200 audio samples known
        a = torch.zeros(L, dtype=torch.uint8)
        a[:200] = 3
        return {"audio": a}
    if kind == "zeros":
        return {"video": torch.zeros(F, Hh, Ww, dtype=torch.bool), "audio": torch.zeros(B, L, dtype=torch.bool)}
    raise ValueError(kind)


def _known(known, masks, B, first=0):
    return {k: known[k][first:first + B].clone() for k in masks}


def _broadcast(mask, like):
    """bool mask [F,H,W] / [B,F,H,W] / [L] / [B,L] -> broadcastable against video [B,F,C,H,W] / audio [B,C,L]"""
    m = mask.to(DEV) != 0
    if like.dim() == 5:
        m = m if m.dim() == 4 else m.unsqueeze(0)
        return m.unsqueeze(2).expand_as(like)
    m = m if m.dim() == 2 else m.unsqueeze(0)
    return m.unsqueeze(1).expand_as(like)


def _new_loop(dt, kind, B, sampler="ddpm", eta=0.0, seed=5, **kw):
    fl, model, diff, known = _model(dt)
    masks = _masks(fl, kind, B)
    _seed(model, diff, seed)
    try:
        return [{k: v.clone() for k, v in s.items()} for s in
                diff.masked_sample_loop_progressive(model, _shape(fl, B), _known(known, masks, B), masks, sampler=sampler, eta=eta, device=DEV, **kw)]
    finally:
        diff.noise_source = None


def _composition(dt, kind, B, sampler="ddpm", eta=0.0, seed=5, paste=True):
    """The host loop of existing pieces: x[k] = where(mask, q_sample(known[k], t, noise = x_T[k]), x[k]), then p_sample / ddim_sample."""
    fl, model, diff, known = _model(dt)
    masks = _masks(fl, kind, B)
    kn = _known(known, masks, B)
    _seed(model, diff, seed)
    try:
        shape = _shape(fl, B)
        x_T = {k: torch.randn(*shape[k]).to(DEV) for k in ("video", "audio")}
        x = dict(x_T)
        out = []
        for i in range(diff.num_timesteps)[::-1]:
            t = torch.tensor([i] * B, device=DEV)
            for k in masks:
                x[k] = torch.where(_broadcast(masks[k], x[k]), diff.q_sample(kn[k], t, noise=x_T[k]), x[k])
            with torch.no_grad():
                x = (diff.ddim_sample(model, x, t, eta=eta) if sampler == "ddim" else diff.p_sample(model, x, t))["sample"]
            if paste and i == 0:
                x = {k: torch.where(_broadcast(masks[k], x[k]), kn[k], x[k]) if k in masks else x[k] for k in x}
            out.append({k: v.clone() for k, v in x.items()})
        return out
    finally:
        diff.noise_source = None


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u[k], v[k]) for u, v in zip(a, b) for k in ("video", "audio"))


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
def test_whole_stream_matches_the_reference_and_the_existing_loop(use_graph, dt):
    from test_model_gpu import cpu_noise_source, replay
    from test_sampling_api_gpu import API_TOL
    g = gold("tiny_cond_video_replace4")
    fl, model, diff, _ = _model(dt)
    B = int(g["B"])
    cond = torch.from_numpy(g["cond"]).cuda()
    finals = []
    try:
        for new in (True, False):
            replay(model, g["shifts"])
            diff.noise_source = cpu_noise_source()
            torch.manual_seed(int(g["seed"]))
            if new:
                gen = diff.masked_sample_loop_progressive(model, _shape(fl, B), {"video": cond}, None, paste_known=False, device=DEV, use_graph=use_graph)
            else:
                gen = diff.conditional_p_sample_loop_progressive_unscale(model, _shape(fl, B), False, model_kwargs={"video": cond}, device=DEV,
                                                                         use_graph=use_graph)
            finals.append([{k: v.clone() for k, v in s.items()} for s in gen])
    finally:
        diff.noise_source, model.shift_source = None, None
    final = finals[0][-1]
    ev, ea = rel_l2(final["video"].cpu(), g["video"]), rel_l2(final["audio"].cpu(), g["audio"])
    print(f"masked whole-stream {dt} graph={use_graph}: rel-L2 vs tiny_cond_video_replace4 video {ev:.3e} audio {ea:.3e}")
    assert ev < API_TOL[dt] and ea < API_TOL[dt]
    assert _same(finals[0], finals[1])          # every state of the trajectory, bit for bit


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,sampler,eta", [("prefix3", "ddpm", 0.0), ("random", "ddpm", 0.0), ("audio", "ddpm", 0.0), ("prefix3", "ddim", 0.0),
                                              ("random", "ddim", 0.5)])
def test_partial_masks_equal_the_composition_of_existing_pieces(dt, kind, sampler, eta):
    B = 2
    want = _composition(dt, kind, B, sampler, eta)
    got = _new_loop(dt, kind, B, sampler, eta)
    assert torch.isfinite(got[-1]["video"]).all() and torch.isfinite(got[-1]["audio"]).all()
    assert _same(got, want), (kind, sampler, eta)
    assert _same(_new_loop(dt, kind, B, sampler, eta, use_graph=False), want), (kind, sampler, eta, "eager")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sampler,eta", [("ddpm", 0.0), ("ddim", 0.5)])
def test_empty_masks_give_the_unconditional_trajectory(dt, sampler, eta):
    fl, model, diff, _ = _model(dt)
    B = 4
    _seed(model, diff)
    try:
        if sampler == "ddpm":
            gen = diff.p_sample_loop_progressive(model, _shape(fl, B), device=DEV)
        else:
            gen = diff.ddim_sample_loop_progressive(model, _shape(fl, B), device=DEV, eta=eta)
        free = [{k: v.clone() for k, v in s.items()} for s in gen]
    finally:
        diff.noise_source = None
    assert _same(_new_loop(dt, "zeros", B, sampler, eta), free)
    # per-sample masks in a batch of 4: the row whose masks are empty (the last) is its own unconditional trajectory, the others are not
    got = _new_loop(dt, "random", B, sampler, eta)
    for s, f in zip(got, free):
        for k in ("video", "audio"):
            assert torch.equal(s[k][-1], f[k][-1])
    assert all(not torch.equal(got[-1]["video"][r], free[-1]["video"][r]) for r in range(B - 1))


@pytest.mark.parametrize("dt", DTYPES)
def test_paste_and_the_condition_acts(dt):
    fl, model, diff, known = _model(dt)
    B = 2
    masks = _masks(fl, "prefix3", B)
    pasted = _new_loop(dt, "prefix3", B)
    raw = _new_loop(dt, "prefix3", B, paste_known=False)
    assert _same(pasted[:-1], raw[:-1])          # only the last state is pasted
    fl_ = _shape(fl, B)
    _seed(model, diff)
    try:
        free = [s for s in diff.p_sample_loop_progressive(model, fl_, device=DEV)][-1]
    finally:
        diff.noise_source = None
    for k in ("video", "audio"):
        on = _broadcast(masks[k], pasted[-1][k])
        assert torch.equal(pasted[-1][k][on], known[k][:B][on])                     # the known cells are `known`, bit for bit
        assert torch.equal(pasted[-1][k][~on], raw[-1][k][~on])                     # the paste wrote nothing else
        assert not torch.equal(raw[-1][k][on], known[k][:B][on])                    # (the raw step output is not)
        assert not torch.equal(pasted[-1][k][~on], free[k][~on])                    # the condition reached the unknown region


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_graph_eager_and_lane_counts_agree(dt, sampler):
    B, eta = 4, 0.5
    ref = _new_loop(dt, "random", B, sampler, eta, lanes=2)
    assert _same(_new_loop(dt, "random", B, sampler, eta, lanes=1), ref), "one lane"
    assert _same(_new_loop(dt, "random", B, sampler, eta, use_graph=False), ref), "eager"
    assert _same(_new_loop(dt, "random", B, sampler, eta), ref), "default lanes"


def _ctr_loop(dt, B, first, sampler, seed=42, **kw):
    """Rows first ... first + B - 1 of `seed` under the per-sample random masks of a batch of 4 -> [B, video + audio values]"""
    fl, model, diff, known = _model(dt)
    masks = {k: v[first:first + B] for k, v in _masks(fl, "random", 4).items()}
    model.shift_source = None
    diff.noise_source = _src(seed, first_sample=first)
    try:
        final = diff.masked_sample_loop(model, _shape(fl, B), _known(known, masks, B, first), masks, sampler=sampler, eta=0.5, device=DEV, **kw)
    finally:
        diff.noise_source = None
    return torch.cat([final["video"].float().flatten(1), final["audio"].float().flatten(1)], dim=1).clone()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_counter_noise_sample_k_is_the_same_in_any_batch(dt, sampler):
    ref = _ctr_loop(dt, 4, 0, sampler)
    assert torch.isfinite(ref).all() and len({ref[r].cpu().numpy().tobytes() for r in range(4)}) == 4
    assert torch.equal(torch.cat([_ctr_loop(dt, 2, 0, sampler), _ctr_loop(dt, 2, 2, sampler)]), ref), "batch 2 + batch 2"
    assert torch.equal(torch.cat([_ctr_loop(dt, 1, k, sampler) for k in range(4)]), ref), "four batch-1 runs"
    assert torch.equal(_ctr_loop(dt, 4, 0, sampler, use_graph=False), ref), "eager"
    assert torch.equal(_ctr_loop(dt, 4, 0, sampler, lanes=1), ref), "one lane"
    torch.randn(1000)
    torch.randn(1000, device=DEV)
    random.seed(99)
    [random.randint(0, 7) for _ in range(17)]
    assert torch.equal(_ctr_loop(dt, 4, 0, sampler), ref), "after unrelated draws"
    assert not torch.equal(_ctr_loop(dt, 1, 2, sampler, seed=43)[0], ref[2]), "another seed"


def test_counter_noise_takes_no_noise_tensors_and_the_stepper_records_the_ctr_kernel():
    from mm_diffusion import masking
    from mm_diffusion._hip import MMDError
    from mm_diffusion.sampler import GraphStepper
    fl, model, diff, known = _model(torch.float32)
    B = 2
    shape = _shape(fl, B)
    masks = _masks(fl, "audio", B)
    kn = _known(known, masks, B)
    noise = {k: torch.randn(*shape[k], device=DEV) for k in shape}
    diff.noise_source = _src(42)
    try:
        with pytest.raises(MMDError):
            diff.masked_sample_loop(model, shape, kn, masks, noise=noise, device=DEV)
    finally:
        diff.noise_source = None
    names = lambda plans: [[op[2] for op in plan] for plan in plans]      # noqa: E731
    cond = masking.normalize({"video": known["video"][:B], "audio": known["audio"][:B]}, {"audio": masks["audio"].to(DEV)}, shape)
    st = GraphStepper(diff, model, B, DEV, cond=cond, lanes=1)
    assert names(st.pre_plans) == [["mmd_cond_replace", "mmd_cond_replace"]] and st.cond["video"]["mask"] is None
    assert st.cond["audio"]["noise"].shape == (B, *fl["audio_size"])
    with pytest.raises(MMDError):
        st.load_cond(cond)                       # the fixed conditioning noise is missing
    st.close()
    st = GraphStepper(diff, model, B, DEV, lanes=1)
    assert st.pre_plans == [] and st.cond == {}          # cond=None records nothing
    st.close()
    diff.noise_source = _src(42)
    try:
        st = GraphStepper(diff, model, B, DEV, update="ddim", cond={"audio": cond["audio"]}, lanes=2)
        assert names(st.pre_plans) == [["mmd_cond_replace_ctr"], ["mmd_cond_replace_ctr"]] and st.cond["audio"]["noise"] is None
        st.close()
        with pytest.raises(MMDError):
            GraphStepper(diff, model, B, DEV, update="vlb", cond=cond)
    finally:
        diff.noise_source = None


def test_user_noise_is_x_T_and_the_conditioning_noise():
    """noise= handed in: the same trajectory as the run that drew that x_T itself"""
    dt = torch.float32
    fl, model, diff, known = _model(dt)
    B = 2
    masks = _masks(fl, "prefix3", B)
    ref = _new_loop(dt, "prefix3", B)
    _seed(model, diff)
    try:
        shape = _shape(fl, B)
        x_T = {k: torch.randn(*shape[k]).to(DEV) for k in ("video", "audio")}
        keep = {k: v.clone() for k, v in x_T.items()}
        for use_graph in (True, False):
            _seed(model, diff)
            {k: torch.randn(*shape[k]) for k in ("video", "audio")}          # (the draws the other run spent on x_T)
            got = [s for s in diff.masked_sample_loop_progressive(model, shape, _known(known, masks, B), masks, noise=x_T, device=DEV, use_graph=use_graph)]
            assert _same(got, ref), use_graph
            assert all(torch.equal(x_T[k], keep[k]) for k in x_T)          # the caller's tensors are not written
    finally:
        diff.noise_source = None
