"""Resampling jumps of masked sampling on the device.  Kernel level: mmd_renoise_ctr against mmd_ctr_fill + mmd_q_sample (bitwise), the
float64 restatement within its derived bound (repaint_ref.py), guard values, batch-1 calls and levels outside the table;
mmd_ddpm_update_ctr_at against mmd_ctr_fill(draw) + mmd_ddpm_update and, with draw == t, mmd_ddpm_update_ctr; the refused arguments.
Loop level, tiny model: masked_sample_loop with jump_length / n_resample against today's loop (n_resample = 1), against a host composition
of cond_replace's pieces, p_sample and q_sample over the restated schedule, and its invariances (graph / eager, lanes, batch composition)."""
import numpy as np
import pytest
import torch

import repaint_ref as R
from helpers import flags, synth_sd

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GUARD, SENTINEL = 64, 12345.0
IDS = [7, 2 ** 32 - 1, 8]
DRAWS = [0x80000000, 0x80000003, 13]          # per sample: two jump draws and a small one
J_K = 10                                      # the kernel cases jump 10 of 1000 levels


def _src(seed=42, **kw):
    from mm_diffusion.seeded import CounterNoise
    return CounterNoise(seed, **kw)


_DIFF = {}


def _diffusion(learn_sigma=False, resp=""):
    key = (learn_sigma, resp)
    if key not in _DIFF:
        from mm_diffusion import multimodal_script_util as msu
        _DIFF[key] = msu.create_gaussian_diffusion(steps=1000, learn_sigma=learn_sigma, timestep_respacing=resp)
    return _DIFF[key]


def _guarded(values):
    """float32 [N, per] -> (the whole buffer with GUARD sentinels on each side, the view of its middle)"""
    buf = torch.full((values.size + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + values.size].view(values.shape)
    view.copy_(torch.from_numpy(values))
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _i64(v):
    return torch.tensor([int(a) for a in v], dtype=torch.int64, device=DEV)


def _fill_rows(shape, tag, ids, draws):
    """mmd_ctr_fill(kind 0) per sample at its own draw -> [N, F, C, HW]"""
    return torch.cat([_src(42, sample_ids=[sid]).randn((1,) + tuple(shape[1:]), tag, d, DEV) for sid, d in zip(ids, draws)])


# ----------------------------------------------------------------------------- kernel level: the jump
def _jump_pair(shape, m, seed=1, ids=IDS, draws=DRAWS):
    """(mmd_renoise_ctr, mmd_ctr_fill + in-place mmd_q_sample) on the same input -> the two guarded buffers, the counter form's view, and
    the numpy x, z and table"""
    from mm_diffusion import ops
    N, F, C, HW = shape
    tag = 0 if F > 1 else 1
    x, _ = R.make_case(shape, seed)
    jtab = _diffusion().jump_tables(J_K, DEV)
    src = _src(42, sample_ids=ids[:N])
    fill = _fill_rows(shape, tag, ids[:N], draws[:N])
    dm, dd = _i64(m), _i64(draws[:N])
    buf_c, xc = _guarded(x)
    buf_m, xm = _guarded(x)
    ops.renoise_ctr(xc.view(N, F, C, HW), src.key(DEV), src.ids(N, DEV), tag, jtab, dm, dd)
    xm4 = xm.view(N, F, C, HW)
    ops.q_sample(xm4, fill, xm4, jtab, dm)
    return buf_c, buf_m, xc, (x, fill.view(N, -1).cpu().numpy(), jtab.cpu().numpy())


@pytest.mark.parametrize("shape", R.SHAPES)
def test_renoise_is_fill_plus_q_sample_within_the_bound(shape):
    N = shape[0]
    T = _diffusion().num_timesteps
    m = R.levels(N, T, J_K)
    buf_c, buf_m, xc, (x, z, tab) = _jump_pair(shape, m)
    assert _guards_intact(buf_c), shape
    assert torch.equal(buf_c, buf_m), shape                         # bitwise the memory form of the jump
    got = xc.cpu().numpy()
    y, bound = R.jump64(x, z, tab, m)
    nv = R.violations(got, y, bound)
    ratio = float((np.abs(got.astype(np.float64) - y) / np.maximum(bound, 1e-300)).max())
    print(shape, "violations", nv, "largest |err| / bound", ratio)
    assert nv == 0 and not np.array_equal(got, x)
    assert tab[0][m].min() > 0 and tab[1][m].min() > 0              # the levels used are levels a jump may leave
    # a second run writes the same bits
    buf_2, _, _, _ = _jump_pair(shape, m)
    assert torch.equal(buf_c, buf_2)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[2], (3, 1, 1, 5)])
def test_renoise_rows_do_not_depend_on_the_batch(shape):
    N = shape[0]
    T = _diffusion().num_timesteps
    m = R.levels(N, T, J_K)
    _, _, whole, _ = _jump_pair(shape, m)
    x, _ = R.make_case(shape, 1)
    rows = set()
    for r in range(N):
        from mm_diffusion import ops
        one = _src(42, sample_ids=[IDS[r]])
        xr = torch.from_numpy(x[r:r + 1]).to(DEV).view(1, *shape[1:])
        ops.renoise_ctr(xr, one.key(DEV), one.ids(1, DEV), 0 if shape[1] > 1 else 1, _diffusion().jump_tables(J_K, DEV), _i64(m[r:r + 1]), _i64(DRAWS[r:r + 1]))
        assert torch.equal(xr.view(-1), whole[r]), r
        rows.add(whole[r].cpu().numpy().tobytes())
    assert len(rows) == N


def test_a_level_outside_the_table_leaves_its_sample_untouched():
    shape = R.SHAPES[0]
    T = _diffusion().num_timesteps
    ok = R.levels(3, T, J_K)
    ref = _jump_pair(shape, ok)[2].cpu().numpy()
    for bad_row, bad in ((0, T), (1, -1), (2, 2 ** 40), (1, -2 ** 33)):
        m = ok.copy()
        m[bad_row] = bad
        from mm_diffusion import ops
        N, F, C, HW = shape
        x, _ = R.make_case(shape, 1)
        src = _src(42, sample_ids=IDS)
        buf, xc = _guarded(x)
        ops.renoise_ctr(xc.view(N, F, C, HW), src.key(DEV), src.ids(N, DEV), 0, _diffusion().jump_tables(J_K, DEV), _i64(m), _i64(DRAWS))
        got = xc.cpu().numpy()
        assert _guards_intact(buf)
        for r in range(3):
            want = x[r] if r == bad_row else ref[r]
            assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (bad_row, bad, r)


def test_the_draw_is_the_draw_and_not_the_level():
    shape = R.SHAPES[0]
    T = _diffusion().num_timesteps
    m = R.levels(3, T, J_K)
    a = _jump_pair(shape, m)[2].cpu().numpy()
    b = _jump_pair(shape, m, draws=[int(v) for v in m])[2].cpu().numpy()           # the seeded defect of test_repaint_cpu, as a run
    c = _jump_pair(shape, m, draws=[d + 1 for d in DRAWS])[2].cpu().numpy()
    x, z, tab = _jump_pair(shape, m)[3]
    y, bound = R.jump64(x, z, tab, m)
    assert R.violations(a, y, bound) == 0 and R.violations(b, y, bound) > y.size // 2 and R.violations(c, y, bound) > y.size // 2


# ----------------------------------------------------------------------------- kernel level: the update with a draw handed in
T_VEC = [0, 5, 2]


def _update_case(shape, learn_sigma, seed):
    N, F, C, HW = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, F, C, HW, generator=g).to(DEV)
    mo = (0.7 * torch.randn(N, F, 2 * C if learn_sigma else C, HW, generator=g)).to(DEV)
    return x, mo


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[1], R.SHAPES[2], R.SHAPES[3]])
@pytest.mark.parametrize("learn_sigma,clip", [(False, True), (True, False)])
def test_update_at_is_fill_at_the_draw_plus_memory_kernel(shape, learn_sigma, clip):
    from mm_diffusion import ops
    diff = _diffusion(learn_sigma, "8")
    tab, _ = diff.device_tables(DEV)
    N, F, C, HW = shape
    tag = 0 if F > 1 else 1
    x, mo = _update_case(shape, learn_sigma, 3)
    tv = T_VEC if N > 1 else [5]                          # (a batch of one runs a step that draws)
    t, draws = _i64(tv), [8 + 5, 2 * 8 + 5, 0x7FFFFFFF][:N]
    src = _src(42, sample_ids=IDS[:N])
    key, ids = src.key(DEV), src.ids(N, DEV)
    fl = diff._flags(clip)
    a = [torch.full_like(x, 9.0) for _ in range(4)]
    b = [torch.full_like(x, 7.0) for _ in range(4)]
    ops.ddpm_update(x, mo, _fill_rows(shape, tag, IDS[:N], draws), a[0], tab, t, F, C, HW, fl, x0_out=a[1], mean_out=a[2], logvar_out=a[3])
    ops.ddpm_update_ctr_at(x, mo, key, ids, tag, b[0], tab, t, _i64(draws), F, C, HW, fl, x0_out=b[1], mean_out=b[2], logvar_out=b[3])
    for name, u, v in zip(("sample", "x0", "mean", "logvar"), a, b):
        assert torch.equal(u, v), name
    assert torch.equal(a[0][0], a[2][0]) == (tv[0] == 0)  # t == 0: no noise, whatever the draw
    # draw == t: the kernel that takes the draw from t, bit for bit
    c, d = torch.full_like(x, 5.0), torch.full_like(x, 3.0)
    ops.ddpm_update_ctr(x, mo, key, ids, tag, c, tab, t, F, C, HW, fl)
    ops.ddpm_update_ctr_at(x, mo, key, ids, tag, d, tab, t, t.clone(), F, C, HW, fl)
    assert torch.equal(c, d)
    # only the low 32 bits of a draw count
    ops.ddpm_update_ctr_at(x, mo, key, ids, tag, d, tab, t, t + (1 << 32), F, C, HW, fl)
    assert torch.equal(c, d)
    r = N - 1 if N == 1 else 1                            # a sample that runs at t = 5
    assert not torch.equal(b[0][r], c[r])                 # two draws at one timestep: other noise
    if N > 1:
        e = torch.empty_like(x)
        ops.ddpm_update_ctr_at(x, mo, key, ids, tag, e, tab, t, _i64([d_ + 8 for d_ in draws]), F, C, HW, fl)
        assert not torch.equal(e[1], b[0][1]) and torch.equal(e[0], b[0][0])
    # the steppers' form: the sample alone, in place
    xin = x.clone()
    ops.ddpm_update_ctr_at(xin, mo, key, ids, tag, xin, tab, t, _i64(draws), F, C, HW, fl)
    assert torch.equal(xin, a[0])


def test_refused_arguments_return_their_error_without_a_launch():
    from mm_diffusion import _hip, ops
    from mm_diffusion._hip import MMDError
    lib = _hip.lib()
    shape = R.SHAPES[0]
    N, F, C, HW = shape
    diff = _diffusion(False, "8")
    tab, _ = diff.device_tables(DEV)
    jtab = diff.jump_tables(2, DEV)
    T = jtab.shape[1]
    x, mo = _update_case(shape, False, 6)
    before = x.clone()
    src = _src(42, sample_ids=IDS)
    key, ids = src.key(DEV), src.ids(N, DEV)
    t, dd = _i64(T_VEC), _i64(DRAWS)
    P = lambda v: None if v is None else v.data_ptr()      # noqa: E731

    def jump(x=x, key=key, ids=ids, tag=0, jtab=jtab, m=t, draw=dd, T=T, N=N, F=F, C=C, HW=HW):
        return lib.mmd_renoise_ctr(P(x), P(key), P(ids), tag, P(jtab), P(m), P(draw), T, N, F, C, HW, None)

    def upd(x=x, mo=mo, key=key, ids=ids, tag=0, out=x, tab=tab, t=t, draw=dd, T=T, N=N, F=F, C=C, HW=HW):
        return lib.mmd_ddpm_update_ctr_at(P(x), P(mo), P(key), P(ids), tag, P(out), None, None, None, P(tab), P(t), P(draw), T, N, F, C, HW, 1, None)
    for kw in (dict(x=None), dict(jtab=None), dict(m=None), dict(draw=None), dict(key=None), dict(ids=None), dict(tag=-1), dict(tag=4), dict(T=0),
               dict(N=0), dict(F=0), dict(C=-1), dict(HW=0)):
        assert jump(**kw) == -1 and b"renoise_ctr" in lib.mmd_last_error(), kw
    assert jump(N=1, F=1, C=2 ** 20, HW=2 ** 15) == -1 and b"too large" in lib.mmd_last_error()
    for kw in (dict(x=None), dict(mo=None), dict(tab=None), dict(t=None), dict(draw=None), dict(key=None), dict(ids=None), dict(tag=-1), dict(tag=4),
               dict(T=0), dict(N=0), dict(F=0), dict(C=-1), dict(HW=0)):
        assert upd(**kw) == -1 and b"ddpm_update_ctr_at" in lib.mmd_last_error(), kw
    assert upd(N=1, F=1, C=2 ** 20, HW=2 ** 15) == -1 and b"too large" in lib.mmd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before)                                 # nothing ran
    # the op's own checks
    for kw in (dict(x=x.double()), dict(x=x[:, :, :, ::2]), dict(jtab=jtab.double()), dict(jtab=jtab[0]), dict(m=t.int()), dict(m=t[:2]),
               dict(draw=dd.int()), dict(draw=dd[:1]), dict(ids=ids[:2]), dict(x=x.view(-1)), dict(m=t.cpu())):
        args = dict(x=x, key=key, ids=ids, tag=0, jtab=jtab, m=t, draw=dd)
        args.update(kw)
        with pytest.raises(MMDError):
            ops.renoise_ctr(**args)
    with pytest.raises(MMDError):
        ops.ddpm_update_ctr_at(x, mo, key, ids, 0, x, tab, t, dd.int(), F, C, HW, 1)
    with pytest.raises(MMDError):
        ops.ddpm_update_ctr_at(x, mo, key, ids, 0, x, tab, t, dd.cpu(), F, C, HW, 1)
    assert torch.equal(x, before)


# ----------------------------------------------------------------------------- loop level, tiny model
_MODELS = {}
DTYPES = [torch.float32, torch.bfloat16]
CONFIGS = [("8", 2, 2), ("4", 1, 2)]          # (timestep_respacing, jump_length, n_resample)


def _model(dt, resp):
    if (dt, resp) not in _MODELS:
        from mm_diffusion import logger, multimodal_script_util as msu
        logger.set_quiet(True)
        fl = flags("tiny", timestep_respacing=resp, use_fp16=(dt == torch.bfloat16))
        model, diff = msu.create_model_and_diffusion(**fl)
        model.load_state_dict(synth_sd("tiny"))
        model.cuda().eval()
        assert model.dtype == dt and diff.noise_source is None and diff.num_timesteps == int(resp)
        g = torch.Generator().manual_seed(21)
        known = {"video": (0.5 * torch.randn(4, *fl["video_size"], generator=g)).to(DEV),
                 "audio": (0.5 * torch.randn(4, *fl["audio_size"], generator=g)).to(DEV)}
        _MODELS[(dt, resp)] = fl, model, diff, known
    return _MODELS[(dt, resp)]


def _shape(fl, B):
    return {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}


def _seed(model, diff, s=5):
    """The CPU noise source on a seeded generator; the window shifts a fixed sequence by call order."""
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
    if kind == "prefix3":               # clip continuation: three frames and the audio they span
        return masking.prefix_masks(fl["video_size"], fl["audio_size"], 3)
    if kind == "audio":                 # audio continuation: video free, the first 200 audio samples known
        a = torch.zeros(L, dtype=torch.uint8)
        a[:200] = 3
        return {"audio": a}
    if kind == "spatial":               # inpainting: everything but a box of every frame is known, the audio is free
        v = torch.ones(F, Hh, Ww, dtype=torch.bool)
        v[:, Hh // 4:Hh // 4 + 7, 3:Ww - 4] = False
        return {"video": v}
    if kind == "random":                # per sample, both streams; the last row's masks are empty
        m = {"video": torch.rand(B, F, Hh, Ww, generator=g) < 0.5, "audio": torch.rand(B, L, generator=g) < 0.5}
        m["video"][-1] = False
        m["audio"][-1] = False
        return m
    raise ValueError(kind)


def _known(known, masks, B, first=0):
    return {k: known[k][first:first + B].clone() for k in masks}


def _broadcast(mask, like):
    m = mask.to(DEV) != 0
    if like.dim() == 5:
        m = m if m.dim() == 4 else m.unsqueeze(0)
        return m.unsqueeze(2).expand_as(like)
    m = m if m.dim() == 2 else m.unsqueeze(0)
    return m.unsqueeze(1).expand_as(like)


def _loop(dt, cfg, kind, B, seed=5, **kw):
    resp, J, U = cfg
    fl, model, diff, known = _model(dt, resp)
    masks = _masks(fl, kind, B)
    _seed(model, diff, seed)
    try:
        return [{k: v.clone() for k, v in s.items()} for s in
                diff.masked_sample_loop_progressive(model, _shape(fl, B), _known(known, masks, B), masks, device=DEV, **kw)]
    finally:
        diff.noise_source, model.shift_source = None, None


def _composition(dt, cfg, kind, B, seed=5):
    """The host loop of existing pieces over the restated schedule: a step is x[k] = where(mask, q_sample(known[k], t, noise = x_T[k]),
    x[k]) and p_sample; a jump is mmd_q_sample of the state and fresh noise (video first, then audio) by a jump table built here."""
    from mm_diffusion import ops
    resp, J, U = cfg
    fl, model, diff, known = _model(dt, resp)
    masks = _masks(fl, kind, B)
    kn = _known(known, masks, B)
    a, b = R.jump_coef(np.asarray(diff.alphas_cumprod, dtype=np.float64), J)
    jtab = torch.from_numpy(np.stack([a, b]).astype(np.float32)).to(DEV)
    _seed(model, diff, seed)
    try:
        shape = _shape(fl, B)
        x_T = {k: torch.randn(*shape[k]).to(DEV) for k in ("video", "audio")}
        x = dict(x_T)
        out = []
        for op, i, _ in R.schedule(diff.num_timesteps, J, U):
            t = torch.tensor([i] * B, device=DEV)
            if op == "jump":
                x = {k: ops.q_sample(x[k].contiguous(), torch.randn(*shape[k]).to(DEV), torch.empty_like(x[k]), jtab, t) for k in ("video", "audio")}
                continue
            for k in masks:
                x[k] = torch.where(_broadcast(masks[k], x[k]), diff.q_sample(kn[k], t, noise=x_T[k]), x[k])
            with torch.no_grad():
                x = diff.p_sample(model, x, t)["sample"]
            out.append({k: v.clone() for k, v in x.items()})
        out[-1] = {k: torch.where(_broadcast(masks[k], out[-1][k]), kn[k], out[-1][k]) if k in masks else out[-1][k] for k in out[-1]}
        return out
    finally:
        diff.noise_source, model.shift_source = None, None


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u[k], v[k]) for u, v in zip(a, b) for k in ("video", "audio"))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_one_resample_is_todays_loop(dt, cfg):
    resp, J, U = cfg
    today = _loop(dt, cfg, "prefix3", 2)
    assert len(today) == int(resp)
    assert _same(_loop(dt, cfg, "prefix3", 2, jump_length=J, n_resample=1), today)
    assert _same(_loop(dt, cfg, "prefix3", 2, jump_length=None, n_resample=U), today)
    assert _same(_loop(dt, cfg, "prefix3", 2, jump_length=J, n_resample=1, use_graph=False), today)
    # and resampling is another trajectory from the first jump on: the states up to it are today's
    got = _loop(dt, cfg, "prefix3", 2, jump_length=J, n_resample=U)
    first = next(n for n, (op, _, _) in enumerate(R.schedule(int(resp), J, U)) if op == "jump")
    assert _same(got[:first], today[:first]) and not torch.equal(got[first]["video"], today[first]["video"])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("kind", ["prefix3", "audio", "spatial"])
def test_resampled_loop_equals_the_composition_of_existing_pieces(dt, cfg, kind):
    resp, J, U = cfg
    B = 2
    want = _composition(dt, cfg, kind, B)
    got = _loop(dt, cfg, kind, B, jump_length=J, n_resample=U)
    assert len(got) == R.evaluations(int(resp), J, U)              # one state per evaluation, none per jump
    assert torch.isfinite(got[-1]["video"]).all() and torch.isfinite(got[-1]["audio"]).all()
    assert _same(got, want), (cfg, kind)
    assert _same(_loop(dt, cfg, kind, B, jump_length=J, n_resample=U, use_graph=False), want), (cfg, kind, "eager")
    # the known cells of the final state are `known`, bit for bit
    fl, _, _, known = _model(dt, resp)
    masks = _masks(fl, kind, B)
    for k in masks:
        on = _broadcast(masks[k], got[-1][k])
        assert torch.equal(got[-1][k][on], known[k][:B][on])
    raw = _loop(dt, cfg, kind, B, jump_length=J, n_resample=U, paste_known=False)
    assert _same(raw[:-1], got[:-1]) and not _same(raw[-1:], got[-1:])          # the paste follows the last evaluation only


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_graph_eager_and_lane_counts_agree(dt, cfg):
    resp, J, U = cfg
    kw = dict(jump_length=J, n_resample=U)
    ref = _loop(dt, cfg, "random", 4, lanes=2, **kw)
    assert len(ref) == R.evaluations(int(resp), J, U)
    assert _same(_loop(dt, cfg, "random", 4, lanes=1, **kw), ref), "one lane"
    assert _same(_loop(dt, cfg, "random", 4, use_graph=False, **kw), ref), "eager"
    assert _same(_loop(dt, cfg, "random", 4, **kw), ref), "default lanes"


def _ctr_loop(dt, cfg, B, first, seed=42, log=None, **kw):
    """Rows first ... first + B - 1 of `seed` under the per-sample random masks of a batch of 4 -> [B, video + audio values]"""
    resp, J, U = cfg
    fl, model, diff, known = _model(dt, resp)
    masks = {k: v[first:first + B] for k, v in _masks(fl, "random", 4).items()}
    model.shift_source = None
    src = _src(seed, first_sample=first)
    if log is not None:
        shifts = src.shifts

        def logged(i, unet):
            log.append((int(i), tuple(shifts(i, unet))))
            return shifts(i, unet)
        src.shifts = logged
    diff.noise_source = src
    try:
        states = list(diff.masked_sample_loop_progressive(model, _shape(fl, B), _known(known, masks, B, first), masks, device=DEV, jump_length=J,
                                                          n_resample=U, **kw))
    finally:
        diff.noise_source = None
    final = states[-1]
    return torch.cat([final["video"].float().flatten(1), final["audio"].float().flatten(1)], dim=1).clone(), len(states)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cfg", CONFIGS)
def test_counter_noise_sample_k_is_the_same_in_any_batch(dt, cfg):
    resp, J, U = cfg
    log = []
    ref, n = _ctr_loop(dt, cfg, 4, 0, log=log)
    assert n == R.evaluations(int(resp), J, U)
    assert torch.isfinite(ref).all() and len({ref[r].cpu().numpy().tobytes() for r in range(4)}) == 4
    # the steps drew their window shifts at the schedule's draws, and a second visit of a step drew others than its first
    steps = [(i, d) for op, i, d in R.schedule(int(resp), J, U) if op == "step"]
    assert [d for d, _ in log] == [d for _, d in steps]
    by_draw = dict(log)
    again = [(i, d) for i, d in steps if d != i]
    assert again and all(by_draw[d] != by_draw[i] for i, d in again)
    assert torch.equal(torch.cat([_ctr_loop(dt, cfg, 2, 0)[0], _ctr_loop(dt, cfg, 2, 2)[0]]), ref), "batch 2 + batch 2"
    assert torch.equal(torch.cat([_ctr_loop(dt, cfg, 1, k)[0] for k in range(4)]), ref), "four batch-1 runs"
    assert torch.equal(_ctr_loop(dt, cfg, 4, 0, use_graph=False)[0], ref), "eager"
    assert torch.equal(_ctr_loop(dt, cfg, 4, 0, lanes=1)[0], ref), "one lane"
    assert not torch.equal(_ctr_loop(dt, cfg, 1, 2, seed=43)[0][0], ref[2]), "another seed"


def test_the_stepper_records_the_jump_set_and_a_second_visit_draws_other_noise():
    from mm_diffusion import masking
    from mm_diffusion._hip import MMDError
    from mm_diffusion.sampler import GraphStepper
    fl, model, diff, known = _model(torch.float32, "8")
    B = 2
    shape = _shape(fl, B)
    masks = _masks(fl, "audio", B)
    names = lambda plans: [[op[2] for op in plan] for plan in plans]      # noqa: E731
    cond = masking.normalize({"audio": known["audio"][:B]}, {"audio": masks["audio"].to(DEV)}, shape)
    g = torch.Generator().manual_seed(3)
    x_T = {k: torch.randn(*shape[k], generator=g).to(DEV) for k in shape}
    model.shift_source = None
    # without a counter source: the jump is mmd_q_sample on the noise buffers, the step keeps the memory update
    st = GraphStepper(diff, model, B, DEV, cond=cond, lanes=1, jump_length=2)
    assert names(st.jump_plans) == [["sync", "mmd_q_sample", "mmd_q_sample", "sync"]]
    assert names(st.update_plans) == [["mmd_ddpm_update", "mmd_ddpm_update", "sync"]]
    assert st._sets["jump"].bare and not st._sets["step"].bare and st.draw.shape == (B,) and st.draw.dtype == torch.int64
    with pytest.raises(MMDError):
        st.jump(6, 0x80000000)                   # level 6 + 2 is past the last level
    st.close()
    st = GraphStepper(diff, model, B, DEV, lanes=1)
    assert st.jump_plans == [] and "jump" not in st._sets and st.draw is None
    with pytest.raises(MMDError):
        st.jump(0, 0x80000000)
    with pytest.raises(MMDError):
        st.set_step(3, draw=11)
    st.close()
    with pytest.raises(MMDError):
        GraphStepper(diff, model, B, DEV, update="ddim", jump_length=2)
    diff.noise_source = _src(42)
    try:
        plain = GraphStepper(diff, model, B, DEV, cond=cond, lanes=1)
        assert names(plain.update_plans) == [["mmd_ddpm_update_ctr", "mmd_ddpm_update_ctr", "sync"]]
        st = GraphStepper(diff, model, B, DEV, cond=cond, lanes=2, jump_length=2)
        assert names(st.jump_plans) == [["sync", "mmd_renoise_ctr", "mmd_renoise_ctr", "sync"]] * 2
        assert names(st.update_plans) == [["mmd_ddpm_update_ctr_at", "mmd_ddpm_update_ctr_at", "sync"]] * 2
        assert st.noise_v is None and st.noise_a is None

        def run(stepper, i, **kw):
            stepper.load(x_T["video"], x_T["audio"])
            stepper.load_cond(cond)
            stepper.step(i, **kw)
            return stepper.current()
        first = run(plain, 5)
        same_shifts = diff.noise_source.shifts(5, st.unet)
        a = run(st, 5)                           # the first visit: what today's step draws
        b = run(st, 5, draw=13)                  # the second: other shifts and other noise
        c = run(st, 5, draw=13, shifts=same_shifts)          # other noise alone
        assert all(torch.equal(a[k], first[k]) for k in a)
        assert all(not torch.equal(b[k], a[k]) and not torch.equal(c[k], a[k]) for k in a)
        assert diff.noise_source.shifts(13, st.unet) != same_shifts and not torch.equal(c["video"], b["video"])
        # a jump: both streams move, bitwise the kernel on the state; it replays no U-Net plan (the model outputs stay)
        from mm_diffusion import ops
        st.load(x_T["video"], x_T["audio"])
        st.jump(4, 0x80000001)
        got = st.current()
        for k, tag in (("video", 0), ("audio", 1)):
            want = x_T[k].clone()
            ops.renoise_ctr(want, st.key, st.ids, tag, st.jtab, torch.full((B,), 4, dtype=torch.int64, device=DEV),
                            torch.full((B,), 0x80000001, dtype=torch.int64, device=DEV))
            assert torch.equal(got[k], want) and not torch.equal(want, x_T[k])
        assert st._sets["jump"].graphs is not None and len(st._sets["jump"].graphs) == 2
        plain.close()
        st.close()
    finally:
        diff.noise_source = None
