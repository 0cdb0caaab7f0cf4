"""DDIM inversion on the GPU.  Kernel level: mmd_slerp element by element against the float64 closed form (tests/ddim_invert_ref.py has
the bound), endpoints bitwise, the chord cases, views 4 bytes off a multiple of 16 between intact guards, rows against batch-1 calls,
repeatability, a torch.cuda.graph capture and the refused arguments.  Loop level, on the tiny model with a CounterNoise: ddim_encode_loop
on the graph path bitwise against the eager loop and across lane counts, sample addressability, to_level prefixes, the closed-form
recursion of a zero head, ddim_decode_loop against ddim_sample_loop, ddim_interpolate against its three pieces, and two encode steps of
the 1000-step schedule."""
import numpy as np
import pytest
import torch

import ddim_invert_ref as R
from helpers import flags, synth_sd

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -12345.0


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _same_streams(a, b):
    return all(same(a[k], b[k]) for k in ("video", "audio"))


def _guarded(t, shift=0):
    """a device copy of the numpy array / tensor t with GUARD sentinel floats on either side -> (whole buffer, view of t's shape); shift = 1
    starts the view 4 bytes off a multiple of 16"""
    t = torch.as_tensor(t)
    buf = torch.full((t.numel() + 2 * GUARD + shift,), SENTINEL, device="cuda")
    buf[GUARD + shift:GUARD + shift + t.numel()] = t.reshape(-1).cuda()
    return buf, buf[GUARD + shift:GUARD + shift + t.numel()].view(t.shape)


def _guards_intact(buf, shift=0):
    return bool((buf[:GUARD + shift] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _slerp(a, b, lam, shift=0):
    """ops.slerp on guarded device copies -> the result on the host; asserts inputs and guards are left intact"""
    from mm_diffusion import ops
    (ba, av), (bb, bv) = _guarded(a, shift), _guarded(b, shift)
    bo, ov = _guarded(np.full(a.shape, SENTINEL, np.float32), shift)
    got = ops.slerp(av, bv, torch.from_numpy(np.asarray(lam, np.float32)).cuda(), out=ov)
    assert got is ov
    assert same(av, torch.from_numpy(a)) and same(bv, torch.from_numpy(b))
    assert all(_guards_intact(x, shift) for x in (ba, bb, bo))
    return ov.cpu().numpy()


# ----------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("N", R.NS)
@pytest.mark.parametrize("per", R.PERS)
def test_slerp_is_within_the_float64_bound_and_the_endpoints_are_bitwise(N, per):
    worst = 0.0
    for kind in ("random", "same", "opposite", "zero"):
        a, b, lam = R.slerp_case(N, per, kind)
        assert R.branch_margin_ok(a, b), "the case sits near the 0.9995 switch"
        y, wa, wb = R.slerp64(a, b, lam)
        bound = R.combine_bound(a, b, wa, wb, y)
        for shift in (0, 1):          # 16-byte aligned buffers, and views that start 4 bytes later
            got = _slerp(a, b, lam, shift)
            worst = max(worst, float((np.abs(got.astype(np.float64) - y) / bound).max()))
            assert R.violations(got, y, bound) == 0, (kind, shift)
            if shift == 0:
                first = got
            else:
                assert np.array_equal(got.view(np.int32), first.view(np.int32)), "a row's bits do not depend on where its buffers start"
        if kind in ("same", "opposite"):          # the chord: exactly the fp32 weights 1 - lam, lam
            want = R.emulate(a, b, lam)
            assert np.array_equal(first.view(np.int32), want.view(np.int32)), kind
        for l, want in ((0.0, a), (1.0, b)):
            for shift in (0, 1):
                got = _slerp(a, b, np.full(N, l, np.float32), shift)
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (kind, l, shift)
    print(f"N {N} per {per}: largest error / bound {worst:.3f}")


def test_slerp_zero_row_takes_the_chord_and_rows_differ_in_lam():
    a, b, _ = R.slerp_case(3, 1025, "zero")
    lam = np.array([0.25, 0.0, 1.0], np.float32)
    got = _slerp(a, b, lam)
    assert np.array_equal(got[0].view(np.int32), (np.float32(0.25) * b[0]).view(np.int32))          # 0.75 * 0 + fl(0.25 b)
    assert np.array_equal(got[1].view(np.int32), a[1].view(np.int32)) and np.array_equal(got[2].view(np.int32), b[2].view(np.int32))


@pytest.mark.parametrize("per", R.PERS + (2 * 2048 + 3,))
def test_slerp_rows_do_not_depend_on_the_batch_and_runs_repeat(per):
    from mm_diffusion import ops
    a, b, lam = R.slerp_case(3, per)
    ad, bd, ld = (torch.from_numpy(v).cuda() for v in (a, b, lam))
    full = ops.slerp(ad, bd, ld)
    again = ops.slerp(ad, bd, ld)
    assert same(full, again)
    for n in range(3):
        # the row where it lies in the batch (its own alignment) and as a fresh batch-1 tensor (16-byte aligned)
        assert same(ops.slerp(ad[n:n + 1], bd[n:n + 1], ld[n:n + 1]), full[n:n + 1]), n
        assert same(ops.slerp(ad[n:n + 1].clone(), bd[n:n + 1].clone(), ld[n:n + 1].clone()), full[n:n + 1]), n
    if per > 2048:          # more than one workgroup per row
        from mm_diffusion import _hip
        assert _hip.lib().mmd_slerp_ws_bytes(1, per) > 24
        y, wa, wb = R.slerp64(a, b, lam)
        assert R.violations(full.cpu().numpy(), y, R.combine_bound(a, b, wa, wb, y)) == 0


def test_slerp_at_the_video_latent_size_of_the_base_model():
    from mm_diffusion import ops
    per = 16 * 3 * 64 * 64
    rng = np.random.default_rng(5)
    a, b = (rng.standard_normal((2, per)).astype(np.float32) for _ in range(2))
    lam = np.array([0.3, 0.8], np.float32)
    assert R.branch_margin_ok(a, b)
    got = ops.slerp(torch.from_numpy(a).cuda().view(2, 16, 3, 64, 64), torch.from_numpy(b).cuda().view(2, 16, 3, 64, 64), torch.from_numpy(lam).cuda())
    assert tuple(got.shape) == (2, 16, 3, 64, 64)
    y, wa, wb = R.slerp64(a, b, lam)
    assert R.violations(got.cpu().numpy().reshape(2, per), y, R.combine_bound(a, b, wa, wb, y)) == 0


def test_slerp_inside_a_torch_cuda_graph():
    from mm_diffusion import ops
    a, b, lam = R.slerp_case(3, 1025)
    ad, bd, ld = (torch.from_numpy(v).cuda() for v in (a, b, lam))
    want = ops.slerp(ad, bd, ld)
    sa, sb, sl = torch.zeros_like(ad), torch.zeros_like(bd), torch.zeros_like(ld)
    out, ws = torch.zeros_like(ad), ops.slerp_workspace(3, 1025, "cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.slerp(sa, sb, sl, out=out, ws=ws)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        ops.slerp(sa, sb, sl, out=out, ws=ws)
    sa.copy_(ad), sb.copy_(bd), sl.copy_(ld)
    g.replay()
    torch.cuda.synchronize()
    assert same(out, want)
    sl.copy_(torch.ones_like(ld))
    g.replay()
    torch.cuda.synchronize()
    assert same(out, bd)


def test_slerp_refused_arguments_return_a_code_and_leave_out_unwritten():
    from mm_diffusion import _hip, ops
    lib = _hip.lib()
    a, b, lam = R.slerp_case(2, 1025)
    ad, bd, ld = (torch.from_numpy(v).cuda() for v in (a, b, lam))
    ws = ops.slerp_workspace(2, 1025, "cuda")
    big = torch.full((4 * 1025 + 8,), SENTINEL, device="cuda")
    big[:2 * 1025] = ad.reshape(-1)
    x = big[:2 * 1025].view(2, 1025)
    out = torch.full_like(ad, SENTINEL)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()          # noqa: E731
    keep_big, keep_out = big.clone(), out.clone()

    def refused(word, *args):
        assert lib.mmd_slerp(*args, st) < 0
        assert word in lib.mmd_last_error(), lib.mmd_last_error()
        torch.cuda.synchronize()
        assert same(out, keep_out) and same(big, keep_big)
    refused(b"needs", None, p(bd), p(ld), p(out), p(ws), 2, 1025)
    refused(b"needs", p(ad), None, p(ld), p(out), p(ws), 2, 1025)
    refused(b"needs", p(ad), p(bd), None, p(out), p(ws), 2, 1025)
    refused(b"needs", p(ad), p(bd), p(ld), None, p(ws), 2, 1025)
    refused(b"needs", p(ad), p(bd), p(ld), p(out), None, 2, 1025)
    refused(b"N", p(ad), p(bd), p(ld), p(out), p(ws), 0, 1025)
    refused(b"per", p(ad), p(bd), p(ld), p(out), p(ws), 2, 0)
    refused(b"overlap", p(x), p(bd), p(ld), p(x), p(ws), 2, 1025)                     # out = a
    refused(b"overlap", p(bd), p(x), p(ld), p(x), p(ws), 2, 1025)                     # out = b
    refused(b"overlap", p(x), p(bd), p(ld), p(x) + 4 * (2 * 1025 - 1), p(ws), 2, 1025)      # out starts at a's last element
    with pytest.raises(_hip.MMDError, match="overlap"):
        ops.slerp(x, bd, ld, out=x)
    assert same(big, keep_big)
    # a and b may be one buffer: slerp(a, a) = a by the chord
    got = ops.slerp(ad, ad, ld, out=out)
    want = R.emulate(a, a, lam)
    assert np.array_equal(bits(got), want.view(np.int32))


# ----------------------------------------------------------------------------- the loops
_MODELS = {}
SEED = 4321


def _model(dt, respacing="8", zero_head=False):
    key = (dt, respacing, zero_head)
    if key not in _MODELS:
        from mm_diffusion import logger, multimodal_script_util as msu
        logger.set_quiet(True)
        fl = flags("tiny", timestep_respacing=respacing, use_fp16=(dt == torch.bfloat16))
        model, diff = msu.create_model_and_diffusion(**fl)
        sd = synth_sd("tiny")
        if zero_head:
            for k in sd:
                if k.startswith(("video_out.2.", "audio_out.2.")):
                    sd[k] = torch.zeros_like(sd[k])
        model.load_state_dict(sd)
        model.cuda().eval()
        assert model.dtype == dt and model.shift_source is None
        _MODELS[key] = (fl, model, diff)
    return _MODELS[key]


def _clips(fl, B, seed):
    g = torch.Generator().manual_seed(seed)
    return {"video": (torch.randn(B, *fl["video_size"], generator=g) * 0.5).cuda(), "audio": (torch.randn(B, *fl["audio_size"], generator=g) * 0.5).cuda()}


def _rows(x, sl):
    return {k: v[sl] for k, v in x.items()}


def _seeded(diff, **kw):
    from mm_diffusion.seeded import CounterNoise
    diff.noise_source = CounterNoise(SEED, **kw)
    return diff.noise_source


DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dt", DTYPES)
def test_encode_graph_is_bitwise_eager_across_lanes_and_prefixes(dt):
    fl, model, diff = _model(dt)
    T = diff.num_timesteps
    assert T == 8
    x = _clips(fl, 4, 1)
    try:
        _seeded(diff)
        states = list(diff.ddim_encode_loop_progressive(model, x))          # graph path, default lanes (2 at batch 4)
        assert len(states) == T - 1 and all(torch.isfinite(s[k]).all() for s in states for k in s)
        eager = list(diff.ddim_encode_loop_progressive(model, x, use_graph=False))
        assert len(eager) == T - 1
        for i, (g, e) in enumerate(zip(states, eager)):
            assert _same_streams(g, e), i
        for lanes in (1, 2):
            assert _same_streams(diff.ddim_encode_loop(model, x, lanes=lanes), states[-1]), lanes
        assert _same_streams(diff.ddim_encode_loop(model, x, use_graph=False, lanes=1), states[-1])
        for to_level in (1, 3, T - 1):
            assert _same_streams(diff.ddim_encode_loop(model, x, to_level), states[to_level - 1]), to_level
            assert _same_streams(diff.ddim_encode_loop(model, x, to_level, use_graph=False), states[to_level - 1]), to_level
        assert not same(states[-1]["video"], x["video"]) and not same(states[0]["audio"], states[1]["audio"])
        assert model.shift_source is None
        # the window shifts are the counter's: another seed encodes through other windows
        from mm_diffusion.seeded import CounterNoise
        diff.noise_source = CounterNoise(SEED + 1)
        assert not _same_streams(diff.ddim_encode_loop(model, x), states[-1])
    finally:
        diff.noise_source = None


def test_encode_stepper_owns_no_noise_and_without_a_counter_takes_the_models_shifts():
    import random
    from mm_diffusion._hip import MMDError
    from mm_diffusion.sampler import GraphStepper
    from mm_diffusion.seeded import CounterNoise
    fl, model, diff = _model(torch.float32)
    x = _clips(fl, 2, 7)
    assert diff.noise_source is None
    try:
        for src in (None, CounterNoise(SEED)):
            diff.noise_source = src
            st = GraphStepper(diff, model, 2, "cuda", clip_denoised=False, update="ddim_reverse")
            names = [name for _, _, name, *_ in st.update_plans[0]]
            assert names.count("mmd_ddim_update") == 2 and not any("ctr" in n for n in names), names
            assert st.noise_v is None and st.noise_a is None
            with pytest.raises(MMDError, match="draws nothing"):
                st.set_step(0, noise={"video": x["video"], "audio": x["audio"]})
            st.close()
        diff.noise_source = None
        outs = []
        for use_graph, seed in ((True, 5), (False, 5), (True, 6)):
            rng = random.Random(seed)
            model.shift_source = lambda lo, hi: rng.randint(lo, hi)
            outs.append(diff.ddim_encode_loop(model, x, 3, use_graph=use_graph))
        assert _same_streams(outs[0], outs[1]) and all(torch.isfinite(v).all() for v in outs[0].values())
        assert not _same_streams(outs[0], outs[2]), "the windows are the model's own source's"
    finally:
        model.shift_source = None
        diff.noise_source = None


@pytest.mark.parametrize("dt", DTYPES)
def test_encode_rows_are_addressable(dt):
    fl, model, diff = _model(dt)
    x = _clips(fl, 4, 2)
    try:
        _seeded(diff)
        full = diff.ddim_encode_loop(model, x)
        halves = []
        for f in (0, 2):
            _seeded(diff, first_sample=f)
            halves.append(diff.ddim_encode_loop(model, _rows(x, slice(f, f + 2))))
        for k in ("video", "audio"):
            assert same(torch.cat([h[k] for h in halves]), full[k]), k
        for i in (1, 3):
            _seeded(diff, sample_ids=[i])
            one = diff.ddim_encode_loop(model, _rows(x, slice(i, i + 1)))
            for k in ("video", "audio"):
                assert same(one[k][0], full[k][i]), (i, k)
    finally:
        diff.noise_source = None


@pytest.mark.parametrize("dt", DTYPES)
def test_zero_head_encode_is_the_closed_form_recursion(dt):
    fl, model, diff = _model(dt, zero_head=True)
    T = diff.num_timesteps
    x = _clips(fl, 4, 3)
    try:
        _seeded(diff)
        worst = 0.0
        for to_level in (1, T - 1):
            for use_graph in (True, False):
                got = diff.ddim_encode_loop(model, x, to_level, use_graph=use_graph)
                for k in ("video", "audio"):
                    y, bound = R.zero_head_encode(x[k].cpu().numpy(), diff.alphas_cumprod, to_level)
                    err = np.abs(got[k].cpu().numpy().astype(np.float64) - y)
                    worst = max(worst, float((err / bound).max()))
                    assert R.violations(got[k].cpu().numpy(), y, bound) == 0, (to_level, use_graph, k)
        print(f"{dt}: largest error / carried bound {worst:.3f}")
    finally:
        diff.noise_source = None


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_decode_from_the_top_is_ddim_sample_loop_and_from_level_3_its_tail(dt, eta):
    from mm_diffusion.seeded import TAG_AUDIO, TAG_VIDEO, X_T
    fl, model, diff = _model(dt)
    T = diff.num_timesteps
    shape = {"video": (4, *fl["video_size"]), "audio": (4, *fl["audio_size"])}
    try:
        ctr = _seeded(diff)
        want = list(diff.ddim_sample_loop_progressive(model, shape, eta=eta, device="cuda"))
        assert len(want) == T
        x_T = {"video": ctr.randn(shape["video"], TAG_VIDEO, X_T, "cuda"), "audio": ctr.randn(shape["audio"], TAG_AUDIO, X_T, "cuda")}
        got = list(diff.ddim_decode_loop_progressive(model, x_T, eta=eta))
        assert len(got) == T
        for i, (g, w) in enumerate(zip(got, want)):
            assert _same_streams(g, w), i
        assert _same_streams(diff.ddim_decode_loop(model, x_T, T - 1, eta=eta, use_graph=False), want[-1])
        # the state after step 4 is the level-3 state: decoding it is the last four yields
        tail = list(diff.ddim_decode_loop_progressive(model, want[T - 1 - 4], 3, eta=eta))
        assert len(tail) == 4
        for g, w in zip(tail, want[-4:]):
            assert _same_streams(g, w)
        assert _same_streams(diff.ddim_decode_loop(model, want[-2], 0, eta=eta), want[-1])
        if eta:
            other = list(diff.ddim_sample_loop_progressive(model, shape, eta=0.0, device="cuda"))
            assert not _same_streams(other[-1], want[-1]), "the noise term is there"
    finally:
        diff.noise_source = None


@pytest.mark.parametrize("dt", DTYPES)
def test_interpolate_is_the_composition_of_its_pieces(dt):
    from mm_diffusion import ops
    fl, model, diff = _model(dt)
    a, b = _clips(fl, 4, 4), _clips(fl, 4, 5)
    weights = [0.0, 0.3, 1.0]
    level = 5
    try:
        _seeded(diff)
        got = diff.ddim_interpolate(model, a, b, weights, level)
        assert tuple(got["video"].shape) == (4, 3, *fl["video_size"]) and tuple(got["audio"].shape) == (4, 3, *fl["audio_size"])
        ea, eb = diff.ddim_encode_loop(model, a, level), diff.ddim_encode_loop(model, b, level)
        for j, w in enumerate(weights):
            lam = torch.full((4,), w, device="cuda")
            mid = {k: ops.slerp(ea[k], eb[k], lam) for k in ("video", "audio")}
            want = diff.ddim_decode_loop(model, mid, level, clip_denoised=False)
            for k in ("video", "audio"):
                assert torch.isfinite(want[k]).all()
                assert same(got[k][:, j], want[k]), (w, k)
        # w = 0 and w = 1 are the round trips of a and b
        for j, (x, e) in ((0, (a, ea)), (2, (b, eb))):
            back = diff.ddim_decode_loop(model, e, level, clip_denoised=False)
            assert all(same(got[k][:, j], back[k]) for k in ("video", "audio"))
        assert not same(got["video"][:, 1], got["video"][:, 0])
        # chunks of two pairs through steppers of batch 2, and the eager launches: the same bits
        for kw in (dict(batch=2), dict(use_graph=False), dict(batch=2, lanes=1)):
            o = diff.ddim_interpolate(model, a, b, weights, level, **kw)
            assert _same_streams(o, got), kw
    finally:
        diff.noise_source = None


def test_two_encode_steps_of_the_original_1000_step_schedule():
    fl, model, diff = _model(torch.float32, respacing="")
    assert diff.num_timesteps == 1000
    x = _clips(fl, 2, 6)
    try:
        _seeded(diff)
        got = diff.ddim_encode_loop(model, x, 2)
        eager = diff.ddim_encode_loop(model, x, 2, use_graph=False)
        assert _same_streams(got, eager) and all(torch.isfinite(got[k]).all() for k in got)
        back = diff.ddim_decode_loop(model, got, 2, clip_denoised=False)
        assert all(torch.isfinite(back[k]).all() for k in back)
    finally:
        diff.noise_source = None
