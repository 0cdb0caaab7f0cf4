"""The graph-replayed adaptive DPM-Solver++ on the GPU: mmd_dpm_adapt_open / close / commit bitwise against the launches they replace
(mmd_clamp_scale, mmd_lincomb, copies), the error sums of mmd_dpm_adapt_close against their restated order and a float64 sum,
mmd_dpm_adapt_control against the float64 restatement (tests/dpm_adapt_ref.py), and DPM_Solver.sample_graph_adaptive against a host loop
composed from existing ops, against itself under every execution choice, and against the reference's fixture.  The quad kernels of the
step family (these three and mmd_dpmpp_sde_update / _ctr) on buffers one float off a 16-byte boundary against the aligned run, bit for bit.

Bounds.  Everything compared with existing kernels or with another execution of the same loop is compared bit for bit.  The partial sums
are the restated order's bits, and their fold lies within (elements + chunks) 2^-53 relative of numpy's float64 sum of the same fp32 terms
(a fixed-order fp64 sum of non-negative, exactly represented squares).  The controller's s, h, t, s1 are held to 1e-12 relative: a chain
of about a dozen fp64 operations whose library calls (exp, log, expm1, log1p, sqrt) are good to a few ulps; its fp32 rows to 1 ulp;
decisions, flags, counters and model timesteps exactly.  The loops against the reference's fixture and against the eager solver keep
the rel-L2 of 1e-4 that test_dpm_solver_gpu.py applies to the eager loop on the same fixture."""
import random

import numpy as np
import pytest
import torch

import dpm_adapt_ref as R
from helpers import gold, rel_l2

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- the elementwise kernels
GUARD = 64


def _guarded(t, off=0):
    """a copy of t between NaN guard bands, its first element `off` floats past a 256-byte boundary -> (whole buffer, view of t's shape)"""
    buf = torch.full((t.numel() + 2 * GUARD + 4,), float("nan"), device="cuda")
    buf[GUARD + off:GUARD + off + t.numel()] = t.reshape(-1)
    return buf, buf[GUARD + off:GUARD + off + t.numel()].view(t.shape)


def _guards_intact(buf, t, off):
    return bool(torch.isnan(buf[:GUARD + off]).all()) and bool(torch.isnan(buf[GUARD + off + t.numel():]).all())


# N, F, C, HW: video [3,2,3,5,5] (150 elements: a ragged last quad, samples 1 and 2 start off a quad) and audio [3,1,37]
SHAPES = [(3, 2, 3, 25), (3, 1, 1, 37)]
K = [0, -1, 2]          # sample 1 is finished


def _case(shape, Cm_factor, seed=0):
    N, F, C, HW = shape
    g = torch.Generator().manual_seed(seed)
    t = {name: torch.randn(N, F, C, HW, generator=g).cuda() for name in ("x", "xb", "ms", "lo", "prev")}
    src = (torch.randn(N, F, C * Cm_factor, HW, generator=g) * 1.5).cuda()
    src[:, :, C:] = float("nan")          # the variance channels of a learned-sigma output are never read
    tab = torch.tensor([[1.7, 9.0, 1.0002], [-1.3, 9.0, -0.017], [0.99, 9.0, 2.6], [0.01, 9.0, -2.4], [0.7, 9.0, 0.81], [0.3, 9.0, -0.5]])
    return t, src, tab.cuda(), torch.tensor(K, dtype=torch.int64, device="cuda")


def _rowwise(fn, N):
    """cat of fn(n) [1, ...] over the samples: the eager launches take one host scalar per call"""
    return torch.cat([fn(n) for n in range(N)])


def _model_value(shape, t, src, tab, form, s, max_val):
    from mm_diffusion import ops
    N, F, C, HW = shape
    eps = src[:, :, :C].contiguous()
    if form == 1:
        return _rowwise(lambda n: ops.lincomb(t["x"][n:n + 1], float(tab[0, n]), eps[n:n + 1], float(tab[1, n])), N)
    return ops.clamp_scale_(eps.clone(), s, max_val) if s is not None else eps


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("Cm_factor", [1, 2])
@pytest.mark.parametrize("off", [0, 1])
def test_open_close_commit_are_bitwise_the_launches_they_replace(shape, Cm_factor, off):
    from mm_diffusion import ops
    N, F, C, HW = shape
    t, src, tab, k = _case(shape, Cm_factor)
    params = ops.dpm_adapt_params("cuda", atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, h_init=0.05, t_T=1.0, t_0=1e-3)
    s_all = torch.tensor([0.4, 1.3, 2.9], device="cuda")
    for form, s in ((0, None), (0, s_all), (1, None)):
        m = _model_value(shape, t, src, tab, form, s, 1.5)
        live = [n for n in range(N) if K[n] >= 0]
        # ---- open
        g = {name: _guarded(t[name], off) for name in ("x", "xb", "ms", "lo")}
        gs = _guarded(src, off)
        ops.dpm_adapt_open(g["x"][1], gs[1], g["xb"][1], g["ms"][1], g["lo"][1], tab, k, F, C, C * Cm_factor, HW, form=form, s=s, max_val=1.5)
        assert all(_guards_intact(b, t[name], off) for name, (b, _) in g.items()) and same(gs[1][:, :, :C], src[:, :, :C])
        want = {"xb": t["x"], "ms": m,
                "lo": _rowwise(lambda n: ops.lincomb(t["x"][n:n + 1], float(tab[2, n]), m[n:n + 1], float(tab[3, n])), N),
                "x": _rowwise(lambda n: ops.lincomb(t["x"][n:n + 1], float(tab[4, n]), m[n:n + 1], float(tab[5, n])), N)}
        for name in want:
            for n in range(N):
                ref = want[name][n] if n in live else t[name][n]      # the finished sample is untouched
                assert same(g[name][1][n], ref), ("open", form, s is not None, name, n)
        # ---- close: tab rows 2-4 = c0, c1, c2; x holds x_s1 (read by form 1 only)
        g = {name: _guarded(t[name], off) for name in ("x", "xb", "ms", "lo", "prev")}
        chunks = ops.dpm_adapt_chunks(F * C * HW)
        partial = torch.full((N, chunks), -7.0, dtype=torch.float64, device="cuda")
        ops.dpm_adapt_close(g["x"][1], gs[1], g["xb"][1], g["ms"][1], g["lo"][1], g["prev"][1], tab, k, params, partial, F, C, C * Cm_factor, HW,
                            form=form, s=s, max_val=1.5)
        assert all(_guards_intact(b, t[name], off) for name, (b, _) in g.items())
        hi = _rowwise(lambda n: ops.lincomb(t["xb"][n:n + 1], float(tab[2, n]), t["ms"][n:n + 1], float(tab[3, n]), m[n:n + 1], float(tab[4, n])), N)
        for name in ("xb", "ms", "lo", "prev"):
            assert same(g[name][1], t[name]), ("close reads", name)
        for n in range(N):
            if n in live:
                assert same(g["x"][1][n], hi[n]), ("close", form, s is not None, n)
                e = R.error_terms(hi[n].cpu().numpy(), t["lo"][n].cpu().numpy(), t["prev"][n].cpu().numpy(), 0.0078, 0.05)
                assert R.compare_partials(partial[n].cpu().numpy(), e) == [], ("partial", n)
            else:
                assert same(g["x"][1][n], t["x"][n]) and bool((partial[n] == -7.0).all())
    # ---- commit: accept, idle, reject
    cnt = torch.zeros(N, 4, dtype=torch.int32, device="cuda")
    cnt[:, ops.ADAPT_C["flag"]] = torch.tensor([ops.ADAPT_FLAG_ACCEPT, ops.ADAPT_FLAG_IDLE, ops.ADAPT_FLAG_REJECT], dtype=torch.int32)
    g = {name: _guarded(t[name], off) for name in ("x", "xb", "prev", "lo")}
    ops.dpm_adapt_commit(g["x"][1], g["xb"][1], g["prev"][1], g["lo"][1], cnt)
    assert all(_guards_intact(b, t[name], off) for name, (b, _) in g.items())
    assert same(g["xb"][1], t["xb"]) and same(g["lo"][1], t["lo"])
    for n, (wx, wp) in enumerate((("x", "lo"), ("x", "prev"), ("xb", "prev"))):
        got = (g["x"][1][n].cpu().numpy(), g["prev"][1][n].cpu().numpy())
        assert R.compare_commit(got, (t[wx][n].cpu().numpy(), t[wp][n].cpu().numpy())) == [], n


# The quad kernels of the step family take their 16-byte path by the alignment bits of their buffers (one helper computes them for every
# entry point).  Bits must not depend on them: the shape of tests/dpm_sde_ref.py, 6147 elements a sample (ragged last quad, quads that
# straddle a (frame, channel) row, samples 1 and 2 off a quad), with every state buffer one float into its allocation, and with the source
# of the model value alone there, against the run on aligned buffers.
ALIGN_ENTRIES = ["sde_update", "sde_update_ctr", "open_form0", "open_form1", "close_form0", "close_form1", "commit"]


@pytest.mark.parametrize("entry", ALIGN_ENTRIES)
def test_buffers_one_float_off_16_bytes_give_the_aligned_bits(entry):
    import dpm_sde_ref as S
    from mm_diffusion import ops
    N, F, C, HW = shape = (S.N, S.F, S.C, S.HW)
    params = ops.dpm_adapt_params("cuda", **PARAMS)
    key = torch.from_numpy(np.array([S.SEED & 0xFFFFFFFF, S.SEED >> 32], dtype=np.uint32).view(np.int32)).cuda()
    ids = torch.tensor(list(S.IDS), dtype=torch.int64, device="cuda")
    s_all = torch.from_numpy(S.S_VALUES).cuda()
    for cmf in (1, 2):
        t, src, tab, _ = _case(shape, cmf, seed=5)
        sde = S.make_case(cmf, True)
        sde_tab, cz = torch.from_numpy(sde["tab"]).cuda(), torch.from_numpy(sde["cz"]).cuda()
        geom = (F, C, C * cmf, HW)
        k = torch.tensor([2, 0, 1], dtype=torch.int64, device="cuda")
        form, s = (1, None) if entry.endswith("form1") else (0, s_all)
        # entry -> (the state buffers, the runs' launches: each takes the views v and the source's view, and returns its other outputs)
        if entry.startswith("sde"):
            ctr = entry == "sde_update_ctr"
            names = ("x", "ms") if ctr else ("x", "ms", "lo")          # x, M1 and, in the memory form, the noise

            def launch(v, sv):
                for rows in S.K_CASES[4:]:          # rows of every kind, over two launches
                    noise = dict(ctr=(key, ids, 1)) if ctr else dict(noise=v["lo"])
                    ops.dpmpp_sde_update(v["x"], sv, v["ms"], sde_tab, cz, torch.tensor(rows, dtype=torch.int64, device="cuda"), *geom, s=s_all,
                                         max_val=S.MAX_VAL, **noise)
                return {}
        elif entry.startswith("open"):
            names = ("x", "xb", "ms", "lo")

            def launch(v, sv):
                ops.dpm_adapt_open(v["x"], sv, v["xb"], v["ms"], v["lo"], tab, k, *geom, form=form, s=s, max_val=S.MAX_VAL)
                return {}
        elif entry.startswith("close"):
            names = ("x", "xb", "ms", "lo", "prev")

            def launch(v, sv):
                partial = torch.full((N, ops.dpm_adapt_chunks(F * C * HW)), -7.0, dtype=torch.float64, device="cuda")
                ops.dpm_adapt_close(v["x"], sv, v["xb"], v["ms"], v["lo"], v["prev"], tab, k, params, partial, *geom, form=form, s=s, max_val=S.MAX_VAL)
                return {"partial": partial}
        else:
            names = ("x", "xb", "prev", "lo")

            def launch(v, sv):
                cnt = torch.zeros(N, 4, dtype=torch.int32, device="cuda")
                for flags in ((ops.ADAPT_FLAG_ACCEPT, ops.ADAPT_FLAG_IDLE, ops.ADAPT_FLAG_REJECT), (ops.ADAPT_FLAG_REJECT, ops.ADAPT_FLAG_ACCEPT, ops.ADAPT_FLAG_ACCEPT)):
                    cnt[:, ops.ADAPT_C["flag"]] = torch.tensor(flags, dtype=torch.int32)
                    ops.dpm_adapt_commit(v["x"], v["xb"], v["prev"], v["lo"], cnt)
                return {}

        def run(off, off_src):
            g = {name: _guarded(t[name], off) for name in names}
            gs = _guarded(src, off_src)
            assert all(v.data_ptr() % 16 == 4 * off for _, v in g.values()) and gs[1].data_ptr() % 16 == 4 * off_src
            out = launch({name: v for name, (_, v) in g.items()}, gs[1])
            torch.cuda.synchronize()
            assert all(_guards_intact(b, t[name], off) for name, (b, _) in g.items()), (entry, cmf, off, off_src, "a float outside a view was written")
            assert _guards_intact(gs[0], src, off_src) and same(gs[1], src), (entry, cmf, off, off_src, "the source was written")
            return dict({name: v.clone() for name, (_, v) in g.items()}, **out)
        want = run(0, 0)
        assert any(not same(want[name], t[name]) for name in names), "the aligned run wrote something"
        for off, off_src in ((1, 1), (0, 1)) if entry != "commit" else ((1, 0),):          # commit has no source
            got = run(off, off_src)
            for name in want:
                assert same(got[name], want[name]), (entry, cmf, off, off_src, name)


def test_refused_arguments_write_nothing():
    from mm_diffusion import _hip, ops
    shape = SHAPES[0]
    N, F, C, HW = shape
    t, src, tab, k = _case(shape, 1)
    lib, st = _hip.lib(), _hip.stream_handle()
    keep = {name: v.clone() for name, v in t.items()}
    p = {name: v.data_ptr() for name, v in t.items()}
    params = ops.dpm_adapt_params("cuda", atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, h_init=0.05, t_T=1.0, t_0=1e-3)
    partial = torch.zeros(N, 1, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(N, 4, dtype=torch.int32, device="cuda")
    geo = (N, F, C, C, HW)
    assert lib.mmd_dpm_adapt_open(p["x"], src.data_ptr(), 0, p["x"] + 8, p["ms"], p["lo"], None, 1.0, tab.data_ptr(), k.data_ptr(), 3, *geo, st) < 0
    assert lib.mmd_dpm_adapt_open(p["x"], None, 0, p["xb"], p["ms"], p["lo"], None, 1.0, tab.data_ptr(), k.data_ptr(), 3, *geo, st) < 0
    assert lib.mmd_dpm_adapt_open(p["x"], src.data_ptr(), 0, p["xb"], p["ms"], p["lo"], None, 1.0, tab.data_ptr(), k.data_ptr(), 3, 0, F, C, C, HW, st) < 0
    assert lib.mmd_dpm_adapt_close(p["x"], src.data_ptr(), 0, p["xb"], p["ms"], p["lo"], p["lo"], None, 1.0, tab.data_ptr(), k.data_ptr(), 3,
                                   params.data_ptr(), partial.data_ptr(), *geo, st) < 0
    assert lib.mmd_dpm_adapt_close(p["x"], src.data_ptr(), 0, p["xb"], p["ms"], p["lo"], p["prev"], None, 1.0, tab.data_ptr(), k.data_ptr(), 3,
                                   None, partial.data_ptr(), *geo, st) < 0
    assert lib.mmd_dpm_adapt_commit(p["x"], p["xb"], p["x"], p["lo"], cnt.data_ptr(), N, F * C * HW, st) < 0
    assert lib.mmd_dpm_adapt_commit(p["x"], p["xb"], p["prev"], p["lo"], cnt.data_ptr(), -1, F * C * HW, st) < 0
    torch.cuda.synchronize()
    assert all(same(t[name], keep[name]) for name in t) and float(partial.abs().sum()) == 0.0
    with pytest.raises(_hip.MMDError, match="form"):
        ops.dpm_adapt_open(t["x"], src, t["xb"], t["ms"], t["lo"], tab, k, F, C, C, HW, form=1, s=torch.ones(N, device="cuda"))


@pytest.mark.parametrize("per", [1, 150, R.CHUNK - 1, R.CHUNK + 1, 3 * R.CHUNK + 5])
def test_error_partials(per):
    """The restated order bit for bit and the float64 bound (R.compare_partials), two calls with the same bits, and row n alone =
    row n inside a batch, at another address."""
    from mm_diffusion import ops
    N = 3
    g = torch.Generator().manual_seed(per)
    xb, ms, lo, prev, src = (torch.randn(N, 1, 1, per, generator=g).cuda() for _ in range(5))
    tab = torch.tensor([[1.0] * N, [0.0] * N, [0.9, 0.8, 0.7], [0.0] * N, [0.11, 0.21, 0.31], [0.0] * N]).cuda()
    params = ops.dpm_adapt_params("cuda", atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, h_init=0.05, t_T=1.0, t_0=1e-3)
    chunks = ops.dpm_adapt_chunks(per)

    def run(sl, rows):
        n = sl.stop - sl.start
        x = torch.zeros(n, 1, 1, per, device="cuda")
        partial = torch.zeros(n, chunks, dtype=torch.float64, device="cuda")
        k = torch.tensor(rows, dtype=torch.int64, device="cuda")
        ops.dpm_adapt_close(x, src[sl].clone(), xb[sl].clone(), ms[sl].clone(), lo[sl].clone(), prev[sl].clone(), tab, k, params, partial, 1, 1, 1, per)
        return x, partial
    x, partial = run(slice(0, N), [0, 1, 2])
    x2, partial2 = run(slice(0, N), [0, 1, 2])
    assert same(x, x2) and np.array_equal(partial.cpu().numpy().view(np.int64), partial2.cpu().numpy().view(np.int64))
    worst = 0.0
    for n in range(N):
        e = R.error_terms(x[n].cpu().numpy(), lo[n].cpu().numpy(), prev[n].cpu().numpy(), 0.0078, 0.05)
        assert R.compare_partials(partial[n].cpu().numpy(), e) == [], n
        ref = float(np.sum(e.astype(np.float64) ** 2))
        worst = max(worst, abs(float(R.fold(partial[n].cpu().numpy())) - ref) / ref / ((per + chunks) * 2.0 ** -53))
        xa, pa = run(slice(n, n + 1), [n])
        assert same(xa[0], x[n]) and np.array_equal(pa[0].cpu().numpy().view(np.int64), partial[n].cpu().numpy().view(np.int64)), n
    print(f"per {per}: worst |fold - fp64 sum| = {worst:.3f} of the bound")


# ----------------------------------------------------------------------------- the controller
PARAMS = dict(atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, h_init=0.05, t_T=1.0, t_0=1e-3)


def _log_alpha():
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64)
    return (0.5 * torch.log(torch.cumprod(1 - betas, 0).float())).double()


def _boundary_distance(S, t):
    v = (np.float64(np.float32(t)) - 1.0 / S.T) * S.T
    return abs(v - np.round(v))


def _draw_states(S, p, n, seed, chunks=(2, 1), pers=(5000, 37)):
    """n random mid-loop states with the partial sums that end their trial, drawn by rejection: the restatement's own E at least 1e-6
    from 1 and its next model times at least 1e-6 from an integer boundary.  Every third state sits near t_0, where the cap of h binds
    and steps finish."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        s = float(rng.uniform(1.2e-3, 1.0)) if i % 3 else float(rng.uniform(1.0e-3 + 2e-5, 4e-3))
        st = R.init_state(S, dict(p, t_T=s))
        st["h"] = float(min(rng.uniform(0.02, 1.2), st["lam_0"] - st["lam_s"]))
        st["rows"] = R.rows(S, st["s"], st["h"], st["lam_s"])
        st["attempts"], st["accepted"] = int(rng.integers(0, 50)), int(rng.integers(0, 20))
        target = float(np.exp(rng.uniform(-2.5, 1.0)))
        parts = [rng.dirichlet(np.ones(c)) * target ** 2 * per * (1.0 if j == 0 else rng.uniform(0.2, 1.0)) for j, (c, per) in enumerate(zip(chunks, pers))]
        E = R.error_norm([R.fold(q) for q in parts], pers)
        want = R.control(S, p, st, E)
        if abs(E - 1.0) < 1e-6:
            continue
        if not want["done"] and min(_boundary_distance(S, want["s"]), _boundary_distance(S, want["rows"]["s1"])) < 1e-6:
            continue
        out.append((st, parts, E, want))
    return out


def _load_block(blk, states):
    from mm_diffusion import ops
    N = len(states)
    state = np.zeros((N, ops.ADAPT_STATE_WORDS))
    cnt = np.zeros((N, 4), dtype=np.int32)
    ftab = np.zeros((16, N), dtype=np.float32)
    itab = np.zeros((3, N), dtype=np.int64)
    for n, st in enumerate(states):
        for name in ("s", "h", "lam_s", "lam_0"):
            state[n, ops.ADAPT_S[name]] = st[name]
        state[n, ops.ADAPT_S["t"]], state[n, ops.ADAPT_S["s1"]] = st["rows"]["t"], st["rows"]["s1"]
        cnt[n] = (st["attempts"], st["accepted"], st["flag"], int(st["done"]))
        ftab[:, n] = st["rows"]["ftab"]
        itab[:, n] = (-1 if st["done"] else n, st["rows"]["tm_s"], st["rows"]["tm_s1"])
    blk.state.copy_(torch.from_numpy(state))
    blk.cnt.copy_(torch.from_numpy(cnt))
    blk.ftab.copy_(torch.from_numpy(ftab))
    blk.itab.copy_(torch.from_numpy(itab))
    blk.status.zero_()


def _read_block(blk, n):
    from mm_diffusion import ops
    state, cnt, ftab, itab = blk.state[n].cpu().numpy(), blk.cnt[n].cpu().numpy(), blk.ftab[:, n].cpu().numpy(), blk.itab[:, n].cpu().numpy()
    return {"s": state[ops.ADAPT_S["s"]], "h": state[ops.ADAPT_S["h"]], "lam_s": state[ops.ADAPT_S["lam_s"]], "E": state[ops.ADAPT_S["E"]],
            "attempts": cnt[0], "accepted": cnt[1], "flag": cnt[2], "done": cnt[3], "fault": bool(np.isnan(state[ops.ADAPT_S["E"]])), "k": int(itab[0]),
            "rows": {"t": state[ops.ADAPT_S["t"]], "s1": state[ops.ADAPT_S["s1"]], "tm_s": itab[1], "tm_s1": itab[2], "ftab": ftab}}


def test_controller_matches_the_float64_restatement():
    from mm_diffusion import ops
    la = _log_alpha()
    S, p = R.Schedule(la.numpy()), PARAMS
    params, la_dev = ops.dpm_adapt_params("cuda", **p), la.cuda()
    # ---- init
    blk = ops.AdaptBlock(3, "cuda")
    ops.dpm_adapt_control(blk, params, la_dev, init=True)
    want = R.init_state(S, p)
    for n in range(3):
        got = _read_block(blk, n)
        bad, _ = R.compare_control(got, want)
        assert bad == [] and got["k"] == n and got["flag"] == R.IDLE, bad
    assert blk.status.tolist() == [3, 0]
    # ---- 200 random states, every sample its own decision
    cases = _draw_states(S, p, 200, 11)
    blk = ops.AdaptBlock(len(cases), "cuda")
    _load_block(blk, [c[0] for c in cases])
    pv = torch.from_numpy(np.stack([c[1][0] for c in cases])).cuda()
    pa = torch.from_numpy(np.stack([c[1][1] for c in cases])).cuda()
    ops.dpm_adapt_control(blk, params, la_dev, [(pv, 5000), (pa, 37)])
    worst, ndone, nacc = 0.0, 0, 0
    for n, (st, parts, E, want) in enumerate(cases):
        got = _read_block(blk, n)
        bad, dev = R.compare_control(got, want)
        assert bad == [], (n, bad)
        assert float(got["E"]) == E and got["k"] == (-1 if want["done"] else n), n
        worst, ndone, nacc = max(worst, dev), ndone + bool(want["done"]), nacc + (want["flag"] == R.ACCEPT)
    print(f"controller: largest relative deviation of s, h, lambda_s, t, s1 = {worst:.3e} (allowance 1e-12); {nacc} accepted, {ndone} done of {len(cases)}")
    assert 20 < nacc < 180 and ndone > 0
    assert blk.status.tolist() == [len(cases) - ndone, 0]
    # a second trial's end: the finished samples idle and nothing of theirs moves
    before = {name: getattr(blk, name).clone() for name in ("state", "cnt", "ftab", "itab")}
    ops.dpm_adapt_control(blk, params, la_dev, [(pv, 5000), (pa, 37)])
    for n, (_, _, _, want) in enumerate(cases):
        if want["done"]:
            assert int(blk.cnt[n, 2]) == R.IDLE and int(blk.itab[0, n]) == -1
            assert torch.equal(blk.state[n], before["state"][n]) and torch.equal(blk.ftab[:, n], before["ftab"][:, n])


def test_controller_batch_rule_fault_and_finish():
    from mm_diffusion import ops
    la = _log_alpha()
    S, p = R.Schedule(la.numpy()), PARAMS
    params, la_dev = ops.dpm_adapt_params("cuda", **p), la.cuda()
    # ---- batch: one shared state, the decision is the maximum's
    st = R.init_state(S, dict(p, t_T=0.5))
    N = 5
    for Es in ([0.3, 0.9, 0.5, 0.2, 0.7], [0.3, 0.9, 1.4, 0.2, 0.7]):
        blk = ops.AdaptBlock(N, "cuda")
        _load_block(blk, [st] * N)
        pv = torch.tensor([[e * e * 100.0] for e in Es], dtype=torch.float64, device="cuda")
        ops.dpm_adapt_control(blk, params, la_dev, [(pv, 100)], batch=True)
        E = max(R.error_norm([e * e * 100.0], [100]) for e in Es)
        want = R.control(S, p, st, E)
        for n in range(N):
            got = _read_block(blk, n)
            assert R.compare_control(got, want)[0] == [] and float(got["E"]) == E, n
        assert want["flag"] == (R.ACCEPT if max(Es) <= 1 else R.REJECT) and blk.status.tolist() == [N, 0]
    # ---- an infinite sum: the fault bit, that sample's state as it was, the others go on; the bit stays until the next init
    blk = ops.AdaptBlock(3, "cuda")
    _load_block(blk, [st] * 3)
    pv = torch.tensor([[25.0], [float("inf")], [400.0]], dtype=torch.float64, device="cuda")
    before = blk.state[1].clone(), blk.cnt[1].clone(), blk.ftab[:, 1].clone()
    ops.dpm_adapt_control(blk, params, la_dev, [(pv, 100)])
    assert blk.status.tolist() == [3, 1]
    assert torch.equal(blk.state[1][:5], before[0][:5]) and blk.cnt[1].tolist() == [0, 0, R.REJECT, 0] and torch.equal(blk.ftab[:, 1], before[2])
    for n, e2 in ((0, 25.0), (2, 400.0)):
        assert R.compare_control(_read_block(blk, n), R.control(S, p, st, R.error_norm([e2], [100])))[0] == []
    pv[1] = 25.0
    ops.dpm_adapt_control(blk, params, la_dev, [(pv, 100)])
    assert blk.status.tolist() == [3, 1]
    ops.dpm_adapt_control(blk, params, la_dev, init=True)
    assert blk.status.tolist() == [3, 0]
    # the batch rule faults as a whole
    blk = ops.AdaptBlock(3, "cuda")
    _load_block(blk, [st] * 3)
    pv[1] = float("nan")
    ops.dpm_adapt_control(blk, params, la_dev, [(pv, 100)], batch=True)
    assert blk.status.tolist() == [3, 1] and blk.cnt[:, 2].tolist() == [R.REJECT] * 3 and blk.cnt[:, 0].tolist() == [0, 0, 0]
    # ---- done at t_0: a step whose h is the whole rest finishes when it is accepted
    last = R.init_state(S, dict(p, t_T=0.004))
    last["h"] = last["lam_0"] - last["lam_s"]
    last["rows"] = R.rows(S, last["s"], last["h"], last["lam_s"])
    blk = ops.AdaptBlock(2, "cuda")
    _load_block(blk, [last, last])
    pv = torch.tensor([[25.0], [400.0]], dtype=torch.float64, device="cuda")
    ops.dpm_adapt_control(blk, params, la_dev, [(pv, 100)])
    got = [_read_block(blk, n) for n in range(2)]
    assert got[0]["done"] == 1 and got[0]["k"] == -1 and abs(got[0]["s"] - p["t_0"]) <= 1e-12 and got[0]["flag"] == R.ACCEPT
    assert got[1]["done"] == 0 and got[1]["k"] == 1 and got[1]["flag"] == R.REJECT
    assert blk.status.tolist() == [1, 0]
    for n, e2 in enumerate((25.0, 400.0)):
        assert R.compare_control(got[n], R.control(S, p, last, R.error_norm([e2], [100])))[0] == []
    # a loop that starts at its end is done by init
    blk = ops.AdaptBlock(1, "cuda")
    ops.dpm_adapt_control(blk, ops.dpm_adapt_params("cuda", **dict(p, t_T=1e-3)), la_dev, init=True)
    assert blk.status.tolist() == [0, 0] and int(blk.itab[0, 0]) == -1


# ----------------------------------------------------------------------------- the loop
_MODELS = {}
LOOSE = dict(atol=0.05, rtol=0.1)          # fewer trial steps than the defaults: the loops that only compare executions


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


def _clone(x):
    return {k: v.clone() for k, v in x.items()}


def _same_stats(a, b):
    """the per-sample statistics (the trial steps replayed round up to a multiple of poll)"""
    return all(torch.equal(a[k], b[k]) for k in ("attempts", "accepted", "nfe"))


def test_trace_is_the_host_composition():
    """With the device's coefficients and decisions of every trial step (stepper.trace()), a host loop of existing ops - the model call,
    lincomb for the data prediction, abs_quantile, clamp_scale_, lincomb for the three updates - gives x and PREV bit for bit after every
    trial step, and its own mmd_dpm_err value gives the device's E."""
    from mm_diffusion import ops
    fl, model, solver = _solver()
    B = 2
    x_T = _x_T(fl, B, 31)
    try:
        _replay(model, 5)
        out, stats = solver.sample_graph_adaptive(_clone(x_T), poll=1, return_stats=True, **LOOSE)
        stepper = solver._stepper[1]
        # the same loop again by hand, reading the controller's block around every trial step
        _replay(model, 5)
        stepper.load(x_T["video"], x_T["audio"])
        stepper.start()
        log = []
        for _ in range(stats["trials"]):
            before = stepper.trace()
            stepper.trial()
            log.append((before, stepper.trace(), _clone(stepper.current()), {b["stream"]: b["prev"].clone() for b in stepper._bufs}))
        assert stepper.poll() == (0, False)
        assert same(stepper.current()["video"], out["video"]) and same(stepper.current()["audio"], out["audio"])
        # the host loop
        _replay(model, 5)
        x, prev = _clone(x_T), _clone(x_T)
        worst = 0.0

        def predict(x, tm, cx, ce):
            with torch.no_grad():
                v, a = model(x["video"], x["audio"], tm.to(torch.int).cuda())
            eps, m = {"video": v[:, :, :3].float().contiguous(), "audio": a[:, :1].float().contiguous()}, {}
            for k in x:
                x0 = _rowwise(lambda n: ops.lincomb(x[k][n:n + 1], float(cx[n]), eps[k][n:n + 1], float(ce[n])), B)
                m[k] = ops.clamp_scale_(x0, ops.abs_quantile(x0, 0.995), 1.0)
            return m
        for before, after, x_dev, prev_dev in log:
            f, it = before["ftab"], before["itab"]
            live = [n for n in range(B) if int(it[0, n]) >= 0]
            m0 = predict(x, it[1], f[0], f[1])
            lo = {k: _rowwise(lambda n: ops.lincomb(x[k][n:n + 1], float(f[2, n]), m0[k][n:n + 1], float(f[3, n])), B) for k in x}
            x1 = {k: _rowwise(lambda n: ops.lincomb(x[k][n:n + 1], float(f[4, n]), m0[k][n:n + 1], float(f[5, n])) if n in live else x[k][n:n + 1], B)
                  for k in x}
            m1 = predict(x1, it[2], f[6], f[7])
            hi = {k: _rowwise(lambda n: ops.lincomb(x[k][n:n + 1], float(f[8, n]), m0[k][n:n + 1], float(f[9, n]), m1[k][n:n + 1], float(f[10, n])), B)
                  for k in x}
            acc = torch.zeros(2 * B, dtype=torch.float64, device="cuda")
            for i, k in enumerate(x):
                ops.dpm_err(hi[k], lo[k], prev[k], LOOSE["atol"], LOOSE["rtol"], acc[i * B:(i + 1) * B])
            per = torch.tensor([x[k][0].numel() for k in x for _ in range(B)], dtype=torch.float64, device="cuda")
            E = torch.sqrt(acc / per).float().reshape(2, B).max(dim=0).values.cpu()
            for n in range(B):
                flag = int(after["cnt"][n, ops.ADAPT_C["flag"]])
                if n not in live:
                    assert flag == ops.ADAPT_FLAG_IDLE
                    continue
                E_dev = float(after["state"][n, ops.ADAPT_S["E"]])
                worst = max(worst, abs(float(E[n]) - E_dev) / E_dev)
                assert flag == (ops.ADAPT_FLAG_ACCEPT if E_dev <= 1.0 else ops.ADAPT_FLAG_REJECT)
                for k in x:
                    if flag == ops.ADAPT_FLAG_ACCEPT:
                        x[k][n], prev[k][n] = hi[k][n], lo[k][n]
            for k in x:
                assert same(x[k], x_dev[k]) and same(prev[k], prev_dev[k]), k
        print(f"trace: {len(log)} trial steps, largest relative distance of the host's mmd_dpm_err E from the device's = {worst:.3e}")
        assert worst <= 1e-12
    finally:
        model.shift_source = None


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_graph_eager_poll_and_lanes_agree(dt):
    fl, model, solver = _solver(dt)
    x_T = _x_T(fl, 4, 5)
    runs = []
    cases = [dict(lanes=1), dict(lanes=1, use_graph=False), dict(lanes=2, poll=3)]
    if dt == torch.float32:
        cases += [dict(lanes=1, poll=1), dict(lanes=1, poll=3), dict(lanes=1, poll=8), dict(lanes=2, poll=3, use_graph=False)]
    try:
        for kw in cases:
            _replay(model, 9)
            nfe = solver.nfe
            out, stats = solver.sample_graph_adaptive(_clone(x_T), return_stats=True, **dict(LOOSE, **kw))
            assert solver.nfe - nfe == 2 * stats["trials"] and stats["trials"] >= int(stats["attempts"].max())
            assert stats["host_reads"] == -(-stats["trials"] // kw.get("poll", 4))
            runs.append((out, stats))
        names = [name for _, _, name, *_ in solver._stepper[1]._sets["stage"].plans[0]]
        per_stream = ["mmd_dpmpp_x0", "mmd_dpmpp_select", "mmd_dpm_adapt_close"]
        assert names == per_stream * 2 + ["sync", "mmd_dpm_adapt_control", "mmd_dpm_adapt_commit", "mmd_dpm_adapt_commit"]
    finally:
        model.shift_source = None
    out0, st0 = runs[0]
    assert torch.isfinite(out0["video"]).all() and torch.isfinite(out0["audio"]).all()
    print(f"{dt}: attempts {st0['attempts'].tolist()} accepted {st0['accepted'].tolist()} trials {st0['trials']}")
    for out, st in runs[1:]:
        assert same(out["video"], out0["video"]) and same(out["audio"], out0["audio"])
        assert _same_stats(st, st0)


def test_counter_noise_samples_are_addressable():
    from mm_diffusion.seeded import CounterNoise
    fl, model, solver = _solver()
    assert model.shift_source is None
    shape = lambda B: {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}      # noqa: E731
    full, stats = solver.sample_graph_adaptive(shape=shape(3), noise_source=CounterNoise(1234), return_stats=True, **LOOSE)
    for i in range(3):      # batch 1 is accepted; per-sample statistics are that sample's in any batch
        one, st1 = solver.sample_graph_adaptive(shape=shape(1), noise_source=CounterNoise(1234, sample_ids=[i]), return_stats=True, **LOOSE)
        for k in ("video", "audio"):
            assert same(one[k][0], full[k][i]), (i, k)
        assert int(st1["attempts"][0]) == int(stats["attempts"][i]) and int(st1["accepted"][0]) == int(stats["accepted"][i])
    print(f"counter noise: attempts {stats['attempts'].tolist()} accepted {stats['accepted'].tolist()}")
    other = solver.sample_graph_adaptive(shape=shape(1), noise_source=CounterNoise(1235, sample_ids=[0]), **LOOSE)
    assert not same(other["video"][0], full["video"][0])


def test_kept_stepper_serves_other_tolerances_on_the_same_graphs():
    from mm_diffusion.sampler import DpmAdaptiveStepper
    fl, model, solver = _solver()
    x_T = _x_T(fl, 2, 7)
    try:
        _replay(model, 13)
        solver.sample_graph_adaptive(_clone(x_T), **LOOSE)
        kept = solver._stepper[1]
        graphs = {name: list(ps.graphs) for name, ps in kept._sets.items()}
        assert isinstance(kept, DpmAdaptiveStepper) and all(g is not None for gs in graphs.values() for g in gs)
        _replay(model, 13)
        got, st = solver.sample_graph_adaptive(_clone(x_T), atol=0.02, rtol=0.08, theta=0.8, h_init=0.1, return_stats=True)
        assert solver._stepper[1] is kept and {name: list(ps.graphs) for name, ps in kept._sets.items()} == graphs
        _replay(model, 13)      # a new solver builds a new stepper and captures anew
        fresh, st2 = _solver()[2].sample_graph_adaptive(_clone(x_T), atol=0.02, rtol=0.08, theta=0.8, h_init=0.1, return_stats=True)
        for k in ("video", "audio"):
            assert same(got[k], fresh[k]), k
        assert _same_stats(st, st2)
    finally:
        model.shift_source = None


def test_reference_fixture_and_the_eager_solver():
    """control="batch", poll=1: the reference's own 68 evaluations (34 trial steps, 24 accepted) on its x_T and shifts, its samples to
    1e-4, and the eager sample(method="adaptive") - fp32 coefficients, a host decision per trial - to the same count and bound."""
    g = gold("tiny_dpmpp_adaptive2")
    fl, model, solver = _solver()
    B = int(g["B"])
    torch.manual_seed(int(g["seed"]))
    x_T = {"video": torch.randn(B, *fl["video_size"]).cuda(), "audio": torch.randn(B, *fl["audio_size"]).cuda()}
    try:
        it = iter(int(s) for s in g["shifts"])
        model.shift_source = lambda lo, hi: next(it)
        out, stats = solver.sample_graph_adaptive(_clone(x_T), control="batch", poll=1, return_stats=True)
        assert next(it, None) is None, "different number of network evaluations than the reference"
        it = iter(int(s) for s in g["shifts"])
        nfe = solver.nfe
        with torch.no_grad():
            eager = solver.sample(_clone(x_T), order=2, method="adaptive")
        assert next(it, None) is None and solver.nfe - nfe == int(g["nfe"])
    finally:
        model.shift_source = None
    ev, ea = rel_l2(out["video"].cpu(), g["video"]), rel_l2(out["audio"].cpu(), g["audio"])
    dv, da = rel_l2(out["video"].cpu(), eager["video"].cpu()), rel_l2(out["audio"].cpu(), eager["audio"].cpu())
    print(f"fixture: rel-L2 video {ev:.3e} audio {ea:.3e}; against the eager solver video {dv:.3e} audio {da:.3e}; "
          f"trials {stats['trials']} accepted {stats['accepted'].tolist()}")
    assert stats["trials"] == 34 and stats["accepted"].tolist() == [24] * B and stats["nfe"].tolist() == [68] * B and stats["host_reads"] == 34
    assert ev < 1e-4 and ea < 1e-4
    assert dv < 1e-4 and da < 1e-4


def test_conditioning():
    fl, model, solver = _solver()
    B = 2
    x_T = _x_T(fl, B, 8)
    g = torch.Generator().manual_seed(3)
    F, C, Hh, Ww = fl["video_size"]
    L = fl["audio_size"][1]
    known = {"video": (torch.randn(B, F, C, Hh, Ww, generator=g) * 0.5).cuda(), "audio": (torch.randn(B, 1, L, generator=g) * 0.5).cuda()}
    empty = {"video": torch.zeros(B, F, Hh, Ww, dtype=torch.bool), "audio": torch.zeros(L, dtype=torch.bool)}
    try:
        _replay(model, 6)
        want = solver.sample_graph_adaptive(_clone(x_T), **LOOSE)
        _replay(model, 6)
        got = solver.sample_graph_adaptive(_clone(x_T), known=known, mask=empty, **LOOSE)
        assert same(got["video"], want["video"]) and same(got["audio"], want["audio"])
        # video -> audio: the whole video stream is known
        outs = []
        for kw in (dict(lanes=1), dict(lanes=1, poll=1), dict(lanes=2, poll=7)):
            _replay(model, 6)
            outs.append(solver.sample_graph_adaptive(_clone(x_T), known={"video": known["video"]}, **dict(LOOSE, **kw)))
        _replay(model, 6)
        raw = solver.sample_graph_adaptive(_clone(x_T), known={"video": known["video"]}, paste_known=False, **LOOSE)
    finally:
        model.shift_source = None
    assert same(outs[0]["video"], known["video"]) and not same(raw["video"], known["video"]) and same(raw["audio"], outs[0]["audio"])
    assert not same(outs[0]["audio"], want["audio"]) and torch.isfinite(outs[0]["audio"]).all()
    for o in outs[1:]:
        assert same(o["video"], outs[0]["video"]) and same(o["audio"], outs[0]["audio"])


def test_limits_and_refusals():
    from mm_diffusion._hip import MMDError
    from mm_diffusion.seeded import CounterNoise
    fl, model, solver = _solver()
    x_T = _x_T(fl, 2, 4)
    with pytest.raises(MMDError, match="max_attempts = 3 trial steps"):
        solver.sample_graph_adaptive(_clone(x_T), max_attempts=3, poll=2)
    assert solver._stepper is None          # a loop that raised keeps no stepper
    out = solver.sample_graph_adaptive(_clone(x_T), **LOOSE)      # and the next call builds a new one
    assert torch.isfinite(out["video"]).all()
    for kw, word in ((dict(order=3), "order"), (dict(solver_type="taylor"), "solver_type"), (dict(control="batch", lanes=2), "lanes"),
                     (dict(poll=0), "poll"), (dict(noise_source=CounterNoise(1)), "x_T must be None"), (dict(lanes=3), "lanes")):
        with pytest.raises(MMDError, match=word):
            solver.sample_graph_adaptive(_clone(x_T), **kw)
    with pytest.raises(MMDError, match="CPU tensor"):
        solver.sample_graph_adaptive({k: v.cpu() for k, v in x_T.items()})
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    with pytest.raises(MMDError, match="predict_x0"):
        DPM_Solver(model=model, alphas_cumprod=torch.linspace(0.999, 0.001, 1000), predict_x0=False).sample_graph_adaptive(_clone(x_T))
