"""CPU-side checks of the graph-replayed adaptive DPM-Solver++ (DPM_Solver.sample_graph_adaptive): the float64 restatement of the device
controller (tests/dpm_adapt_ref.py) against oracle/dpm_ref.py's schedule and against the identities of its coefficient rows, its model
timesteps against model_wrapper.get_model_input_time, the C ABI of the mmd_dpm_adapt_* entry points, the refused arguments, the restated
loop against the reference's fixture, and the comparisons of the GPU tests against seeded defects.

Bounds.  The restatement evaluates the schedule in float64 from the fp32 knots the oracle interpolates in fp32: the two agree to fp32
accuracy - for lambda 2^-24 (1 / sigma^2 + 2 (1 + |lambda|)): the fp32 form of 1 - exp(2 log alpha) cancels near t_0; for a time 1e-5
relative to 1 + t.  The
identities hold to 1e-12: a dozen float64 operations on values of magnitude at most 10.  The restated loop is held to the 1e-3 rel-L2
that tests/test_oracle_golden.py grants the oracle's own adaptive solver on the same fixture."""
import os
import re

import numpy as np
import pytest
import torch

import dpm_adapt_ref as R
from conftest import ROOT
from helpers import flags, gold, rel_l2, synth_sd

NEW = ("mmd_dpm_adapt_open", "mmd_dpm_adapt_close", "mmd_dpm_adapt_control", "mmd_dpm_adapt_commit", "mmd_dpm_adapt_time", "mmd_dpm_adapt_chunks")
PARAMS = dict(atol=0.0078, rtol=0.05, theta=0.9, t_err=1e-5, h_init=0.05, t_T=1.0, t_0=1e-3)


class _Model:
    video_out_channels, audio_out_channels = 3, 1


def _alphas_cumprod():
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64)
    return torch.cumprod(1 - betas, 0).float()


def _solver(predict_x0=True, thresholding=False, **kw):
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    return DPM_Solver(_Model(), alphas_cumprod=_alphas_cumprod(), predict_x0=predict_x0, thresholding=thresholding, **kw)


def _schedule():
    return R.Schedule(_solver().adaptive_tables()["log_alpha"])


# ----------------------------------------------------------------------------- the float64 restatement
def test_schedule_agrees_with_the_oracle_to_fp32_accuracy():
    from oracle import dpm_ref
    S, O = _schedule(), dpm_ref.Schedule(_alphas_cumprod())
    ts = np.concatenate([np.linspace(1e-3, 1.0, 397), [1e-3, 1.0, 0.5, 0.0015]])
    for t in ts:
        lam_o = float(O.lam(torch.tensor([t], dtype=torch.float32)))
        lam = S.lam(np.float32(t))
        # the oracle forms sigma^2 = 1 - exp(2 log alpha) in fp32: 1.5 x 2^-24 absolute on it, half of that over sigma^2 on lambda
        assert abs(lam - lam_o) <= 2.0 ** -24 * (1.0 / S.sigma(np.float32(t)) ** 2 + 2 * (1 + abs(lam_o))), (t, lam, lam_o)
        t_o = float(O.inv_lam(torch.tensor([lam_o], dtype=torch.float32)))
        assert abs(S.inv_lam(lam_o) - t_o) <= 1e-5 * (1 + abs(t_o)), (t, S.inv_lam(lam_o), t_o)
        assert abs(S.inv_lam(S.lam(t)) - t) <= 1e-12, t          # the inverse is the inverse
    assert S.T == 1000 and abs(S.alpha(0.37) ** 2 + S.sigma(0.37) ** 2 - 1.0) <= 1e-15


def test_coefficient_rows_keep_the_mean():
    """a0 alpha_s + a1 = alpha_t, b0 alpha_s + b1 = alpha_s1, c0 alpha_s + c1 + c2 = alpha_t: with a perfect data prediction m = mu and
    x = alpha_s mu + sigma_s eps, every update keeps the mean alpha mu of its target time."""
    S = _schedule()
    rng = np.random.default_rng(0)
    for _ in range(300):
        s = float(rng.uniform(2e-3, 1.0))
        lam_s = S.lam(s)
        h = float(min(rng.uniform(1e-3, 1.5), S.lam(1e-3) - lam_s))
        r = R.rows(S, s, h, lam_s)
        f, al_s = r["f64"], S.alpha(s)
        assert abs(f[2] * al_s + f[3] - S.alpha(r["t"])) <= 1e-12
        assert abs(f[4] * al_s + f[5] - S.alpha(r["s1"])) <= 1e-12
        assert abs(f[8] * al_s + f[9] + f[10] - S.alpha(r["t"])) <= 1e-12
        assert f[9] == 0.0 and f[8] == f[2] and f[10] == f[3]      # r1 = 1/2: the second-order result needs the midpoint value alone
        assert abs(f[0] * al_s - 1.0) <= 1e-15 and abs(f[0] * S.sigma(s) + f[1]) <= 1e-12      # x0 of x = alpha mu + sigma eps is mu
        assert abs(S.lam(r["s1"]) - (lam_s + 0.5 * h)) <= 1e-12 and abs(S.lam(r["t"]) - (lam_s + h)) <= 1e-12
        mu = 0.7
        x = al_s * mu
        assert abs((f[2] * x + f[3] * mu) - S.alpha(r["t"]) * mu) <= 1e-12


def test_rows_are_the_host_helpers_values():
    """The rows against what the eager solver's helpers compute in fp32 for the same s and t: 2e-5 relative (they evaluate lambda, about
    10, in fp32: 10 x 2^-24 absolute on h, which the coefficients inherit)."""
    sv, S = _solver(), _schedule()
    for s, h in ((1.0, 0.05), (0.6, 0.8), (0.05, 0.3)):
        lam_s = S.lam(np.float32(s))
        r = R.rows(S, float(np.float32(s)), h, lam_s)
        st, tt = torch.tensor([s]), torch.tensor([r["t"]], dtype=torch.float32)
        a = sv._first_coefs(st, tt)["video"]
        _, b, c = sv._single_second_coefs(st, tt, 0.5, "dpm_solver")
        cx, ce = sv._x0_coefs(st)
        want = [cx, ce, a[0], a[1], b[0], b[1]]
        for got, w in zip(r["f64"][:6], want):
            assert abs(got - w) <= 2e-5 * max(abs(w), 1e-2), (s, h, got, w)
        assert abs(r["f64"][8] - c[0]) <= 2e-5 and abs(r["f64"][10] - c[2]) <= 2e-5 * max(abs(c[2]), 1e-2) and c[1] == 0.0


def test_model_timesteps_are_the_wrappers():
    sv, S = _solver(), _schedule()
    ts = np.concatenate([np.linspace(1e-3, 1.0, 20001), (np.arange(1000) + 1) / 1000.0, [1.0, 1e-3]])
    want = sv.model.get_model_input_time(torch.tensor(ts, dtype=torch.float32))
    got = np.array([S.model_time(t) for t in ts])
    assert np.array_equal(got, want.numpy().astype(np.int64))
    assert S.model_time(1.0) == int(want[-2]) and S.model_time(1e-3) == int(want[-1]) == 0


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_in_header_binding_and_library():
    from mm_diffusion import _hip, ops
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(_hip.lib(), name), name
    assert ops.DPM_ADAPT_CHUNK == R.CHUNK == int(re.search(r"#define MMD_DPM_ADAPT_CHUNK (\d+)", hdr).group(1))
    assert (ops.ADAPT_FLAG_REJECT, ops.ADAPT_FLAG_ACCEPT, ops.ADAPT_FLAG_IDLE) == (R.REJECT, R.ACCEPT, R.IDLE)
    for name, i in ops.ADAPT_P.items():
        assert int(re.search(r"#define MMD_ADAPT_P_%s (\d+)" % {"t_err": "TERR", "h_init": "HINIT", "t_T": "TT", "t_0": "T0"}.get(name, name.upper()), hdr).group(1)) == i
    lib = _hip.lib()
    assert [lib.mmd_dpm_adapt_chunks(p) for p in (0, 1, 4096, 4097, 3 * 4096 + 5)] == [0, 1, 1, 2, 4]
    assert [ops.dpm_adapt_chunks(p) for p in (1, 4096, 4097)] == [1, 1, 2]


def test_bad_arguments_return_codes_and_name_the_entry():
    from mm_diffusion import _hip
    lib = _hip.lib()
    # non-NULL pointers that are never dereferenced (the checks run before any launch), far enough apart not to overlap
    x, src, XB, MS, LO, PREV, s, tab, k, par, part = (4096 * (i + 1) for i in range(11))

    def refused(f, name, word, *args):
        assert f(*args) < 0
        msg = lib.mmd_last_error()
        assert name in msg and word in msg, msg
    f = lib.mmd_dpm_adapt_open
    refused(f, b"dpm_adapt_open", b"LO", x, src, 0, XB, MS, None, None, 1.0, tab, k, 4, 1, 1, 1, 1, 1, None)
    refused(f, b"dpm_adapt_open", b"N (", x, src, 0, XB, MS, LO, None, 1.0, tab, k, 4, 0, 1, 1, 1, 1, None)
    refused(f, b"dpm_adapt_open", b"2C", x, src, 0, XB, MS, LO, None, 1.0, tab, k, 4, 1, 1, 3, 5, 1, None)
    refused(f, b"dpm_adapt_open", b"overlap", x, src, 0, XB, MS, x + 4, None, 1.0, tab, k, 4, 1, 1, 1, 1, 2, None)
    refused(f, b"dpm_adapt_open", b"form 0", x, src, 1, XB, MS, LO, s, 1.0, tab, k, 4, 1, 1, 1, 1, 1, None)
    refused(f, b"dpm_adapt_open", b"max_val", x, src, 0, XB, MS, LO, s, 0.0, tab, k, 4, 1, 1, 1, 1, 1, None)
    f = lib.mmd_dpm_adapt_close
    refused(f, b"dpm_adapt_close", b"PREV", x, src, 0, XB, MS, LO, None, None, 1.0, tab, k, 4, par, part, 1, 1, 1, 1, 1, None)
    refused(f, b"dpm_adapt_close", b"partial", x, src, 0, XB, MS, LO, PREV, None, 1.0, tab, k, 4, par, None, 1, 1, 1, 1, 1, None)
    refused(f, b"dpm_adapt_close", b"overlap", x, src, 0, XB, MS, LO, XB, None, 1.0, tab, k, 4, par, part, 1, 1, 1, 1, 1, None)
    refused(f, b"dpm_adapt_close", b"N (", x, src, 0, XB, MS, LO, PREV, None, 1.0, tab, k, 4, par, part, -1, 1, 1, 1, 1, None)
    f = lib.mmd_dpm_adapt_control
    refused(f, b"dpm_adapt_control", b"status", 1, 0, par, tab, 1000, None, 0, 0, None, 0, 0, x, k, XB, MS, None, 2, None)
    refused(f, b"dpm_adapt_control", b"mode", 2, 0, par, tab, 1000, None, 0, 0, None, 0, 0, x, k, XB, MS, LO, 2, None)
    refused(f, b"dpm_adapt_control", b"N must", 1, 0, par, tab, 1000, None, 0, 0, None, 0, 0, x, k, XB, MS, LO, 0, None)
    refused(f, b"dpm_adapt_control", b"partial sums", 0, 0, par, tab, 1000, None, 1, 5, None, 0, 0, x, k, XB, MS, LO, 2, None)
    f = lib.mmd_dpm_adapt_commit
    refused(f, b"dpm_adapt_commit", b"counters", x, XB, PREV, LO, None, 1, 8, None)
    refused(f, b"dpm_adapt_commit", b"overlap", x, XB, x, LO, k, 1, 8, None)
    refused(f, b"dpm_adapt_commit", b"N in", x, XB, PREV, LO, k, 0, 8, None)
    f = lib.mmd_dpm_adapt_time
    refused(f, b"dpm_adapt_time", b"needs", None, x, 2, None)
    refused(f, b"dpm_adapt_time", b"overlap", x, x + 8, 2, None)


def test_sample_graph_adaptive_names_what_it_refuses():
    from mm_diffusion._hip import MMDError
    from mm_diffusion.seeded import CounterNoise
    s = _solver()
    cpu = {"video": torch.zeros(2, 8, 3, 16, 16), "audio": torch.zeros(2, 1, 512)}
    for kw, word in ((dict(order=3), "order"), (dict(order=1), "order"), (dict(solver_type="taylor"), "solver_type"),
                     (dict(control="batch", lanes=2), "lanes"), (dict(poll=0), "poll"), (dict(control="each"), "control"),
                     (dict(max_attempts=0), "max_attempts")):
        with pytest.raises(MMDError, match=word):
            s.sample_graph_adaptive(cpu, **kw)
    with pytest.raises(MMDError, match="predict_x0"):
        _solver(predict_x0=False).sample_graph_adaptive(cpu)
    with pytest.raises(MMDError, match="model_kwargs"):
        _solver(model_kwargs={"y": 1}).sample_graph_adaptive(cpu)
    with pytest.raises(MMDError, match="x_T must be None"):
        s.sample_graph_adaptive(cpu, noise_source=CounterNoise(1))
    with pytest.raises(MMDError, match="CounterNoise"):
        s.sample_graph_adaptive(cpu, noise_source=lambda like: like)
    with pytest.raises(MMDError, match="CPU tensor"):
        s.sample_graph_adaptive(cpu)
    with pytest.raises(MMDError, match="x_T or shape"):
        s.sample_graph_adaptive()
    from mm_diffusion.dpm_solver_plus import DPM_Solver as TensorSolver
    sr = TensorSolver(_Model(), alphas_cumprod=_alphas_cumprod(), predict_x0=True)
    with pytest.raises(MMDError, match="tensor solver"):
        sr.sample_graph_adaptive({"x": torch.zeros(1, 3, 8, 8)})
    # the fixed-grid entries still refuse the method, and say where it went
    for fn, kw in ((s.sample_graph, dict(steps=4, method="adaptive")), (s.sample_graph_singlestep, dict(steps=4, method="adaptive"))):
        with pytest.raises(MMDError, match="adaptive.*sample_graph_adaptive"):
            fn(cpu, **kw)
    # the parameter block takes exactly its seven values
    from mm_diffusion import ops
    with pytest.raises(MMDError, match="needs exactly"):
        ops.dpm_adapt_params("cpu", atol=1.0)
    assert sorted(s.adaptive_tables()["params"]) == sorted(ops.ADAPT_P)


# ----------------------------------------------------------------------------- the restated loop against the reference's fixture
def test_restated_loop_matches_the_reference_fixture():
    """control="batch" with the oracle's U-Net on the tiny configuration: the reference's own 68 evaluations, 34 trial steps of which 24
    are accepted, and its samples."""
    from oracle import unet_ref as uref
    from oracle import diffusion_ref as dref
    g = gold("tiny_dpmpp_adaptive2")
    fl = flags("tiny")
    B = int(g["B"])
    oracle = uref.OracleModel(synth_sd("tiny"), fl, shifts=list(g["shifts"]))
    torch.manual_seed(int(g["seed"]))
    x_T = {"video": torch.randn(B, *fl["video_size"]).numpy(), "audio": torch.randn(B, *fl["audio_size"]).numpy()}
    ac = torch.tensor(dref.Schedule().alphas_cumprod, dtype=torch.float32)
    S = R.Schedule((0.5 * torch.log(ac)).double().numpy())
    p = dict(PARAMS, t_T=1.0, t_0=1.0 / S.T)

    def model(x, tm):
        with torch.no_grad():
            v, a = oracle(torch.from_numpy(x["video"]), torch.from_numpy(x["audio"]), torch.from_numpy(tm).to(torch.int))
        return {"video": v[:, :, :3].float().numpy(), "audio": a[:, :1].float().numpy()}
    out, info = R.adaptive_loop(S, p, x_T, model, thresholding=True, control_rule="batch")
    ev, ea = rel_l2(torch.from_numpy(out["video"]), g["video"]), rel_l2(torch.from_numpy(out["audio"]), g["audio"])
    print(f"trials {info['trials']} accepted {info['accepted']} nfe {info['nfe']} margin |E - 1| {info['margin']:.3e} rel-L2 video {ev:.3e} audio {ea:.3e}")
    assert info["nfe"] == int(g["nfe"]) == 68 and info["trials"] == 34 and info["accepted"] == [24] * B
    assert ev < 1e-3 and ea < 1e-3


# ----------------------------------------------------------------------------- seeded defects
def _states(S, p, n, seed):
    """Random mid-loop states with their rows, a share of them close to the end where the cap of h binds."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = float(rng.uniform(1.2e-3, 1.0)) if i % 3 else float(rng.uniform(1.0e-3 + 2e-5, 3e-3))
        st = R.init_state(S, dict(p, t_T=s, h_init=1.0))
        st["h"] = float(min(rng.uniform(0.02, 1.2), st["lam_0"] - st["lam_s"]))
        st["rows"] = R.rows(S, st["s"], st["h"], st["lam_s"])
        out.append(st)
    return out, rng


def test_seeded_defects_are_flagged():
    S, p = _schedule(), PARAMS
    states, rng = _states(S, p, 60, 5)
    Es = [float(np.float32(np.exp(rng.uniform(-2.5, 1.0)))) for _ in states]

    def flagged(defect):
        n = 0
        for st, E in zip(states, Es):
            E_in = E * (1 + 2.0 ** -30) if defect == "E_not_fp32" else E          # what the fp64 square root holds before its rounding
            want = R.control(S, p, st, float(np.float32(E_in)))
            got = R.control(S, p, st, E_in if defect == "E_not_fp32" else E, defect)
            n += bool(R.compare_control(got, want)[0])
        return n
    assert flagged(None) == 0
    assert flagged("E_not_fp32") > 0 and flagged("h_not_capped") > 0 and flagged("s1_at_h") > 0
    # the partial sums: another order inside a chunk gives other bits, which the bitwise comparison sees (the bound alone would not)
    per = 3 * R.CHUNK + 5
    hi, lo, prev = (rng.standard_normal(per).astype(np.float32) for _ in range(3))
    e = R.error_terms(hi, lo, prev, p["atol"], p["rtol"])
    assert R.compare_partials(R.chunk_sums(e), e) == []
    bad = R.compare_partials(R.chunk_sums(e, "chunk_order"), e)
    assert [b[0] for b in bad] == ["order"]
    # the commit: PREV moves on accept only
    x, xb, pv, l = (rng.standard_normal(150).astype(np.float32) for _ in range(4))
    for flag in (R.ACCEPT, R.REJECT, R.IDLE):
        want = R.commit(flag, x, xb, pv, l)
        assert R.compare_commit(R.commit(flag, x, xb, pv, l), want) == []
        assert R.compare_commit(R.commit(flag, x, xb, pv, l, "prev_on_reject"), want) == (["PREV"] if flag == R.REJECT else [])
