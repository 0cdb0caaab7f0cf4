"""CPU-side checks of the graph-replayed single-step DPM-Solver loop: the C ABI of mmd_dpm_single_update, the tables of
DPM_Solver.singlestep_tables against the scalars the eager single-step updates hand to their kernels, the coefficient helpers the eager
methods now share with the tables, the refused arguments, and the numpy restatement of the three row kinds (tests/dpm_single_ref.py)
driven by the tables against oracle/dpm_ref.py's single-step solver on a closed-form model."""
import os
import re

import numpy as np
import pytest
import torch

import dpm_single_ref as R
from conftest import ROOT
from helpers import rel_l2

NEW = "mmd_dpm_single_update"


class _Model:
    video_out_channels, audio_out_channels = 3, 1


def _alphas_cumprod():
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64)
    return torch.cumprod(1 - betas, 0).float()


def _solver(predict_x0, thresholding=False, **kw):
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    return DPM_Solver(_Model(), alphas_cumprod=_alphas_cumprod(), predict_x0=predict_x0, thresholding=thresholding, **kw)


def test_symbol_in_header_binding_and_library():
    from mm_diffusion import _hip, ops
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    assert NEW in declared and NEW in _hip.EXPORTS and hasattr(_hip.lib(), NEW)
    assert (ops.DPM1_KIND_OPEN, ops.DPM1_KIND_STAGE, ops.DPM1_KIND_DENOISE) == (0, 1, 2) == (R.OPEN, R.STAGE, R.DENOISE)


def test_bad_arguments_return_codes_and_name_the_entry():
    from mm_diffusion import _hip
    lib = _hip.lib()
    # non-NULL pointers that are never dereferenced (the checks run before any launch), far enough apart not to overlap
    x, src, XB, MS, s, tab, k = (4096 * (i + 1) for i in range(7))
    f = lib.mmd_dpm_single_update

    def refused(word, *args):
        assert f(*args) < 0
        msg = lib.mmd_last_error()
        assert b"dpm_single_update" in msg and word in msg, msg
    refused(b"XB", x, src, 0, None, MS, None, 1.0, tab, k, 4, 1, 1, 1, 1, 1, None)
    refused(b"2C", x, src, 0, XB, MS, None, 1.0, tab, k, 4, 1, 1, 3, 5, 1, None)
    refused(b"rows", x, src, 0, XB, MS, None, 1.0, tab, k, 0, 1, 1, 3, 3, 1, None)
    refused(b"max_val", x, src, 0, XB, MS, s, 0.0, tab, k, 4, 1, 1, 1, 1, 1, None)
    refused(b"form 0", x, src, 1, XB, MS, s, 1.0, tab, k, 4, 1, 1, 1, 1, 1, None)
    refused(b"overlap", x, src, 0, x, MS, None, 1.0, tab, k, 4, 1, 1, 1, 1, 1, None)
    refused(b"overlap", x, src, 0, XB, x + 4, None, 1.0, tab, k, 4, 1, 1, 1, 1, 2, None)      # HW = 2 elements: MS starts inside x
    refused(b"form", x, src, 2, XB, MS, None, 1.0, tab, k, 4, 1, 1, 1, 1, 1, None)


def test_cpu_tensors_raise():
    from mm_diffusion import ops
    from mm_diffusion._hip import MMDError
    x, k, tab = torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(6, 4)
    with pytest.raises(MMDError, match="CPU tensor"):
        ops.dpm_single_update(x, x.clone(), x.clone(), x.clone(), tab, k, 1, 1, 1, 8)


# ----------------------------------------------------------------------------- tables
class _Recorder:
    """Stands in for ops.lincomb: keeps the scalars as the C ABI receives them (fp32) and returns its first tensor."""

    def __init__(self):
        self.calls = []

    def __call__(self, a, ca, b=None, cb=0.0, c=None, cc=0.0, out=None):
        self.calls.append((np.float32(ca), np.float32(cb), np.float32(cc), c is not None))
        return a


def _eager_scalars(solver, monkeypatch, steps, order, skip_type, method, solver_type, denoise):
    """Walk sample(method=...) on one-element CPU tensors with the kernels replaced by a recorder: per evaluation the (cx, ce) of
    data_prediction_fn, per update the coefficients of each stream, and the model's integer timesteps."""
    from mm_diffusion import multimodal_dpm_solver_plus as M
    rec = _Recorder()
    monkeypatch.setattr(M.ops, "lincomb", rec)
    monkeypatch.setattr(solver, "_prep", lambda x: x)
    tms = []

    def fake_noise(x, t):
        tms.append(int(solver.model.get_model_input_time(t.reshape(-1)[:1])[0]))
        return {k: torch.zeros(2, 1) for k in solver.KEYS}
    monkeypatch.setattr(solver, "noise_prediction_fn", fake_noise)
    x = {k: torch.zeros(2, 1) for k in solver.KEYS}
    solver.sample(x, steps=steps, order=order, skip_type=skip_type, method=method, denoise=denoise, solver_type=solver_type)
    return rec.calls, tms


# every tail of the orders list occurs: [1], [2, 1], [2, 2], [2, 1] / [3, 1] / [3, 2] / [3, 2, 1] / [3 x 6, 2]
GRIDS = [(1, 2), (2, 3), (2, 4), (3, 3), (3, 4), (3, 5), (3, 6), (3, 20)]
CASES = [(px, o, st, skip, "singlestep", "dpm_solver", True) for px in (True, False) for o, st in GRIDS
         for skip in ("logSNR", "time_uniform", "time_quadratic")]
CASES += [(px, o, st, "logSNR", "singlestep_fixed", "dpm_solver", True) for px in (True, False) for o, st in ((3, 7), (2, 5))]
CASES += [(px, 2, st, skip, "singlestep", "taylor", True) for px in (True, False) for st in (3, 4) for skip in ("logSNR", "time_uniform")]
CASES += [(px, o, st, "logSNR", "singlestep", "dpm_solver", False) for px in (True, False) for o, st in ((3, 5), (2, 3), (1, 2))]


def _orders(solver, steps, order, method):
    return solver.get_orders_for_singlestep_solver(steps, order) if method == "singlestep" else [order] * (steps // order)


@pytest.mark.parametrize("px,order,steps,skip,method,st,denoise", CASES)
def test_table_rows_equal_the_eager_scalars(monkeypatch, px, order, steps, skip, method, st, denoise):
    solver = _solver(px)
    tabs = solver.singlestep_tables(steps, order, skip, method, st, denoise=denoise)
    calls, tms = _eager_scalars(_solver(px), monkeypatch, steps, order, skip, method, st, denoise)
    orders = _orders(solver, steps, order, method)
    kinds = [kd for p in orders for kd in [R.OPEN] + [R.STAGE] * (p - 1)] + ([R.DENOISE] if denoise else [])
    assert tabs["rows"] == len(tms) == sum(orders) + (1 if denoise else 0) and tabs["tm"] == tms, (tabs["tm"], tms)
    it = iter(calls)
    for j, kind in enumerate(kinds):
        if px or kind == R.DENOISE:                      # data_prediction_fn: one lincomb per stream
            for k in solver.KEYS:
                ca, cb, _, _ = next(it)
                assert (tabs["tab"][k][0, j], tabs["tab"][k][1, j]) == (ca, cb), (j, k)
        else:
            assert all(tabs["tab"][k][0, j] == 0 and tabs["tab"][k][1, j] == 0 for k in solver.KEYS)
        assert all(tabs["tab"][k][5, j] == kind for k in solver.KEYS), (j, kind)
        if kind == R.DENOISE:
            break
        for k in solver.KEYS:               # the state the next evaluation (or the next step) starts from: one lincomb per stream
            ca, cb, cc, three = next(it)
            row = tabs["tab"][k][:, j]
            assert three == (kind == R.STAGE), (j, k)
            assert (row[2], row[3]) == (ca, cb), (j, k, row, ca, cb)
            assert row[4] == (cc if three else 0.0), (j, k, row, cc)
    assert next(it, None) is None
    if not px and orders[-1] == 1:      # the reference's quirk: a first-order noise-prediction step moves the audio stream otherwise
        j = sum(orders) - 1
        assert tabs["tab"]["audio"][2, j] != tabs["tab"]["video"][2, j]
    # the conditioning table is alpha, sigma of the evaluation times
    ns = solver.noise_schedule
    np.testing.assert_array_equal(tabs["tab2"][0], ns.marginal_alpha(tabs["timesteps"]).numpy())
    np.testing.assert_array_equal(tabs["tab2"][1], ns.marginal_std(tabs["timesteps"]).numpy())
    assert solver.singlestep_tables(steps, order, skip, method, st, denoise=denoise) is tabs, "the tables are kept per argument set"


@pytest.mark.parametrize("px", [True, False])
def test_eager_refactor_keeps_the_scalars(px):
    """The helpers the eager single-step updates now call compute what the methods computed inline: restated here from the schedule."""
    from mm_diffusion.multimodal_dpm_solver_plus import _f
    sv = _solver(px)
    ns = sv.noise_schedule
    s, t = torch.tensor([0.9]), torch.tensor([0.5])
    r1, r2 = torch.tensor([0.3]), torch.tensor([0.7])
    lam, la, sg = ns.marginal_lambda, ns.marginal_log_mean_coeff, ns.marginal_std
    h = lam(t) - lam(s)
    s1, s2 = ns.inverse_lambda(lam(s) + r1 * h), ns.inverse_lambda(lam(s) + r2 * h)
    r1f, r2f = _f(r1), _f(r2)
    a_s1, a_s2, a_t = torch.exp(la(s1)), torch.exp(la(s2)), torch.exp(la(t))
    if px:
        p11, p12, p1 = torch.expm1(-r1 * h), torch.expm1(-r2 * h), torch.expm1(-h)
        p22, p2 = torch.expm1(-r2 * h) / (r2 * h) + 1., p1 / h + 1.
        a1, b1 = _f(sg(s1) / sg(s)), -_f(a_s1 * p11)
        a2, b2, d2 = _f(sg(s2) / sg(s)), -_f(a_s2 * p12), (r2f / r1f) * _f(a_s2 * p22)
        c0, c1 = _f(sg(t) / sg(s)), -_f(a_t * p1)
        c2_3 = (1. / r2f) * _f(a_t * p2)
        c2_2 = -(0.5 / r1f) * _f(a_t * p1)
        c2_2t = (1. / r1f) * _f(a_t * ((torch.exp(-h) - 1.) / h + 1.))
    else:
        p11, p12, p1 = torch.expm1(r1 * h), torch.expm1(r2 * h), torch.expm1(h)
        p22, p2 = torch.expm1(r2 * h) / (r2 * h) - 1., p1 / h - 1.
        a1, b1 = _f(torch.exp(la(s1) - la(s))), -_f(sg(s1) * p11)
        a2, b2, d2 = _f(torch.exp(la(s2) - la(s))), -_f(sg(s2) * p12), -(r2f / r1f) * _f(sg(s2) * p22)
        c0, c1 = _f(torch.exp(la(t) - la(s))), -_f(sg(t) * p1)
        c2_3 = -(1. / r2f) * _f(sg(t) * p2)
        c2_2 = -(0.5 / r1f) * _f(sg(t) * p1)
        c2_2t = -(1. / r1f) * _f(sg(t) * ((torch.exp(h) - 1.) / h - 1.))
    g1, g2, first, mid, last = sv._single_third_coefs(s, t, r1, r2, "dpm_solver")
    assert torch.equal(g1, s1) and torch.equal(g2, s2)
    assert (first, mid, last) == ((a1, b1), (a2, b2 - d2, d2), (c0, c1 - c2_3, c2_3))
    for st, c2 in (("dpm_solver", c2_2), ("taylor", c2_2t)):
        g1, first, last = sv._single_second_coefs(s, t, r1, st)
        assert torch.equal(g1, s1) and (first, last) == ((a1, b1), (c0, c1 - c2, c2)), st
    # the defaults of the public methods: r1 = 1/2, and 1/3, 2/3
    assert torch.equal(sv._single_second_coefs(s, t, None, "dpm_solver")[0], ns.inverse_lambda(lam(s) + torch.tensor([0.5]) * h))
    assert torch.equal(sv._single_third_coefs(s, t, None, None, "dpm_solver")[1], ns.inverse_lambda(lam(s) + torch.tensor([2. / 3.]) * h))
    with pytest.raises(NotImplementedError, match="taylor"):
        sv._single_third_coefs(s, t, r1, r2, "taylor")
    with pytest.raises(ValueError, match="solver_type"):
        sv._single_second_coefs(s, t, r1, "midpoint")


# ----------------------------------------------------------------------------- refused arguments
def test_sample_graph_singlestep_names_what_it_refuses():
    from mm_diffusion._hip import MMDError
    s = _solver(True)
    cpu = {"video": torch.zeros(2, 8, 3, 16, 16), "audio": torch.zeros(2, 1, 512)}
    for kw, word in ((dict(order=4), "order"), (dict(order=3, solver_type="taylor"), "taylor"), (dict(method="adaptive"), "adaptive"),
                     (dict(method="multistep"), "'multistep'"), (dict(steps=0), "steps"), (dict(solver_type="midpoint"), "solver_type"),
                     (dict(method="singlestep_fixed", steps=2, order=3), "steps")):
        with pytest.raises(MMDError, match=word):
            s.sample_graph_singlestep(cpu, **dict(dict(steps=4), **kw))
        kw.pop("denoise", None)
        if "method" not in kw or kw["method"] == "singlestep_fixed":
            with pytest.raises(MMDError, match=word):
                s.singlestep_tables(**dict(dict(steps=4), **kw))
    with pytest.raises(MMDError, match="CPU tensor"):
        s.sample_graph_singlestep(cpu, steps=4)
    with pytest.raises(MMDError, match="CounterNoise"):
        s.sample_graph_singlestep(cpu, steps=4, noise_source=lambda like: like)
    from mm_diffusion.seeded import CounterNoise
    with pytest.raises(MMDError, match="x_T must be None"):
        s.sample_graph_singlestep(cpu, steps=4, noise_source=CounterNoise(1))
    with pytest.raises(MMDError, match="model_kwargs"):
        _solver(True, model_kwargs={"y": 1}).sample_graph_singlestep(cpu, steps=4)
    with pytest.raises(MMDError, match="x_T or shape"):
        s.sample_graph_singlestep(steps=4)
    # the multistep entry still refuses the single-step method, and says where it went
    with pytest.raises(MMDError, match="single-step.*sample_graph_singlestep"):
        s.sample_graph(cpu, steps=4, method="singlestep")


# ----------------------------------------------------------------------------- the three kinds, restated, against the oracle's solver
def _toy(video, audio, ti):
    """A closed-form noise prediction: smooth in the state, weakly dependent on the integer timestep."""
    w = ti.float() / 1000.
    return 0.5 * torch.tanh(video) + 0.02 * w.reshape(-1, 1, 1, 1, 1), 0.5 * torch.sin(audio) - 0.02 * w.reshape(-1, 1, 1)


def _toy_np(x, tm):
    B = x["video"].shape[0]
    v, a = _toy(torch.from_numpy(x["video"]), torch.from_numpy(x["audio"]), torch.full((B,), int(tm), dtype=torch.int))
    return {"video": v.numpy(), "audio": a.numpy()}


_ORACLE = {}
ORACLE_CASES = [(True, 3, 6, "logSNR", True), (False, 3, 6, "logSNR", True), (True, 3, 5, "time_uniform", False), (False, 3, 4, "logSNR", False),
                (False, 2, 3, "time_uniform", True), (True, 2, 4, "time_quadratic", False), (False, 1, 2, "logSNR", False)]


def _oracle(px, order, steps, skip, denoise):
    """(x_T, the oracle's result), computed once per case and shared (never modified)."""
    key = (px, order, steps, skip, denoise)
    if key not in _ORACLE:
        from oracle import dpm_ref
        g = torch.Generator().manual_seed(3)
        x_T = {"video": torch.randn(2, 2, 3, 4, 4, generator=g), "audio": torch.randn(2, 1, 16, generator=g)}
        ref = dpm_ref.Solver(_toy, _alphas_cumprod(), predict_x0=px).sample({k: v.clone() for k, v in x_T.items()}, steps=steps, order=order,
                                                                            skip_type=skip, method="singlestep", denoise=denoise)
        _ORACLE[key] = ({k: v.numpy() for k, v in x_T.items()}, ref)
    return _ORACLE[key]


@pytest.mark.parametrize("px,order,steps,skip,denoise", ORACLE_CASES)
def test_restated_kinds_agree_with_the_oracle_solver(px, order, steps, skip, denoise):
    x_T, ref = _oracle(px, order, steps, skip, denoise)
    tabs = _solver(px).singlestep_tables(steps, order, skip, "singlestep", "dpm_solver", denoise=denoise)
    got = R.run(tabs, _toy_np, x_T, px)
    for k in ("video", "audio"):
        err = rel_l2(torch.from_numpy(got[k]), ref[k])
        print(f"px {px} order {order} steps {steps} {skip} denoise {denoise} {k}: rel-L2 {err:.3e}")
        assert err < 1e-4, (k, err)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_are_flagged(defect):
    flagged = 0
    for px in (True, False):
        x_T, ref = _oracle(px, 3, 6, "logSNR", True)
        tabs = _solver(px).singlestep_tables(6, 3, "logSNR", "singlestep", "dpm_solver", denoise=True)
        got = R.run(tabs, _toy_np, x_T, px, defect=defect)
        errs = [rel_l2(torch.from_numpy(got[k]), ref[k]) for k in ("video", "audio")]
        print(f"{defect} px {px}: rel-L2 {errs}")
        flagged += max(errs) >= 1e-4
    assert flagged == 2, (defect, flagged)
