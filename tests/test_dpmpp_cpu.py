"""CPU-side checks of the graph-replayed DPM-Solver++ loop: the C ABI, the coefficient tables against the scalars the eager update
methods hand to their kernels, the numpy restatement of the multi-level selection (tests/dpmpp_ref.py) and the refused arguments."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import dpmpp_ref as R
from conftest import ROOT

NEW = ("mmd_dpmpp_workspace_bytes", "mmd_dpmpp_x0", "mmd_dpmpp_select", "mmd_dpmpp_update")


class _Model:
    video_out_channels, audio_out_channels = 3, 1


def _solver(predict_x0, thresholding=False, **kw):
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64)
    return DPM_Solver(_Model(), alphas_cumprod=torch.cumprod(1 - betas, 0).float(), predict_x0=predict_x0, thresholding=thresholding, **kw)


def test_symbols_in_header_binding_and_library():
    from mm_diffusion import _hip
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    lib = _hip.lib()
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert lib.mmd_dpmpp_workspace_bytes(3) == 3 * R.WS_WORDS * 4 and lib.mmd_dpmpp_workspace_bytes(0) == 0


def test_bad_arguments_return_codes_and_name_the_entry():
    from mm_diffusion import _hip
    lib = _hip.lib()
    one = 8      # a non-NULL pointer that is never dereferenced: the checks run before any launch
    assert lib.mmd_dpmpp_x0(None, one, one, one, one, 4, None, 1, 1, 1, 1, 1, None) < 0 and b"dpmpp_x0" in lib.mmd_last_error()
    assert lib.mmd_dpmpp_x0(one, one, one, one, one, 4, None, 1, 1, 3, 5, 1, None) < 0 and b"2C" in lib.mmd_last_error()
    assert lib.mmd_dpmpp_x0(one, one, one, one, one, 0, None, 1, 1, 3, 3, 1, None) < 0 and b"rows" in lib.mmd_last_error()
    assert lib.mmd_dpmpp_select(one, None, 0, 1, 16, 0.5, one, None) < 0 and b"dpmpp_select" in lib.mmd_last_error()
    assert lib.mmd_dpmpp_select(one, one, 0, 1, 16, 1.5, one, None) < 0 and b"q must be" in lib.mmd_last_error()
    assert lib.mmd_dpmpp_select(one, one, 0, 1, 0, 0.5, one, None) < 0 and b"per_sample" in lib.mmd_last_error()
    assert lib.mmd_dpmpp_update(one, one, None, None, 1.0, one, one, 4, 1, 1, 1, 1, 1, None) < 0 and b"dpmpp_update" in lib.mmd_last_error()
    assert lib.mmd_dpmpp_update(one, one, one, one, 0.0, one, one, 4, 1, 1, 1, 1, 1, None) < 0 and b"max_val" in lib.mmd_last_error()


# ----------------------------------------------------------------------------- tables
class _Recorder:
    """Stands in for ops.lincomb: keeps the scalars as the C ABI receives them (fp32) and returns its first tensor."""

    def __init__(self):
        self.calls = []

    def __call__(self, a, ca, b=None, cb=0.0, c=None, cc=0.0, out=None):
        self.calls.append((np.float32(ca), np.float32(cb), np.float32(cc), c is not None))
        return a


def _eager_scalars(solver, monkeypatch, steps, order, skip_type, solver_type, denoise):
    """Walk sample(method="multistep") on one-element CPU tensors with the kernels replaced by a recorder: per evaluation the (cx, ce) of
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
    solver.sample(x, steps=steps, order=order, skip_type=skip_type, method="multistep", denoise=denoise, solver_type=solver_type)
    return rec.calls, tms


CASES = [(px, order, skip, steps, st) for px in (True, False) for order in (1, 2) for skip in ("logSNR", "time_uniform", "time_quadratic")
         for steps in (2, 10, 20, 50) for st in ("dpm_solver", "taylor") if not (st == "taylor" and not px)]


@pytest.mark.parametrize("px,order,skip,steps,st", CASES)
def test_table_rows_equal_the_eager_scalars(monkeypatch, px, order, skip, steps, st):
    from mm_diffusion import ops
    solver = _solver(px)
    tabs = solver.graph_tables(steps, order, skip, st, denoise=True)
    calls, tms = _eager_scalars(_solver(px), monkeypatch, steps, order, skip, st, denoise=True)
    assert tabs["rows"] == steps + 1 and tabs["tm"] == tms, (tabs["tm"], tms)
    it = iter(calls)
    for i in range(steps + 1):
        last = i == steps
        if px or last:                      # data_prediction_fn: one lincomb per stream
            for k in solver.KEYS:
                ca, cb, _, _ = next(it)
                assert (tabs["tab"][k][0, i], tabs["tab"][k][1, i]) == (ca, cb), (i, k)
        if last:
            assert all(tabs["tab"][k][5, i] == ops.DPMPP_KIND_DENOISE for k in solver.KEYS)
            break
        second = order == 2 and i > 0
        for k in solver.KEYS:               # the update from evaluation i: one lincomb per stream
            ca, cb, cc, three = next(it)
            row = tabs["tab"][k][:, i]
            assert three == second and row[5] == (ops.DPMPP_KIND_SECOND if second else ops.DPMPP_KIND_FIRST)
            assert (row[2], row[3]) == (ca, cb), (i, k, row, ca, cb)
            assert row[4] == (cc if second else 0.0)
    assert next(it, None) is None
    if not px:      # the reference's quirk: the first-order noise-prediction step moves the audio stream with the x0-form coefficients
        assert tabs["tab"]["audio"][2, 0] != tabs["tab"]["video"][2, 0]
    # the conditioning table is alpha, sigma of the evaluation times
    ns = solver.noise_schedule
    np.testing.assert_array_equal(tabs["tab2"][0], ns.marginal_alpha(tabs["timesteps"]).numpy())
    np.testing.assert_array_equal(tabs["tab2"][1], ns.marginal_std(tabs["timesteps"]).numpy())


def test_eager_refactor_keeps_the_scalars(monkeypatch):
    """The helpers the eager updates now call compute what the methods computed inline: restated here from the schedule."""
    from mm_diffusion.multimodal_dpm_solver_plus import _f
    s = _solver(True)
    ns = s.noise_schedule
    t1, t0, t = torch.tensor([0.9]), torch.tensor([0.7]), torch.tensor([0.5])
    lam = ns.marginal_lambda
    h0, h = lam(t0) - lam(t1), lam(t) - lam(t0)
    a_t, sg_t, sg_0 = ns.marginal_alpha(t), ns.marginal_std(t), ns.marginal_std(t0)
    c0, c1 = _f(sg_t / sg_0), -_f(a_t * (torch.exp(-h) - 1.))
    cd, inv = -0.5 * _f(a_t * (torch.exp(-h) - 1.)), _f(1. / (h0 / h))
    assert s._second_coefs(t1, t0, t, "dpm_solver") == (c0, c1 + cd * inv, -cd * inv)
    assert s._first_coefs(t0, t)["video"] == (_f(sg_t / sg_0), -_f(a_t * torch.expm1(-h)))
    assert s._x0_coefs(t) == (1.0 / _f(a_t), -_f(sg_t) / _f(a_t))


# ----------------------------------------------------------------------------- the selection, restated
@pytest.mark.parametrize("per", R.PER_CASES)
def test_multilevel_select_agrees_with_partition(per):
    for kind, q in itertools.product(R.INPUT_KINDS, R.Q_CASES):
        x = R.make_input(kind, 1, per)[0]
        got, bits = R.select(x, q)
        want32, want64 = R.reference(x, q)
        lo, hi, _ = R.ranks(per, q)
        assert bits == (R.partition_bits(x, lo), R.partition_bits(x, hi)), (kind, q)
        assert np.array_equal(np.array([got]).view(np.uint32), np.array([want32]).view(np.uint32)), (kind, q, got, want32)
        if np.isfinite(want64):      # the fp32 lerp is within one rounding of the float64 one
            assert abs(float(got) - want64) <= 2.0 ** -23 * abs(want64) + 1e-45, (kind, q, got, want64)


@pytest.mark.parametrize("defect", ["rank_off_by_one", "dropped_flush", "prefix_wrong_level"])
def test_seeded_defects_are_flagged(defect):
    flagged = 0
    for per, kind, q in itertools.product((R.CHUNK + 1, 3 * R.CHUNK + 5), ("normal_1", "share11"), (0.5, 0.995)):
        x = R.make_input(kind, 1, per)[0]
        lo, hi, _ = R.ranks(per, q)
        _, bits = R.select(x, q, defect=defect)
        flagged += bits != (R.partition_bits(x, lo), R.partition_bits(x, hi))
    assert flagged >= 4, (defect, flagged)


# ----------------------------------------------------------------------------- refused arguments
def test_sample_graph_names_what_it_refuses():
    from mm_diffusion._hip import MMDError
    s = _solver(True)
    cpu = {"video": torch.zeros(2, 8, 3, 16, 16), "audio": torch.zeros(2, 1, 512)}
    for kw, word in ((dict(order=3), "order"), (dict(method="singlestep"), "single-step"), (dict(method="adaptive"), "adaptive"),
                     (dict(solver_type="midpoint"), "solver_type"), (dict(steps=1, order=2), "steps")):
        with pytest.raises(MMDError, match=word):
            s.sample_graph(cpu, **dict(dict(steps=4), **kw))
    with pytest.raises(MMDError, match="CPU tensor"):
        s.sample_graph(cpu, steps=4)
    with pytest.raises(MMDError, match="taylor"):
        _solver(False).sample_graph(cpu, steps=4, solver_type="taylor")
    with pytest.raises(MMDError, match="CounterNoise"):
        s.sample_graph(cpu, steps=4, noise_source=lambda like: like)
    with pytest.raises(MMDError, match="model_kwargs"):
        _solver(True, model_kwargs={"y": 1}).sample_graph(cpu, steps=4)
    with pytest.raises(MMDError, match="x_T or shape"):
        s.sample_graph(steps=4)


def test_cpu_tensors_raise():
    from mm_diffusion import ops
    from mm_diffusion._hip import MMDError
    x, k, tab = torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(6, 4)
    with pytest.raises(MMDError, match="CPU tensor"):
        ops.dpmpp_x0(x, x, x.clone(), tab, k, 1, 1, 1, 8)
    with pytest.raises(MMDError, match="CPU tensor"):
        ops.dpmpp_update(x, x, x.clone(), tab, k, 1, 1, 1, 8)
    with pytest.raises(MMDError, match="CPU tensor"):
        ops.dpmpp_select(x, 0.5, torch.zeros(2), torch.zeros(2 * R.WS_WORDS, dtype=torch.int32))
