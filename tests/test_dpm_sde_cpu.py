"""CPU-side checks of the stochastic multistep solver (SDE-DPM-Solver++, DPM_Solver.sample_graph_sde): the C ABI of
mmd_dpmpp_sde_update / mmd_dpmpp_sde_update_ctr, the two identities of its coefficients in float64 and on the fp32 tables of sde_tables
(bounds: tests/dpm_sde_ref.py), the tables against _sde_coefs, the refused arguments, and the restated kernel: its fp32 emulation keeps the
element-wise bound of every GPU case, every seeded defect breaks it, and the float64 emulation of the marginal-preservation case passes
the statistical check the GPU test applies to the kernel."""
import os
import re

import numpy as np
import pytest
import torch

import dpm_sde_ref as R
from conftest import ROOT

NEW = ("mmd_dpmpp_sde_update", "mmd_dpmpp_sde_update_ctr")


class _Model:
    video_out_channels, audio_out_channels = 3, 1


def _solver(kind="linear", predict_x0=True, **kw):
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    return DPM_Solver(_Model(), alphas_cumprod=torch.from_numpy(R.alphas_cumprod(kind)).float(), predict_x0=predict_x0, **kw)


# ----------------------------------------------------------------------------- C ABI
def test_symbols_in_header_binding_and_library():
    from mm_diffusion import _hip, ops
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _hip.EXPORTS and hasattr(_hip.lib(), name), name
    assert callable(ops.dpmpp_sde_update)
    # the draw convention stands next to the existing ones
    fill = hdr[hdr.index("Counter-based noise"):hdr.index("int mmd_ctr_fill(")]
    assert "mmd_dpmpp_sde_update_ctr" in fill and "k[n]" in fill


def test_bad_arguments_return_codes_and_name_the_entry():
    from mm_diffusion import _hip
    lib = _hip.lib()
    # non-NULL pointers that are never dereferenced (the checks run before any launch), far enough apart not to overlap
    x, m0, M1, nz, s, tab, cz, k, key, ids = (4096 * (i + 1) for i in range(10))
    mem, ctr = lib.mmd_dpmpp_sde_update, lib.mmd_dpmpp_sde_update_ctr

    def refused(f, who, word, *args):
        assert f(*args) < 0
        msg = lib.mmd_last_error()
        assert who + b":" in msg and word in msg, msg
    g = (4, 1, 1, 1, 1, 1, None)          # rows, N, F, C, Cm, HW, stream
    refused(mem, b"dpmpp_sde_update", b"M1", x, m0, None, nz, None, 1.0, tab, cz, k, *g)
    refused(mem, b"dpmpp_sde_update", b"cz", x, m0, M1, nz, None, 1.0, tab, None, k, *g)
    refused(mem, b"dpmpp_sde_update", b"noise", x, m0, M1, None, None, 1.0, tab, cz, k, *g)
    refused(mem, b"dpmpp_sde_update", b"max_val", x, m0, M1, nz, s, 0.0, tab, cz, k, *g)
    refused(mem, b"dpmpp_sde_update", b"2C", x, m0, M1, nz, None, 1.0, tab, cz, k, 4, 1, 1, 3, 5, 1, None)
    refused(mem, b"dpmpp_sde_update", b"rows", x, m0, M1, nz, None, 1.0, tab, cz, k, 0, 1, 1, 1, 1, 1, None)
    refused(mem, b"dpmpp_sde_update", b"overlap", x, m0, x, nz, None, 1.0, tab, cz, k, *g)
    refused(mem, b"dpmpp_sde_update", b"overlap", x, m0, M1, x + 4, None, 1.0, tab, cz, k, 4, 1, 1, 1, 1, 2, None)      # HW = 2: noise starts inside x
    refused(mem, b"dpmpp_sde_update", b"overlap", x, m0, M1, M1, None, 1.0, tab, cz, k, *g)
    refused(ctr, b"dpmpp_sde_update_ctr", b"M1", x, m0, None, key, ids, 0, None, 1.0, tab, cz, k, *g)
    refused(ctr, b"dpmpp_sde_update_ctr", b"cz", x, m0, M1, key, ids, 0, None, 1.0, tab, None, k, *g)
    refused(ctr, b"dpmpp_sde_update_ctr", b"key", x, m0, M1, None, ids, 0, None, 1.0, tab, cz, k, *g)
    refused(ctr, b"dpmpp_sde_update_ctr", b"tag", x, m0, M1, key, ids, 4, None, 1.0, tab, cz, k, *g)
    refused(ctr, b"dpmpp_sde_update_ctr", b"max_val", x, m0, M1, key, ids, 0, s, -1.0, tab, cz, k, *g)
    refused(ctr, b"dpmpp_sde_update_ctr", b"overlap", x, m0, x, key, ids, 0, None, 1.0, tab, cz, k, *g)


def test_cpu_tensors_and_noise_sources_raise():
    from mm_diffusion import ops
    from mm_diffusion._hip import MMDError
    x, k, tab, cz = torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64), torch.zeros(6, 4), torch.zeros(4)
    with pytest.raises(MMDError, match="CPU tensor"):
        ops.dpmpp_sde_update(x, x.clone(), x.clone(), tab, cz, k, 1, 1, 1, 8, noise=x.clone())
    with pytest.raises(MMDError, match="CPU tensor"):
        ops.dpmpp_sde_update(x, x.clone(), x.clone(), tab, cz, k, 1, 1, 1, 8, ctr=(torch.zeros(2, dtype=torch.int32), k.clone(), 0))
    with pytest.raises(MMDError, match="exactly one"):
        ops.dpmpp_sde_update(x, x.clone(), x.clone(), tab, cz, k, 1, 1, 1, 8)
    with pytest.raises(MMDError, match="exactly one"):
        ops.dpmpp_sde_update(x, x.clone(), x.clone(), tab, cz, k, 1, 1, 1, 8, noise=x.clone(), ctr=(k, k, 0))


def test_timing_tool_parses_its_arguments():
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dpm_sde_bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 0 and b"--repeats" in p.stdout and b"--out" in p.stdout, p.stdout


# ----------------------------------------------------------------------------- the identities
GRIDS = [(kind, skip, steps, order) for kind in ("linear", "cosine") for skip in ("logSNR", "time_uniform", "time_quadratic")
         for steps in (2, 5, 20) for order in (1, 2)]


@pytest.mark.parametrize("kind,skip,steps,order", GRIDS)
def test_identities_hold_in_float64(kind, skip, steps, order):
    worst = 0.0
    for a_s, s_s, a_t, s_t, (c0, c1, c2, cz) in R.schedule_rows64(R.Schedule64(R.alphas_cumprod(kind)), skip, steps, order):
        e1 = abs(c0 * a_s + c1 + c2 - a_t) / a_t
        e2 = abs(c0 ** 2 * s_s ** 2 + cz ** 2 - s_t ** 2) / s_t ** 2
        worst = max(worst, e1, e2)
        assert e1 <= 1e-12 and e2 <= 1e-12, (e1, e2)
    print(f"{kind} {skip} steps {steps} order {order}: largest relative residual {worst:.3e}")


@pytest.mark.parametrize("kind,skip,steps,order", GRIDS)
def test_identities_hold_for_the_tables_within_the_derived_bound(kind, skip, steps, order):
    sv = _solver(kind)
    tabs = sv.sde_tables(steps, order, skip, denoise=True)
    assert tabs["rows"] == steps + 1
    ts = tabs["timesteps"]
    grid = sv.get_time_steps(skip, sv.noise_schedule.T, 1. / sv.noise_schedule.total_N, steps, "cpu")
    assert torch.equal(ts[:steps], grid[:steps])
    worst = [0.0, 0.0]
    for i in range(steps):
        (lam_s, la_s, sig_s), (lam_t, la_t, sig_t) = (tuple(float(v[0]) for v in sc) for sc in sv._sc(grid[i:i + 1], grid[i + 1:i + 2]))
        a_s, a_t = np.exp(la_s), np.exp(la_t)
        for k in ("video", "audio"):
            c0, c1, c2 = (float(tabs["tab"][k][j, i]) for j in (2, 3, 4))
            cz = float(tabs["cz"][k][i])
            b1, b2 = R.table_bounds((c0, c1, c2, cz), a_s, a_t, sig_s, lam_s, lam_t, sig_t)
            r1, r2 = abs(c0 * a_s + c1 + c2 - a_t), abs(c0 ** 2 * sig_s ** 2 + cz ** 2 - sig_t ** 2)
            worst = [max(worst[0], r1 / b1), max(worst[1], r2 / b2)]
            assert r1 <= b1 and r2 <= b2, (i, k, r1, b1, r2, b2)
            assert cz > 0 and (c2 == 0) == (i == 0 or order == 1)
    print(f"{kind} {skip} steps {steps} order {order}: largest residual / bound  I1 {worst[0]:.3f}  I2 {worst[1]:.3f}")


@pytest.mark.parametrize("order,skip,steps,denoise", [(2, "logSNR", 5, True), (1, "time_uniform", 4, False), (2, "time_quadratic", 20, True),
                                                      (2, "logSNR", 2, False)])
def test_table_rows_are_the_scalars_of_sde_coefs(order, skip, steps, denoise):
    from mm_diffusion import ops
    sv = _solver()
    tabs = sv.sde_tables(steps, order, skip, denoise=denoise)
    det = sv.graph_tables(steps, order, skip, "dpm_solver", denoise)
    assert tabs["rows"] == steps + (1 if denoise else 0) == det["rows"] and tabs["tm"] == det["tm"]
    assert torch.equal(tabs["timesteps"], det["timesteps"]) and np.array_equal(tabs["tab2"], det["tab2"])
    grid = sv.get_time_steps(skip, sv.noise_schedule.T, 1. / sv.noise_schedule.total_N, steps, "cpu")
    for i in range(steps):
        second = order == 2 and i > 0
        want = sv._sde_coefs(grid[i - 1:i] if second else None, grid[i:i + 1], grid[i + 1:i + 2])
        assert all(isinstance(v, float) and v == float(np.float32(v)) for v in want), "each coefficient is rounded to fp32 once"
        for k in ("video", "audio"):
            row = tabs["tab"][k][:, i]
            got = (float(row[2]), float(row[3]), float(row[4]), float(tabs["cz"][k][i]))
            assert got == want, (i, k, got, want)
            assert int(row[5]) == (ops.DPMPP_KIND_SECOND if second else ops.DPMPP_KIND_FIRST)
            assert (row[0], row[1]) == (det["tab"][k][0, i], det["tab"][k][1, i]), "cx, ce are graph_tables'"
    if denoise:
        for k in ("video", "audio"):
            assert int(tabs["tab"][k][5, steps]) == ops.DPMPP_KIND_DENOISE == R.DENOISE and tabs["cz"][k][steps] == 0
            assert np.array_equal(tabs["tab"][k][:, steps], det["tab"][k][:, steps])
    assert tabs["cz"]["video"].dtype == np.float32 and tabs["cz"]["video"].shape == (tabs["rows"],)
    assert sv.sde_tables(steps, order, skip, denoise=denoise) is tabs, "the tables are kept per argument set"
    assert sv.graph_tables(steps, order, skip, "dpm_solver", denoise) is det, "graph_tables keeps its own"


# ----------------------------------------------------------------------------- refused arguments
def test_every_refusal_names_what_it_refuses():
    from mm_diffusion._hip import MMDError
    from mm_diffusion.seeded import CounterNoise
    s = _solver()
    cpu = {"video": torch.zeros(2, 8, 3, 16, 16), "audio": torch.zeros(2, 1, 512)}
    shape = {k: tuple(v.shape) for k, v in cpu.items()}
    for kw, word in ((dict(order=3), "order"), (dict(order=0), "order"), (dict(steps=1, order=2), "steps")):
        with pytest.raises(MMDError, match=word):
            s.sample_graph_sde(cpu, **dict(dict(steps=4), **kw))
        with pytest.raises(MMDError, match=word):
            s.sde_tables(**dict(dict(steps=4), **kw))
        with pytest.raises(MMDError, match=word):
            s.sample(cpu, method="multistep_sde", **dict(dict(steps=4, order=2), **kw))
    for fn in (lambda sv: sv.sample_graph_sde(cpu, steps=4), lambda sv: sv.sde_tables(4), lambda sv: sv.sample(cpu, steps=4, order=2, method="multistep_sde")):
        with pytest.raises(MMDError, match="predict_x0.*marginal"):
            fn(_solver(predict_x0=False))
    with pytest.raises(MMDError, match="solver_type.*'taylor'"):
        s.sample(cpu, steps=4, order=2, method="multistep_sde", solver_type="taylor")
    with pytest.raises(MMDError, match="model_kwargs"):
        _solver(model_kwargs={"y": 1}).sample_graph_sde(cpu, steps=4)
    with pytest.raises(MMDError, match="x_T must be None"):
        s.sample_graph_sde(cpu, steps=4, noise_source=CounterNoise(1))
    with pytest.raises(MMDError, match="CounterNoise"):
        s.sample_graph_sde(cpu, steps=4, noise_source=lambda like: like)
    with pytest.raises(MMDError, match="CounterNoise"):
        s.sample(cpu, steps=4, order=2, method="multistep_sde", noise_source=lambda like: like)
    with pytest.raises(MMDError, match="no MultimodalUNet"):
        s.sample_graph_sde(shape=shape, steps=4)
    with pytest.raises(MMDError, match="x_T or shape"):
        s.sample_graph_sde(steps=4)
    with pytest.raises(MMDError, match="CPU tensor"):
        s.sample_graph_sde(cpu, steps=4)
    with pytest.raises(MMDError, match="CPU tensor"):
        s.sample(cpu, steps=4, order=2, method="multistep_sde")
    # a noise source makes no sense for the deterministic methods, and the deterministic graph loop still refuses other methods
    with pytest.raises(MMDError, match="noise_source.*multistep_sde"):
        s.sample(cpu, steps=4, order=2, method="multistep", noise_source=CounterNoise(1))
    with pytest.raises(MMDError, match="only method 'multistep'"):
        s.sample_graph(cpu, steps=4, method="multistep_sde")
    # the SR stage's tensor-valued solver has no graph form and no stochastic method
    from mm_diffusion.dpm_solver_plus import DPM_Solver as SRSolver
    sr = SRSolver(_Model(), alphas_cumprod=torch.from_numpy(R.alphas_cumprod("linear")).float(), predict_x0=True)
    with pytest.raises(MMDError, match="multimodal"):
        sr.sample(torch.zeros(2, 3, 8, 8), steps=4, order=2, method="multistep_sde")


# ----------------------------------------------------------------------------- the restated kernel
def _z32(case_k, tag):
    return R.counter_noise64(case_k, tag).astype(np.float32)


@pytest.mark.parametrize("cmf,with_s", R.CASES)
def test_fp32_emulation_keeps_the_bound_on_every_gpu_case(cmf, with_s):
    c = R.make_case(cmf, with_s)
    for k in R.K_CASES + [(0, 4, -1)]:
        z = _z32(k, 0)
        want, m1w, by, bm = R.update64(c["x"], c["m0raw"], c["m1"], z, c["tab"], c["cz"], k, c["s"], c["max_val"])
        got, m1g = R.emulate32(c["x"], c["m0raw"], c["m1"], z, c["tab"], c["cz"], k, c["s"], c["max_val"])
        margin = float((np.abs(got.astype(np.float64) - want) / np.maximum(by, 1e-300)).max())
        print(f"Cm {cmf}C s {with_s} k {k}: largest error / bound {margin:.3f}")
        assert R.violations(got, want, by) == 0 and R.violations(m1g, m1w, bm) == 0, k
        if not with_s:
            assert np.array_equal(m1g.astype(np.float64), m1w), "without thresholding the history is exact"
    # a k outside the table writes nothing
    got, m1g = R.emulate32(c["x"], c["m0raw"], c["m1"], z, c["tab"], c["cz"], (0, 4, -1), c["s"], c["max_val"])
    assert np.array_equal(got[1:], c["x"][1:]) and np.array_equal(m1g[1:], c["m1"][1:]) and not np.array_equal(got[0], c["x"][0])


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_are_flagged_by_the_bound(defect):
    flagged = 0
    for cmf, with_s in R.CASES:
        c = R.make_case(cmf, with_s)
        for k in R.K_CASES:
            z = _z32(k, 1)
            z_k0 = _z32((k[0],) * R.N, 1)
            want, m1w, by, bm = R.update64(c["x"], c["m0raw"], c["m1"], z, c["tab"], c["cz"], k, c["s"], c["max_val"])
            got, m1g = R.emulate32(c["x"], c["m0raw"], c["m1"], z, c["tab"], c["cz"], k, c["s"], c["max_val"], defect=defect, z_k0=z_k0)
            flagged += (R.violations(got, want, by) + R.violations(m1g, m1w, bm)) > 0
    print(f"{defect}: flagged in {flagged} of {len(R.CASES) * len(R.K_CASES)} runs")
    assert flagged > 0, defect


def test_float64_emulation_of_the_marginal_case_passes_the_statistical_check():
    m = R.marginal_case()
    zm, zv = R.marginal_scores(m["want"], m["mu"], m["alpha_t"], m["sigma_t"])
    print(f"float64 emulation: mean off by {zm:.2f} se, variance by {zv:.2f} se; largest carried bound {m['bound'].max():.3e}")
    assert zm <= 5.0 and zv <= 5.0
    # the bound stays far below the scale the statistics resolve: sigma_t / sqrt(n)
    assert m["bound"].max() < m["sigma_t"] / np.sqrt(m["want"].size)
    # the table-driven loop, restated, gives the same trajectory
    import seeded_ref as S
    got = R.run({"rows": R.M_ROWS, "tab": {"video": m["tab"]}, "cz": {"video": m["cz"]}}, lambda x, i: m["mu"], m["x0"],
                lambda i: np.stack([S.normals(R.M_SEED, sid, i, R.M_TAG, R.PER) for sid in R.M_IDS]))
    assert np.allclose(got, m["want"], rtol=0, atol=1e-13)
