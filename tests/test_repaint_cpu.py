"""Resampling jumps of masked sampling, the parts that need no GPU: the C ABI of mmd_ddpm_update_ctr_at / mmd_renoise_ctr, the schedule
(masking.repaint_schedule) against its restatement (repaint_ref.py), the draws, the refused arguments, the jump table's identities, the
float64 restatement of the jump checked against an fp32 emulation and two seeded defects, and the refusal of CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

import repaint_ref as R
import seeded_ref as S
from conftest import ROOT

SYMBOLS = ("mmd_ddpm_update_ctr_at", "mmd_renoise_ctr")


# ----------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_bound_and_exported():
    from mm_diffusion import _hip
    hdr = open(os.path.join(ROOT, "include", "mmd.h")).read()
    lib = _hip.lib()
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert name in _hip.EXPORTS and hasattr(lib, name)
        res, args = _hip._PROTOS[name]
        assert res is _hip.i32 and len(args) == len(params), (name, params)
        for p, a in zip(params, args):
            assert a is (_hip.vp if "*" in p else _hip.i32), (name, p)
        assert params[-1] == "void* stream"
        assert "const int64_t* draw" in params
    # the _at form is mmd_ddpm_update_ctr with the draws behind the timesteps
    base = re.search(r"\bint\s+mmd_ddpm_update_ctr\s*\(([^;]*)\)\s*;", hdr).group(1).replace("\n", " ")
    at = re.search(r"\bint\s+mmd_ddpm_update_ctr_at\s*\(([^;]*)\)\s*;", hdr).group(1).replace("\n", " ")
    norm = lambda s: [p.strip() for p in s.split(",")]      # noqa: E731
    assert [p for p in norm(at) if p != "const int64_t* draw"] == norm(base)
    assert norm(at)[norm(at).index("const int64_t* t") + 1] == "const int64_t* draw"
    # the header comment of mmd_ctr_fill names the new draws
    fill = hdr[hdr.index("Counter-based noise"):hdr.index("int mmd_ctr_fill(")]
    assert "0x80000000" in fill and "mmd_renoise_ctr" in fill and "mmd_ddpm_update_ctr_at" in fill


def test_null_arguments_are_refused_before_any_launch():
    from mm_diffusion import _hip
    lib = _hip.lib()
    rc = lib.mmd_ddpm_update_ctr_at(*([None] * 4), 0, *([None] * 7), 4, 1, 1, 1, 8, 0, None)
    assert rc < 0 and b"ddpm_update_ctr_at" in lib.mmd_last_error()
    rc = lib.mmd_renoise_ctr(None, None, None, 0, None, None, None, 4, 1, 1, 1, 8, None)
    assert rc < 0 and b"renoise_ctr" in lib.mmd_last_error()
    rc = lib.mmd_renoise_ctr(None, None, None, 0, None, None, None, 0, 1, 1, 1, 8, None)
    assert rc < 0 and b"renoise_ctr" in lib.mmd_last_error()


# ----------------------------------------------------------------------------- the schedule
def test_the_example_of_eight_steps():
    from mm_diffusion import masking
    s = masking.repaint_schedule(8, 2, 2)
    assert [i for op, i, _ in s if op == "step"] == [7, 6, 5, 6, 5, 4, 3, 4, 3, 2, 1, 2, 1, 0]
    assert [i for op, i, _ in s if op == "jump"] == [4, 2, 0]
    assert [d for op, _, d in s if op == "jump"] == [0x80000000, 0x80000001, 0x80000002]
    assert s[:6] == [("step", 7, 7), ("step", 6, 6), ("step", 5, 5), ("jump", 4, 0x80000000), ("step", 6, 14), ("step", 5, 13)]
    assert sum(op == "step" for op, _, _ in s) == 14 == R.evaluations(8, 2, 2)


def test_twenty_triples_against_the_restatement():
    from mm_diffusion import masking
    assert len(R.TRIPLES) == 20
    for T, J, U in R.TRIPLES:
        s = masking.repaint_schedule(T, J, U)
        assert s == R.schedule(T, J, U), (T, J, U)
        steps = [(i, d) for op, i, d in s if op == "step"]
        jumps = [(m, d) for op, m, d in s if op == "jump"]
        assert len(steps) == R.evaluations(T, J, U), (T, J, U)
        assert s[0] == ("step", T - 1, T - 1) and s[-1] == ("step", 0, 0)
        M = [m for m in range(T) if m % J == 0 and m + J <= T - 1]
        assert sorted(m for m, _ in jumps) == sorted(M * (U - 1)), (T, J, U)
        # the walk is a walk: a step goes one level down, a jump J levels up, and every jump leaves a level it may leave
        level = T - 1
        for op, i, _ in s:
            if op == "step":
                assert i == level
                level -= 1
            else:
                assert i == level and i in M
                level += J
        assert level == -1
        if U == 1:
            assert s == [("step", i, i) for i in range(T - 1, -1, -1)]
    for T in (1, 4, 250):
        plain = [("step", i, i) for i in range(T - 1, -1, -1)]
        assert masking.repaint_schedule(T) == plain and masking.repaint_schedule(T, None, 1) == plain
        assert masking.repaint_schedule(T, None, 3) == plain and masking.repaint_schedule(T, 1, 1) == plain
        assert masking.repaint_schedule(T, T + 5, 1) == plain          # a jump length that is never used is not refused


def test_draws_are_unique_below_the_x_T_draw_and_first_visits_draw_the_step():
    from mm_diffusion import masking
    for T, J, U in R.TRIPLES:
        s = masking.repaint_schedule(T, J, U)
        draws = [d for _, _, d in s]
        assert len(set(draws)) == len(draws), (T, J, U)
        assert all(0 <= d < 0xFFFFFFFF for d in draws), (T, J, U)
        seen = {}
        for op, i, d in s:
            if op == "step":
                r = seen.get(i, 0)
                assert d == i + r * T and d < 2 ** 31 and r < U, (T, J, U, i)
                seen[i] = r + 1
        assert sorted(seen) == list(range(T))
        assert [d for op, _, d in s if op == "jump"] == [0x80000000 + k for k in range(sum(op == "jump" for op, _, _ in s))]


@pytest.mark.parametrize("args,name", [
    ((8, 0, 2), "jump_length=0"),
    ((8, -3, 2), "jump_length=-3"),
    ((8, 2, 0), "n_resample=0"),
    ((8, 2, -1), "n_resample=-1"),
    ((8, None, 0), "n_resample=0"),
    ((8, 8, 2), "jump_length=8"),
    ((4, 9, 3), "jump_length=9"),
    ((1000, 10, 2 ** 31 // 1000 + 1), "n_resample=2147484"),
    ((2 ** 20, None, 2 ** 11), "n_resample=2048"),
])
def test_refused_schedule_arguments_are_named(args, name):
    from mm_diffusion import masking
    from mm_diffusion._hip import MMDError
    with pytest.raises(MMDError) as e:
        masking.repaint_schedule(*args)
    assert name in str(e.value), str(e.value)


def test_the_largest_accepted_resample_count():
    from mm_diffusion import masking
    from mm_diffusion._hip import MMDError
    T, U = 2 ** 16, 2 ** 15 - 1                                     # U T = 2^31 - 2^16: the bound is on the product, whatever the walk
    s = masking.repaint_schedule(T, None, U)
    assert len(s) == T and max(d for _, _, d in s) == T - 1
    with pytest.raises(MMDError):
        masking.repaint_schedule(T, None, U + 1)
    s = masking.repaint_schedule(8, 7, 1000)                        # one level, 999 jumps: the last visit of step 7 draws 7 + 999 * 8
    assert max(d for op, _, d in s if op == "step") == 7 + 999 * 8 and len(s) == 8 + 999 * 7 + 999


def test_the_loop_refuses_jump_arguments_before_anything_else():
    from mm_diffusion import multimodal_script_util as msu
    from mm_diffusion._hip import MMDError
    diff = msu.create_gaussian_diffusion(steps=1000, timestep_respacing="8")
    shape = {"video": (1, 8, 3, 16, 16), "audio": (1, 1, 512)}
    model = lambda v, a, t, **kw: (v, a)      # noqa: E731
    # not even `known` is looked at: a rejected jump argument raises first, and names the value
    for kw, name in ((dict(jump_length=0, n_resample=2), "jump_length=0"), (dict(jump_length=8, n_resample=2), "jump_length=8"),
                     (dict(jump_length=2, n_resample=0), "n_resample=0"), (dict(jump_length=2, n_resample=2, sampler="ddim"), "n_resample=2")):
        with pytest.raises(MMDError) as e:
            diff.masked_sample_loop(model, shape, None, device=torch.device("cuda"), **kw)
        assert name in str(e.value), str(e.value)
    with pytest.raises(TypeError):            # keyword-only
        diff.masked_sample_loop(model, shape, None, None, "ddpm", 0.0, None, True, None, None, False, True, True, None, 2, 2)
    # CPU tensors for a GPU run are refused with resampling as without
    with pytest.raises(MMDError):
        diff.masked_sample_loop(model, shape, {"video": torch.zeros(*shape["video"])}, device=torch.device("cuda"), jump_length=2, n_resample=2)


# ----------------------------------------------------------------------------- the jump table
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("respacing", ["", "250"])
def test_table_identities(schedule, respacing):
    from mm_diffusion import masking, multimodal_script_util as msu
    diff = msu.create_gaussian_diffusion(steps=1000, noise_schedule=schedule, timestep_respacing=respacing)
    ac = np.asarray(diff.alphas_cumprod, dtype=np.float64)
    T = len(ac)
    assert T == (250 if respacing else 1000)
    if not respacing:
        assert np.allclose(ac, R.alphas_cumprod(schedule, T), rtol=1e-12, atol=0)
    for J in (1, 10, T - 1):
        tab64 = masking.jump_table(ac, J)
        assert tab64.dtype == np.float64 and tab64.shape == (2, T)
        a64, b64 = R.jump_coef(ac, J)
        assert np.array_equal(tab64[0], a64) and np.array_equal(tab64[1], b64)
        assert not tab64[:, T - J:].any() and (tab64[0, :T - J] > 0).all()
        tab = tab64.astype(np.float32).astype(np.float64)          # what the kernel reads
        m = np.arange(T - J)
        a, b = tab[0, m], tab[1, m]
        lhs, rhs = a * np.sqrt(ac[m]), np.sqrt(ac[m + J])          # the mean: sqrt(ac[m]) x_0 becomes sqrt(ac[m + J]) x_0
        assert (np.abs(lhs - rhs) <= 1e-6 * rhs).all(), (schedule, respacing, J)
        lhs, rhs = a * a * (1.0 - ac[m]) + b * b, 1.0 - ac[m + J]  # the variance: 1 - ac[m] becomes 1 - ac[m + J]
        assert (np.abs(lhs - rhs) <= 1e-6 * rhs).all(), (schedule, respacing, J)
    # J = 1 is one forward diffusion step: a = sqrt(1 - beta), b = sqrt(beta)
    one = masking.jump_table(ac, 1)
    assert np.allclose(one[0, :T - 1], np.sqrt(1.0 - diff.betas[1:]), rtol=1e-12) and np.allclose(one[1, :T - 1], np.sqrt(diff.betas[1:]), rtol=1e-9)


# ----------------------------------------------------------------------------- the float64 restatement
SEED, TAG, T8, J8 = 42, 0, 8, 2


def _tab(T=1000, J=10):
    from mm_diffusion import masking
    return masking.jump_table(R.alphas_cumprod("linear", T), J).astype(np.float32)


def test_fp32_emulation_keeps_the_bound_on_every_gpu_shape():
    tab = _tab()
    T = tab.shape[1]
    worst = 0.0
    for shape in R.SHAPES:
        x, z = R.make_case(shape, seed=1)
        m = R.levels(shape[0], T, 10)
        y, bound = R.jump64(x, z, tab, m)
        for fused in (True, False):
            got = R.emulate32(x, z, tab, m, fused=fused)
            assert R.violations(got, y, bound) == 0, (shape, fused)
            worst = max(worst, float((np.abs(got.astype(np.float64) - y) / np.maximum(bound, 1e-300)).max()))
        # a level outside the table writes nothing
        bad = m.copy()
        bad[0] = T
        got = R.emulate32(x, z, tab, bad)
        assert np.array_equal(got[0], x[0]) and R.violations(got, *R.jump64(x, z, tab, bad)) == 0
    print("largest |err| / bound of the fp32 emulation:", worst)
    assert 0.0 < worst <= 1.0


def _counter_case(shape, draws, ids):
    N, F, C, HW = shape
    per = F * C * HW
    x, _ = R.make_case(shape, seed=3)
    z = np.stack([S.normals(SEED, ids[n], int(draws[n]), TAG, per) for n in range(N)]).astype(np.float32)
    return x, z


@pytest.mark.parametrize("defect", ["rows_swapped", "draw_from_m"])
def test_seeded_defects_are_flagged(defect):
    tab = _tab()
    shape = R.SHAPES[0]
    N = shape[0]
    ids = [7, 2 ** 32 - 1, 8]
    m = R.levels(N, tab.shape[1], 10)
    draws = np.array([0x80000000 + 5] * N, dtype=np.int64)
    x, z = _counter_case(shape, draws, ids)
    y, bound = R.jump64(x, z, tab, m)
    good = R.emulate32(x, z, tab, m)
    assert R.violations(good, y, bound) == 0
    if defect == "draw_from_m":                # seeded defect: the counter's draw word taken from the level, as the step kernels take it from t
        _, z_bad = _counter_case(shape, m, ids)
        bad = R.emulate32(x, z_bad, tab, m)
        y_bad, _ = R.jump64(x, z_bad, tab, m)
    else:
        bad = R.emulate32(x, z, tab, m, defect=defect)
        y_bad, _ = R.jump64(x, z, tab, m, defect=defect)
    n = R.violations(bad, y, bound)
    print(defect, "violations:", n, "of", y.size)
    assert n > y.size // 2
    assert not np.array_equal(y_bad, y)


# ----------------------------------------------------------------------------- no CPU fallback
def test_cpu_tensors_raise():
    from mm_diffusion import ops
    from mm_diffusion._hip import MMDError
    N, F, C, HW = 2, 1, 1, 8
    x = torch.zeros(N, C, HW)
    key, ids = torch.zeros(2, dtype=torch.int32), torch.zeros(N, dtype=torch.int64)
    jtab, tab = torch.zeros(2, 4), torch.zeros(7, 4)
    t = torch.zeros(N, dtype=torch.int64)
    with pytest.raises(MMDError):
        ops.renoise_ctr(x, key, ids, 1, jtab, t, t)
    with pytest.raises(MMDError):
        ops.ddpm_update_ctr_at(x, x, key, ids, 1, x, tab, t, t, F, C, HW, 0)
