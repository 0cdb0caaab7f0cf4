"""Host side of the seeded, addressable samples (mm_diffusion/seeded.py): the Philox known answers, the C-ABI surface, the window shifts
and the statistics of the float64 emulation of every block of normals whose moments tests/test_seeded_gpu.py checks on the device."""
import random
import re
import os

import numpy as np
import pytest
import torch

import seeded_ref as R
from conftest import ROOT
from helpers import flags

SYMBOLS = ("mmd_ctr_fill", "mmd_ddpm_update_ctr", "mmd_ddim_update_ctr")


@pytest.mark.parametrize("counter,key,want", R.KNOWN)
def test_philox_known_answers(counter, key, want):
    from mm_diffusion.seeded import philox4x32_10
    assert philox4x32_10(counter, key) == want
    assert tuple(int(w) for w in R.philox(*counter, *key)) == want
    assert tuple(int(w[0]) for w in R.philox(*(np.array([c]) for c in counter), *key)) == want


def test_entry_points_are_declared_exported_and_bound():
    from mm_diffusion import _hip
    hdr, lib = open(os.path.join(ROOT, "include", "mmd.h")).read(), _hip.lib()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    # argument errors come back as codes before anything is launched (no GPU needed)
    assert lib.mmd_ctr_fill(None, 0, None, None, 0, 0, 0, 0, None) < 0 and b"ctr_fill" in lib.mmd_last_error()
    assert lib.mmd_ddpm_update_ctr(*([None] * 4), 0, *([None] * 6), 0, 0, 0, 0, 0, 0, None) < 0 and b"ddpm_update_ctr" in lib.mmd_last_error()
    assert lib.mmd_ddim_update_ctr(*([None] * 4), 0, *([None] * 5), 0, 0, 0, 0, 0, 0, 0.0, None) < 0 and b"ddim_update_ctr" in lib.mmd_last_error()


@pytest.fixture(scope="module")
def unet():
    from mm_diffusion import logger, multimodal_script_util as msu
    logger.set_quiet(True)
    model, diff = msu.create_model_and_diffusion(**flags("tiny", timestep_respacing="4"))
    assert diff.noise_source is None          # a fresh diffusion draws as before
    return model


def _ranges(unet):
    F = unet.video_size[0]
    return [F - layer["window"] for blk in unet._arch[0] + [unet._arch[1]] + unet._arch[2] for layer in blk
            if layer["kind"] == "cross" and layer["shift"]]


def test_shifts_are_in_range_and_depend_on_nothing_but_seed_and_index(unet):
    from mm_diffusion.seeded import CounterNoise, philox4x32_10
    hi = _ranges(unet)
    assert hi and len(hi) == len(unet.draw_shifts())
    a = CounterNoise(42)
    first = {i: a.shifts(i, unet) for i in range(40)}
    for i, s in first.items():
        assert len(s) == len(hi) and all(0 <= v <= h for v, h in zip(s, hi)), (i, s)
        # the stated mapping: word 0 of counter (j, i, 0, 3)
        assert s == [(philox4x32_10((j, i, 0, 3), (42, 0))[0] * (h + 1)) >> 32 for j, h in enumerate(hi)]
    # every admissible value of the widest range turns up over 40 draws of all blocks
    widest = max(hi)
    assert {s[j] for s in first.values() for j, h in enumerate(hi) if h == widest} == set(range(widest + 1))
    # any batch size / first sample / call history: the same sequence
    random.seed(1)
    [random.randint(0, 7) for _ in range(13)]
    unet.draw_shifts()
    torch.randn(5)
    for other in (CounterNoise(42, first_sample=96), CounterNoise(42, sample_ids=[5, 3, 1])):
        for i in reversed(range(40)):
            assert other.shifts(i, unet) == first[i]
    assert [CounterNoise(43).shifts(i, unet) for i in range(40)] != [first[i] for i in range(40)]
    # a seed's high word counts too
    assert [CounterNoise(42 + (1 << 32)).shifts(i, unet) for i in range(40)] != [first[i] for i in range(40)]


def test_counter_noise_on_cpu_tensors_raises():
    from mm_diffusion._hip import MMDError
    from mm_diffusion.seeded import CounterNoise
    src = CounterNoise(42)
    src.set_draw(3)
    with pytest.raises(MMDError):
        src(torch.zeros(2, 1, 512))
    with pytest.raises(MMDError):
        src.randn((2, 1, 512), 1, 3, device="cpu")
    with pytest.raises(MMDError):
        src.set_draw(torch.tensor([3, 2]))
    assert src.set_draw(torch.tensor([2, 2])) == 2
    for bad in (dict(first_sample=-1), dict(first_sample=2 ** 32), dict(sample_ids=[0, 2 ** 32]), dict(sample_ids=[-1])):
        with pytest.raises(MMDError):
            CounterNoise(42, **bad)
    with pytest.raises(MMDError):
        CounterNoise(2 ** 64)
    with pytest.raises(MMDError):
        CounterNoise(42, first_sample=2 ** 32 - 2).ids_list(3)          # the batch runs past the last id
    with pytest.raises(MMDError):
        CounterNoise(42, sample_ids=[1, 2]).ids_list(3)
    assert CounterNoise(7, first_sample=10).ids_list(3) == [10, 11, 12]
    assert CounterNoise(0x1234567890ABCDEF).key_words == (0x90ABCDEF, 0x12345678)          # low word first


def test_for_rank_addresses_disjoint_samples(monkeypatch):
    from mm_diffusion import dist_util
    from mm_diffusion.seeded import CounterNoise
    seen = []
    for rnd in range(2):
        for rank in range(3):
            monkeypatch.setattr(dist_util, "rank", lambda rank=rank: rank)
            monkeypatch.setattr(dist_util, "world_size", lambda: 3)
            seen += CounterNoise.for_rank(42, 4, round=rnd).ids_list(4)
    assert seen == list(range(24))


@pytest.mark.parametrize("block", R.BLOCKS + R.PARTNERS)
def test_emulated_normals_pass_the_moment_checks_at_4_sigma(block):
    """The float64 emulation of each block the GPU tests use: mean, variance, fourth moment and lag-1 correlation within 4 standard
    errors, so that the device's 5-sigma checks (fp32 values of the same words) cannot fail by chance."""
    z = R.normals(*block, R.NBLOCK)
    s = R.scores(z)
    print(block, {k: round(float(v), 2) for k, v in s.items()}, "max |z|", float(np.abs(z).max()))
    assert all(v <= 4.0 for v in s.values()), s
    assert np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2.0))


@pytest.mark.parametrize("a,b", list(zip(R.BLOCKS, R.PARTNERS)))
def test_emulated_blocks_are_uncorrelated_at_4_sigma(a, b):
    """Blocks that differ in the tag, the sample id (k, k + 1) or the draw (i, i + 1) alone."""
    c = R.corr_score(R.normals(*a, R.NBLOCK), R.normals(*b, R.NBLOCK))
    print(a, b, round(float(c), 2))
    assert c <= 4.0
