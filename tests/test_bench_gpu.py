"""bench.py's headline run on one GPU (`-m gpu`): a plain run times the steps and prints the line, `--full` adds the side measurements
after the timed steps, and `--dump-outputs` writes what the last timed step computed."""
import os

import numpy as np
import pytest
import torch

from test_multirank_gpu import _bench

pytestmark = pytest.mark.gpu


def test_plain_and_full_runs_dump_the_same_last_step(tmp_path):
    """Same arguments, a plain and a `--full` run: the plain line carries no roofline / breakdown / CPU baseline, the full one does;
    both dump the last timed step's x_{t-1} (bitwise the sample --dump-final saves) and U-Net prediction of both streams in float32.
    Across the two runs (seeded inputs; the side measurements come after the dump) they agree within the bf16 bound of the model
    tests: two processes are not always bitwise equal (seen at batch 4: one sample at bf16 rounding level).  A dump taken after the
    breakdown's eager replays would hold a later step and miss it by far."""
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2"]
    plain = _bench(*argv, "--dump-outputs", str(tmp_path / "plain"), "--dump-final", str(tmp_path / "final"))
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and abs(plain["value"] - 2 * 1000.0 / plain["ms_per_step"]) < 1e-6 * plain["value"]
    assert not {"roofline", "kernel_ms_per_step", "graded", "cpu_baseline"} & set(plain)
    full = _bench(*argv, "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert full["roofline"]["kernel"] and full["kernel_ms_per_step"] and "cpu_baseline" not in full
    names = ["audio", "eps_audio", "eps_video", "video"]
    assert sorted(f[:-len(".npy")] for f in os.listdir(tmp_path / "plain")) == names
    final = torch.load(tmp_path / "final" / "rank0.pt")
    for n in names:
        a, b = np.load(tmp_path / "plain" / f"{n}.npy"), np.load(tmp_path / "full" / f"{n}.npy")
        assert a.dtype == np.float32 and a.shape[0] == 2 and np.isfinite(a).all() and a.shape == b.shape, n
        assert np.linalg.norm(a - b) <= 2e-2 * np.linalg.norm(a), n
    for n in ("video", "audio"):
        assert np.array_equal(np.load(tmp_path / "plain" / f"{n}.npy"), final[n].numpy()), n
