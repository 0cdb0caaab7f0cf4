"""Host side of the training step guard (on-device gradient / parameter norms, non-finite skip, clipping): the C-ABI surface, the
control block's layout, the static chunk table, the unguarded CPU-tensor path of FlatAdamW and the video / audio / shared naming rule."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import gold

SYMBOLS = ("mmd_sumsq_chunks", "mmd_step_control", "mmd_adamw_step_guarded")


def _header():
    return open(os.path.join(ROOT, "include", "mmd.h")).read()


def test_entry_points_are_declared_exported_and_bound():
    from mm_diffusion import _hip
    hdr, lib = _header(), _hip.lib()
    declared = set(re.findall(r"\b(mmd_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS + ("mmd_step_ctrl_bytes",):
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    # argument errors come back as codes before anything is launched (no GPU needed)
    assert lib.mmd_sumsq_chunks(None, None, 0, None, None, 0, None, None) < 0 and b"sumsq_chunks" in lib.mmd_last_error()
    assert lib.mmd_step_control(None, None, 0, None, 0.0, 0.9, 0.999, None, None) < 0 and b"step_control" in lib.mmd_last_error()
    assert lib.mmd_adamw_step_guarded(*([None] * 8), 0.0, 0.0, 0.0, 0.0, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, None) < 0
    assert b"adamw_step_guarded" in lib.mmd_last_error()


def test_control_block_layout_agrees_with_the_header():
    """sizeof(struct mmd_step_ctrl) as the library was compiled against the host's ctypes view; field order and C types against the
    header text; the chunk length constant."""
    from mm_diffusion import _hip, optim
    size = _hip.lib().mmd_step_ctrl_bytes()
    assert size == ctypes.sizeof(optim.StepCtrl) and size <= 128
    body = re.search(r"struct mmd_step_ctrl \{(.*?)\n\};", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"\b(double|float|int64_t|int32_t)\s+([a-z0-9_, ]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    cmap = {"double": ctypes.c_double, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [(n, cmap[c]) for n, c in fields] == list(optim.StepCtrl._fields_)
    for name in ("grad_norm", "param_norm", "took_step", "clip_coef", "steps_taken", "bc1", "bc2", "skipped_total", "first_bad_param",
                 "cum_grad_norm", "cum_param_norm", "cum_count"):
        assert hasattr(optim.StepCtrl, name), name
    assert int(re.search(r"#define MMD_STEP_CHUNK (\d+)", _header()).group(1)) == optim.STEP_CHUNK
    assert int(re.search(r"#define MMD_STEP_MAX_EMA (\d+)", _header()).group(1)) == optim.MAX_GUARD_EMA


def _check_table(sizes, L):
    from mm_diffusion.optim import chunk_table
    lo, ln, first = chunk_table(sizes, L)
    n, P = sum(sizes), len(sizes)
    assert lo.dtype == np.int64 and ln.dtype == np.int32 and first.dtype == np.int32
    assert len(lo) == len(ln) and len(first) == P + 1
    assert (ln > 0).all() and (ln <= L).all()                                   # none exceeds the chunk length (none is empty)
    assert lo[0] == 0 and (lo[1:] == lo[:-1] + ln[:-1]).all() and lo[-1] + ln[-1] == n      # chunks tile [0, n) exactly, in order
    assert first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] == len(lo)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    for i in range(P):                                                          # parameter i's chunks cover exactly parameter i
        c0, c1 = first[i], first[i + 1]
        assert c1 - c0 == -(-sizes[i] // L)
        assert lo[c0] == bounds[i] and lo[c1 - 1] + ln[c1 - 1] == bounds[i + 1]


def test_chunk_table_on_random_parameter_lists():
    from mm_diffusion.optim import STEP_CHUNK
    rng = np.random.default_rng(7)
    for case in range(20):
        L = STEP_CHUNK if case % 2 == 0 else int(rng.integers(2, 300))
        special = [1, L - 1, L, L + 1, 2 * L, 2 * L + 1]
        k = int(rng.integers(1, 40))
        sizes = [int(rng.choice(special)) if rng.random() < 0.4 else int(rng.integers(1, 3 * L)) for _ in range(k)]
        if case == 0:
            sizes = [1]
        if case == 1:
            sizes = [1, 1, L - 1, L, L + 1, 1]
        _check_table(sizes, L)
    _check_table([1, 3, 255, 256, 257, 4093, STEP_CHUNK, STEP_CHUNK + 1, 70001], STEP_CHUNK)


def test_flat_adamw_on_cpu_tensors_is_unguarded_and_guard_raises(monkeypatch):
    from mm_diffusion import _hip
    from mm_diffusion.optim import FlatAdamW

    def no_library():
        raise AssertionError("FlatAdamW on CPU tensors must not load the library")
    monkeypatch.setattr(_hip, "lib", no_library)
    params = [torch.nn.Parameter(torch.randn(s)) for s in (40, 17, 3, 5)]
    opt = FlatAdamW(params, lr=1e-3, grad_buckets=2)
    assert not opt.guard and len(opt.buckets) == 2 and opt.buckets[0][0] == 0 and opt.buckets[-1][1] == 65
    assert opt.steps == 0 and isinstance(opt.steps, int)
    opt.steps = 7
    assert opt.steps == 7 and isinstance(opt.steps, int)
    with pytest.raises(_hip.MMDError):
        FlatAdamW([torch.nn.Parameter(torch.randn(4))], guard=True)
    with pytest.raises(_hip.MMDError):
        opt.read_control()


def test_both_train_loops_take_the_guard_arguments():
    from mm_diffusion import multimodal_train_util as mtu, train_util as tu
    for cls in (mtu.TrainLoop, tu.TrainLoop):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["guard_nonfinite"].default is True and sig["max_grad_norm"].default == 0.0, cls
    assert mtu.TrainLoop.log_stream_norms and not tu.TrainLoop.log_stream_norms


def test_every_parameter_name_is_in_exactly_one_group():
    from mm_diffusion.multimodal_train_util import param_group
    names = [str(n) for n in gold("full_train_grads")["names"]]
    assert len(names) == 1046
    is_audio = lambda n: any(c.startswith("audio_") or c in ("a_norm", "a_qkv") for c in n.split("."))      # noqa: E731
    is_video = lambda n: any(c.startswith("video_") or c in ("spatial_attention_block", "temporal_attention_block", "v_norm", "v_qkv")
                             for c in n.split("."))                                                          # noqa: E731
    groups = {"video": [], "audio": [], "shared": []}
    for n in names:
        assert not (is_audio(n) and is_video(n)), n               # the two rules never both match: no tie to break
        want = "audio" if is_audio(n) else ("video" if is_video(n) else "shared")
        assert param_group(n) == want, n
        groups[want].append(n)
    assert all(groups.values()) and sum(len(v) for v in groups.values()) == len(names)
    assert all(n.startswith("time_embed") or ".emb_layers." in n for n in groups["shared"]), groups["shared"][:5]
