"""CPU-side checks of the SR training surface: the import surface of the reference's py_scripts/image_sr_train.py resolves against this
package, the image loader keeps the generator contract, the widened backward entry points report their limits as error codes, and the
built head-width-192 attention backward kernels use no scratch memory.

The names below are restated as data (what `py_scripts/image_sr_train.py:5-18` imports and the keywords its `TrainLoop(...)` call passes,
`:38-58`); the script's text is not kept here."""
import importlib
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SR_TRAIN_SCRIPT_IMPORTS = {
    "mm_diffusion": ["dist_util", "logger"],
    "mm_diffusion.real_image_datasets": ["load_data"],
    "mm_diffusion.resample": ["create_named_schedule_sampler"],
    "mm_diffusion.common": ["set_seed_logger_random"],
    "mm_diffusion.script_util": ["image_sr_model_and_diffusion_defaults", "image_sr_create_model_and_diffusion", "args_to_dict",
                                 "add_dict_to_argparser"],
    "mm_diffusion.train_util": ["TrainLoop"],
}
TRAINLOOP_KEYWORDS = ["model", "diffusion", "data", "batch_size", "microbatch", "lr", "ema_rate", "log_interval", "save_interval",
                      "resume_checkpoint", "use_fp16", "fp16_scale_growth", "schedule_sampler", "weight_decay", "lr_anneal_steps", "use_db",
                      "save_type", "class_cond", "sample_fn"]
LOAD_DATA_KEYWORDS = ["data_dir", "batch_size", "image_size", "class_cond", "num_workers"]


def test_sr_train_script_import_surface_resolves():
    for mod, names in SR_TRAIN_SCRIPT_IMPORTS.items():
        m = importlib.import_module(mod)
        for n in names:
            obj = getattr(m, n, None)
            if obj is None:
                obj = importlib.import_module(f"{mod}.{n}")
            assert obj is not None, f"{mod}.{n}"
    from mm_diffusion.real_image_datasets import load_data
    from mm_diffusion.train_util import TrainLoop
    have = inspect.signature(TrainLoop.__init__).parameters
    assert [k for k in TRAINLOOP_KEYWORDS if k not in have] == []
    have = inspect.signature(load_data).parameters
    assert [k for k in LOAD_DATA_KEYWORDS if k not in have] == []
    from mm_diffusion.gaussian_diffusion import GaussianDiffusion
    assert list(inspect.signature(GaussianDiffusion.training_losses).parameters) == ["self", "model", "x_start", "t", "model_kwargs", "noise"]
    # the multimodal loop is the shared machinery, not a copy
    from mm_diffusion import multimodal_train_util
    assert issubclass(TrainLoop, multimodal_train_util.TrainLoop) and TrainLoop.save is multimodal_train_util.TrainLoop.save


def _check_batch(lr, hr, sr, cond, B, L):
    assert cond == {} and lr.shape == (B, 3, L // 4, L // 4) and hr.shape == (B, 3, L, L) and sr.shape == (B, 3, L, L)
    for t in (lr, hr, sr):
        assert t.dtype == torch.float32 and float(t.min()) >= -1 and float(t.max()) <= 1
    area = torch.nn.functional.avg_pool2d(hr, 4)
    assert torch.allclose(lr, area, atol=1e-6)                     # lr is the area average of hr
    assert torch.equal(sr[:, :, ::4, ::4], lr) and torch.equal(sr[:, :, 3::4, 3::4], lr)


def test_load_data_synthetic_and_npz(tmp_path, monkeypatch):
    from mm_diffusion import dist_util
    from mm_diffusion.real_image_datasets import load_data
    it = load_data(data_dir="synthetic", batch_size=3, image_size=32)
    _check_batch(*next(it), 3, 32)
    _check_batch(*next(it), 3, 32)
    rng = np.random.default_rng(0)
    imgs = rng.integers(0, 256, size=(6, 16, 16, 3), dtype=np.uint8)
    for i in range(4):
        np.savez(tmp_path / f"img{i}.npz", image=imgs[i])
    np.save(tmp_path / "img4.npy", (np.transpose(imgs[4], (2, 0, 1)).astype(np.float32) / 127.5 - 1))
    np.savez(tmp_path / "img5.npz", images=imgs[5:6])
    it = load_data(data_dir=str(tmp_path), batch_size=2, image_size=16, deterministic=True)
    seen = []
    for _ in range(3):
        lr, hr, sr, cond = next(it)
        _check_batch(lr, hr, sr, cond, 2, 16)
        seen.append(hr)
    got = torch.cat(seen)
    want = torch.from_numpy(np.transpose(imgs, (0, 3, 1, 2)).astype(np.float32) / 127.5 - 1)
    assert torch.allclose(got, want, atol=1e-6)                    # deterministic: sorted file order, no flip
    # rank sharding: rank r of 2 sees files r, r + 2, r + 4 of the sorted list
    monkeypatch.setattr(dist_util, "world_size", lambda: 2)
    for r in (0, 1):
        monkeypatch.setattr(dist_util, "rank", lambda r=r: r)
        it = load_data(data_dir=str(tmp_path), batch_size=3, image_size=16, deterministic=True)
        assert torch.allclose(next(it)[1], want[r::2], atol=1e-6)
    with pytest.raises(ValueError):
        next(load_data(data_dir=str(tmp_path), batch_size=2, image_size=32))          # images are 16 x 16: no resampling here
    with pytest.raises(ValueError):
        next(load_data(data_dir="", batch_size=2, image_size=16))


def test_widened_entry_points_report_their_limits():
    """Width / channel checks come before any launch: error code + a message naming the limit, with otherwise valid dummy arguments."""
    import ctypes as C
    from mm_diffusion import _hip
    lib = _hip.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fp = C.cast(buf, C.POINTER(C.c_float))
    rc = lib.mmd_attn_bwd_mfma(p, 600, 0, p, 600, 200, 400, p, 200, p, 200, p, 600, 0, p, 600, 200, 400, fp, fp, 1, 200, 1, 1, 64, 64, 64, 64, 1,
                               None, None)
    msg = lib.mmd_last_error()
    assert rc < 0 and b"attn_bwd_mfma" in msg and b"200" in msg and b"192" in msg, msg
    rc = lib.mmd_attn_bwd(1, p, 600, 0, p, 600, 200, 400, p, 200, p, 200, p, 600, 0, p, 600, 200, 400, fp, fp, 1, 200, 1, 1,
                          1, 64, 1, 1, 64, 64, 1, 64, 1, 1, 64, 64, 1, None, None)
    msg = lib.mmd_last_error()
    assert rc < 0 and b"attn_bwd" in msg and b"200" in msg and b"192" in msg, msg
    for entry in (lib.mmd_gn_bwd, lib.mmd_gn_bwd_ws0):
        rc = entry(1, p, 4096, p, 4096, p, 4096, 64, 4096, 1, 64, 1, 64, 64, 1, fp, fp, fp, fp, fp, None, 0, 1, fp, fp, None, 0, fp, None)
        msg = lib.mmd_last_error()
        assert rc < 0 and b"gn_bwd" in msg and b"4096" in msg and b"2048" in msg, msg


def _kernel_table(obj, llvm):
    with tempfile.TemporaryDirectory() as d:
        os.symlink(os.path.abspath(obj), os.path.join(d, "k.o"))
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = [f for f in os.listdir(d) if "gfx950" in f][0]
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=d, check=True, capture_output=True, text=True).stdout
    rows = {}
    for blk in re.split(r"\n\s+- \.agpr_count", "\n" + notes)[1:]:
        g = lambda k: int(re.search(r"\." + k + r":\s+(\S+)", blk).group(1))      # noqa: E731
        name = re.search(r"\.name:\s+(\S+)", blk).group(1).strip("'")
        rows[name] = dict(vgpr=g("vgpr_count"), agpr=int(re.match(r":\s+(\S+)", blk).group(1)), spill=g("vgpr_spill_count"),
                          scratch=g("private_segment_fixed_size"))
    return rows


# vgpr_count (VGPRs + AGPRs, as the code-object notes report it) of the instances that existed before head width 192: they must not move
MFMA_BWD_VGPRS = {"dq": {16: 115, 32: 123, 48: 136, 64: 153, 96: 268, 128: 300}, "dkv": {16: 170, 32: 178, 48: 233, 64: 240, 96: 380, 128: 486}}


def test_head_width_192_attention_backward_kernels_use_no_scratch():
    """The built mmd_attn_bwd_mfma.o (tools/kernel_regs.py reads the same notes): both <192> kernels exist with private_segment_fixed_size 0
    and vgpr_spill_count 0 - the one-workgroup dK / dV form at 192 spills 116+ registers, the two-halves form must not - and the instances
    for {16 ... 128} keep their register counts."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mmd_build", os.path.join(ROOT, "mm-diffusion_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    obj = os.path.join(ROOT, "mm-diffusion_amd", "lib", "mmd_attn_bwd_mfma.o")
    if not os.path.exists(obj):
        bld.build(force=True, verbose=False)
    rows = _kernel_table(obj, bld._llvm_bin())
    dq = {int(m.group(1)): v for k, v in rows.items() for m in [re.match(r"_Z23attn_bwd_dq_mfma_kernelILi(\d+)EEv", k)] if m}
    dkv = {int(m.group(1)): (int(m.group(2) or 1), v) for k, v in rows.items()
           for m in [re.match(r"_Z24attn_bwd_dkv_mfma_kernelILi(\d+)E(?:Li(\d+)E)?Ev", k)] if m}
    print("attn_bwd_mfma kernels:", {("dq", d): v for d, v in sorted(dq.items())}, {("dkv", d): v for d, v in sorted(dkv.items())})
    assert sorted(dq) == sorted(dkv) == [16, 32, 48, 64, 96, 128, 192]
    for d in dq:
        assert dq[d]["spill"] == 0 and dq[d]["scratch"] == 0, (d, dq[d])
        assert dkv[d][1]["spill"] == 0 and dkv[d][1]["scratch"] == 0, (d, dkv[d])
    assert dkv[192][0] == 2 and all(dkv[d][0] == 1 for d in dkv if d != 192)          # 192: two 96-column halves
    assert dq[192]["vgpr"] <= 512 and dkv[192][1]["vgpr"] <= 512
    for d, n in MFMA_BWD_VGPRS["dq"].items():
        assert dq[d]["vgpr"] == n, ("dq", d, dq[d])
    for d, n in MFMA_BWD_VGPRS["dkv"].items():
        assert dkv[d][1]["vgpr"] == n, ("dkv", d, dkv[d])
