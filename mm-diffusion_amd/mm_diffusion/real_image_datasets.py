"""`load_data` for py_scripts/image_sr_train.py (reference real_image_datasets.py:12-75,157-186 reads jpg / png files with PIL and
resizes / degrades them with OpenCV: dataset IO and augmentation, out of the hot path; OpenCV is not used here).  This counterpart
keeps the generator contract - `yield (lr [B, 3, S, S], hr [B, 3, L, L], sr [B, 3, L, L], {})` floats in [-1, 1] forever, rank-sharded,
S = L / 4 - over PRE-EXTRACTED images: every `*.npy` (one image, uint8 [L, L, 3] or float [3, L, L]) and `*.npz` (array `image`, or
`images` = a stack of them) under `data_dir` (comma-separated directories like the reference), plus jpg / jpeg / png files when PIL
is importable (they must already be L x L: this loader does not resize).  `data_dir="synthetic"` yields random images (smoke training).

lr is the 4 x 4 area average of hr and sr its nearest-neighbour upsample back to L x L (the reference: bicubic both ways, with random
Gaussian-noise / JPEG degradations of lr in between - augmentation that stays out; the model itself upsamples `low_res` bilinearly and
never sees `sr`, which only feeds the sample dump).  `random_crop` is accepted and ignored (the reference ignores it too);
`class_cond=True` is not built."""
import glob
import os

import numpy as np
import torch as th

from . import dist_util

SCALE = 4          # large_size / small_size of the shipped stage (reference real_image_datasets.py:168-171: 256 -> 64 -> 256)


def _as_chw(a, path):
    a = np.asarray(a)
    if a.dtype == np.uint8:
        a = np.transpose(a, (2, 0, 1)).astype(np.float32) / 127.5 - 1
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[0] != 3 or a.shape[1] != a.shape[2]:
        raise ValueError(f"{path}: expected one square RGB image (uint8 [L, L, 3] or float [3, L, L]), got {a.shape}")
    return a


def _read(path):
    """-> list of float32 [3, L, L] arrays in [-1, 1]."""
    ext = path.rsplit(".", 1)[-1].lower()
    if ext == "npy":
        return [_as_chw(np.load(path), path)]
    if ext == "npz":
        z = np.load(path)
        if "image" in z:
            return [_as_chw(z["image"], path)]
        if "images" in z:
            return [_as_chw(a, path) for a in z["images"]]
        raise ValueError(f"{path}: no `image` / `images` array")
    from PIL import Image
    with Image.open(path) as im:
        return [_as_chw(np.array(im.convert("RGB")), path)]


def _list_files(data_dir, frame_gap=1):
    exts = ["npy", "npz"]
    try:
        import PIL  # noqa: F401
        exts += ["jpg", "jpeg", "png"]
    except ImportError:
        pass
    out = []
    for d in data_dir.split(","):
        found = sorted(f for f in glob.glob(os.path.join(d, "**", "*.*"), recursive=True) if f.rsplit(".", 1)[-1].lower() in exts)
        out.extend(found[::max(1, int(frame_gap))])
    return out


def degrade(hr):
    """hr [B, 3, L, L] -> (lr [B, 3, L/4, L/4] area average, sr [B, 3, L, L] nearest upsample of lr)."""
    B, C, L, _ = hr.shape
    lr = hr.reshape(B, C, L // SCALE, SCALE, L // SCALE, SCALE).mean(dim=(3, 5))
    sr = lr.repeat_interleave(SCALE, dim=2).repeat_interleave(SCALE, dim=3)
    return lr, sr


def load_data(*, data_dir, batch_size, image_size, class_cond=False, deterministic=False, random_crop=False, random_flip=True,
              num_workers=0, frame_gap=1):
    if not data_dir:
        raise ValueError("unspecified data directory")
    if class_cond:
        raise NotImplementedError("class-conditional SR training is not built")
    if image_size % SCALE:
        raise ValueError(f"image_size {image_size} must be a multiple of {SCALE}")
    _ = random_crop, num_workers
    if data_dir == "synthetic":
        g = th.Generator().manual_seed(1234 + dist_util.rank())
        while True:
            hr = th.rand(batch_size, 3, image_size, image_size, generator=g) * 2 - 1
            lr, sr = degrade(hr)
            yield lr, hr, sr, {}
    files = _list_files(data_dir, frame_gap)[dist_util.rank()::dist_util.world_size()]
    if not files:
        raise ValueError(f"no pre-extracted *.npy / *.npz images (or image files readable by PIL) under {data_dir}")
    rng = np.random.default_rng(None if not deterministic else 0)
    pending = []
    while True:
        order = np.arange(len(files)) if deterministic else rng.permutation(len(files))
        for j in order:
            for a in _read(files[j]):
                if a.shape[1] != image_size:
                    raise ValueError(f"{files[j]}: image side {a.shape[1]} is not image_size {image_size} (resize when extracting; "
                                     "this loader does not resample)")
                pending.append(th.from_numpy(a))
            while len(pending) >= batch_size:
                hr, pending = th.stack(pending[:batch_size]), pending[batch_size:]
                if random_flip and not deterministic:
                    flip = th.from_numpy(rng.random(hr.shape[0]) < 0.5)
                    hr[flip] = hr[flip].flip(-1)
                lr, sr = degrade(hr)
                yield lr, hr, sr, {}
