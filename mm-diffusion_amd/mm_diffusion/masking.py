"""Masks of masked conditional sampling (GaussianDiffusion.masked_sample_loop): which cells of a stream are known.

A mask has one cell per (frame, position) of a stream, shared by the channels: video [F, H, W] or [B, F, H, W], audio [L] or [B, L],
bool or uint8, non-zero = known.  A stream of `known` without a mask is known as a whole.  normalize() turns what the caller hands in
into what mmd_cond_replace reads (include/mmd.h): contiguous fp32 values, contiguous uint8 cells and the batch stride of the cells."""
from collections import namedtuple

import torch as th

from . import _hip as H

KEYS = ("video", "audio")

# known: fp32 contiguous [B, ...]; mask: uint8 contiguous or None (the whole stream); stride: 0 (one mask for the batch) or the cells of a sample
Cond = namedtuple("Cond", "known mask stride")


def cells(key, sample_shape):
    """The mask shape of one sample: video (F, C, H, W) -> (F, H, W), audio (C, L) -> (L,)."""
    s = tuple(int(v) for v in sample_shape)
    if len(s) != (4 if key == "video" else 2):
        raise H.MMDError(f"shape[{key!r}]: expected {'[B, F, C, H, W]' if key == 'video' else '[B, C, L]'}, got a sample of shape {s}")
    return (s[0], s[2], s[3]) if key == "video" else (s[1],)


def normalize(known, mask, shape):
    """{key: Cond} for the streams of `known` ({"video": [B,F,C,H,W], "audio": [B,C,L]}, either or both) under `mask` (None, or a dict
    over keys of `known`; a missing key = the whole stream) in a sampling run of `shape` ({"video": (B,F,C,H,W), "audio": (B,C,L)}).
    The tensors stay on their devices.  Every error is an MMDError that names the entry."""
    if not isinstance(known, dict) or not known:
        raise H.MMDError("known: expected a dict with 'video' and / or 'audio'")
    if mask is not None and not isinstance(mask, dict):
        raise H.MMDError("mask: expected None or a dict with the keys of known")
    for name, d in (("known", known), ("mask", mask or {})):
        for k in d:
            if k not in KEYS:
                raise H.MMDError(f"{name}[{k!r}]: unknown stream (video or audio)")
    for k in (mask or {}):
        if k not in known:
            raise H.MMDError(f"mask[{k!r}]: no known[{k!r}] to take the cells from")
    out = {}
    for k in KEYS:
        if k not in known:
            continue
        if k not in shape:
            raise H.MMDError(f"known[{k!r}]: the sampling shape has no {k!r}")
        want = tuple(int(v) for v in shape[k])
        v = known[k]
        if not th.is_tensor(v) or not v.is_floating_point():
            raise H.MMDError(f"known[{k!r}]: expected a floating-point tensor of shape {want}")
        if tuple(v.shape) != want:
            raise H.MMDError(f"known[{k!r}]: shape {tuple(v.shape)} differs from the sampling shape {want}")
        cell = cells(k, want[1:])
        per = 1
        for c in cell:
            per *= c
        m, stride = None, 0
        if mask is not None and k in mask and mask[k] is not None:
            m = mask[k]
            if not th.is_tensor(m) or m.dtype not in (th.bool, th.uint8):
                raise H.MMDError(f"mask[{k!r}]: expected a bool or uint8 tensor, got {getattr(m, 'dtype', type(m).__name__)}")
            if tuple(m.shape) == cell:
                stride = 0
            elif tuple(m.shape) == (want[0],) + cell:
                stride = per
            else:
                raise H.MMDError(f"mask[{k!r}]: shape {tuple(m.shape)} is neither {cell} nor {(want[0],) + cell}")
            m = m.to(th.uint8).contiguous()
        out[k] = Cond(v.detach().float().contiguous(), m, stride)
    return out


def to_device(cond, device):
    """normalize's result with its tensors on `device`: a missing mask stays None, shapes, dtypes and strides stay as they are.  The
    known values of a GPU run must be device tensors already (there is no silent upload of a clip)."""
    if th.device(device).type == "cuda":
        H.require_cuda(*(c.known for c in cond.values()))
    return {k: c._replace(known=c.known.to(device), mask=None if c.mask is None else c.mask.to(device)) for k, c in cond.items()}


def prefix_masks(video_size, audio_size, frames):
    """The masks that continue a clip: the first `frames` of the F video frames and the audio they span, floor(frames * L / F) samples.
    video_size (F, C, H, W), audio_size (C, L) -> {"video": bool [F, H, W], "audio": bool [L]}."""
    F, Hh, Ww = cells("video", video_size)
    L, = cells("audio", audio_size)
    frames = int(frames)
    if not 0 <= frames <= F:
        raise H.MMDError(f"prefix_masks: frames must be in [0, {F}], got {frames}")
    video = th.zeros(F, Hh, Ww, dtype=th.bool)
    video[:frames] = True
    audio = th.zeros(L, dtype=th.bool)
    audio[:frames * L // F] = True
    return {"video": video, "audio": audio}
