"""Masks of masked conditional sampling (GaussianDiffusion.masked_sample_loop): which cells of a stream are known.

A mask has one cell per (frame, position) of a stream, shared by the channels: video [F, H, W] or [B, F, H, W], audio [L] or [B, L],
bool or uint8, non-zero = known.  A stream of `known` without a mask is known as a whole.  normalize() turns what the caller hands in
into what mmd_cond_replace reads (include/mmd.h): contiguous fp32 values, contiguous uint8 cells and the batch stride of the cells.
repaint_schedule() / jump_table() are the evaluation order and the coefficients of the loop's resampling jumps (jump_length, n_resample)."""
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


JUMP_DRAW = 0x80000000                # the draw of the schedule's first forward jump; the k-th draws JUMP_DRAW + k


def repaint_schedule(T, jump_length=None, n_resample=1):
    """The evaluation order of masked sampling with resampling jumps (RePaint, Lugmayr et al., CVPR 2022) over T reverse steps: a list of
    ("step", i, draw) - reverse step i, whose input is the state at level i (marginal alphas_cumprod[i]) - and ("jump", m, draw) - the
    state at level m diffused forward to level m + jump_length.  The jump levels are the multiples m of jump_length with
    m + jump_length <= T - 1; each is jumped from n_resample - 1 times, the first time it is reached from above with jumps left.  So the
    jump_length steps above a jump level run n_resample times: T + (n_resample - 1) jump_length |levels| evaluations.

    The draws are the counter word of seeded.CounterNoise: execution r = 0, 1, ... of step i draws i + r T, so a first visit draws what the
    plain loop draws, and the k-th jump draws 0x80000000 + k.  jump_length=None or n_resample=1: the plain T - 1 ... 0."""
    T, U = int(T), int(n_resample)
    if T < 1:
        raise H.MMDError(f"repaint_schedule: T must be at least 1, got T={T}")
    if U < 1:
        raise H.MMDError(f"repaint_schedule: n_resample must be at least 1, got n_resample={U}")
    if U * T >= 1 << 31:
        raise H.MMDError(f"repaint_schedule: n_resample * T must stay below 2^31 (the draws of the steps), got n_resample={U} with T={T}")
    if jump_length is None:
        J, left = None, {}
    else:
        J = int(jump_length)
        if J < 1:
            raise H.MMDError(f"repaint_schedule: jump_length must be at least 1, got jump_length={J}")
        if U > 1 and J > T - 1:
            raise H.MMDError(f"repaint_schedule: jump_length={J} exceeds T - 1 = {T - 1}: no level to jump from")
        left = {m: U - 1 for m in range(0, T - J, J)}
    out, visits, level = [], [0] * T, T - 1
    jumps = 0
    while level >= 0:
        out.append(("step", level, level + visits[level] * T))
        visits[level] += 1
        level -= 1
        if left.get(level, 0) > 0:
            left[level] -= 1
            out.append(("jump", level, JUMP_DRAW + jumps))
            jumps += 1
            level += J
    return out


def jump_table(alphas_cumprod, jump_length):
    """float64 [2, T]: row 0 a[m] = sqrt(ac[m + J] / ac[m]), row 1 b[m] = sqrt(1 - ac[m + J] / ac[m]), the coefficients that take the state
    at level m to level m + J (x = a x + b z: q(x_{m+J} | x_m)); entries with m + J > T - 1 are zero (never used)."""
    import numpy as np
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    T, J = ac.shape[0], int(jump_length)
    if not 1 <= J <= max(T - 1, 1):
        raise H.MMDError(f"jump_table: jump_length must be in [1, {T - 1}], got jump_length={J}")
    tab = np.zeros((2, T), dtype=np.float64)
    ratio = ac[J:] / ac[:T - J]
    tab[0, :T - J] = np.sqrt(ratio)
    tab[1, :T - J] = np.sqrt(1.0 - ratio)
    return tab


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
