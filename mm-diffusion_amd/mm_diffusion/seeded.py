"""Seeded, addressable samples: a noise source that is a pure function of (seed, sample id, draw, stream, element).

    diffusion.noise_source = CounterNoise(42, first_sample=rank * B)

Sample k of seed s then comes out bitwise the same at any batch position, batch size, lane count and rank count, on the graph and the
eager path, whatever else the process drew before: x_T, the per-step noise (drawn inside the update kernels, mmd_ddpm_update_ctr /
mmd_ddim_update_ctr) and the window shifts all come from Philox4x32-10 on the counter layout of include/mmd.h (mmd_ctr_fill):
    c0 = element >> 2, c1 = draw (the loop index; X_T for the start noise), c2 = sample id, c3 = stream tag.
A loop that runs a step more than once names its draws itself (masked_sample_loop with resampling jumps, masking.repaint_schedule: visit r
of step i draws at i + r T, the k-th forward jump at 0x80000000 + k; drawing_at() is the route through p_sample).
The reference's scripts carry a `--seed` flag that seeds nothing (common.py:103-114), and seeding torch by hand gives a clip that depends
on its batch position, the rank and the window shifts handed out before; with `noise_source` unset (or any other callable) all of that
stays exactly as it is.  The training-side noise (q_sample in the losses, dropout) and the variational-bound stepper are not covered."""
import contextlib

import numpy as np
import torch as th

from . import _hip as H
from . import ops

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
X_T = 0xFFFFFFFF                      # the draw of the start noise
TAG_VIDEO, TAG_AUDIO, TAG_IMAGE, TAG_SHIFTS = 0, 1, 2, 3
_TAG_OF_DIM = {5: TAG_VIDEO, 3: TAG_AUDIO, 4: TAG_IMAGE}


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on Python ints: counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _tag_of(like):
    try:
        return _TAG_OF_DIM[like.dim()]
    except KeyError:
        raise H.MMDError(f"CounterNoise: no stream tag for a tensor of shape {tuple(like.shape)} (video [N,F,C,H,W], audio [N,C,L], "
                         "image [N,C,H,W])") from None


class CounterNoise:
    """callable(like) -> N(0,1) tensor, as every `noise_source`; the sampling loops recognise the class and draw in-kernel instead.

    seed: 64-bit; the samples of a batch of B are first_sample ... first_sample + B - 1, or `sample_ids` (any ids in [0, 2^32), one per
    batch row).  `draw` is the loop index the callable form reads; p_sample / ddim_sample set it from t, or from drawing_at(draw)."""

    def __init__(self, seed, first_sample=0, sample_ids=None):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise H.MMDError(f"CounterNoise: the seed must be in [0, 2^64), got {seed}")
        self.seed = seed
        self.key_words = (seed & MASK, seed >> 32)
        self.first_sample = int(first_sample)
        self.sample_ids = None if sample_ids is None else [int(i) for i in sample_ids]
        for i in (self.sample_ids if self.sample_ids is not None else [self.first_sample]):
            self._check_id(i)
        self.draw = None
        self.explicit = None
        self._dev = {}

    @staticmethod
    def _check_id(i):
        if not 0 <= i < 1 << 32:
            raise H.MMDError(f"CounterNoise: sample ids must be in [0, 2^32), got {i}")

    @classmethod
    def for_rank(cls, seed, batch, round=0):
        """The source of this rank's `batch` samples in sampling round `round` of a run that hands every rank `batch` samples per round:
        ids (round * world + rank) * batch ..."""
        from . import dist_util
        return cls(seed, first_sample=(int(round) * dist_util.world_size() + dist_util.rank()) * int(batch))

    # ------------------------------------------------------------------ device state
    def ids_list(self, batch):
        if self.sample_ids is not None:
            if len(self.sample_ids) != batch:
                raise H.MMDError(f"CounterNoise: {len(self.sample_ids)} sample ids for a batch of {batch}")
            return self.sample_ids
        self._check_id(self.first_sample + batch - 1)
        return list(range(self.first_sample, self.first_sample + batch))

    def key(self, device):
        """device uint32[2] (int32 storage): the seed, low word first."""
        k = ("key", str(device))
        if k not in self._dev:
            self._dev[k] = th.from_numpy(np.array(self.key_words, dtype=np.uint32).view(np.int32)).to(device)
        return self._dev[k]

    def ids(self, batch, device):
        """device int64 [batch]: the sample ids of the batch rows."""
        k = ("ids", int(batch), str(device))
        if k not in self._dev:
            self._dev[k] = th.tensor(self.ids_list(int(batch)), dtype=th.int64).to(device)
        return self._dev[k]

    # ------------------------------------------------------------------ draws
    def set_draw(self, t):
        """The draw of the callable form and of shifts(): an int, or the timestep tensor of a step, which must be uniform across the batch
        (one window-shift draw serves the whole batch)."""
        if self.explicit is not None:      # drawing_at(): the loop names the draw, the timestep does not
            self.draw = self.explicit
            return self.draw
        if th.is_tensor(t):
            lo, hi = int(t.min()), int(t.max())
            if lo != hi:
                raise H.MMDError("CounterNoise: the timesteps of a batch must be uniform (one draw index per step)")
            t = lo
        self.draw = int(t) & MASK
        return self.draw

    @contextlib.contextmanager
    def drawing_at(self, draw):
        """While active, every step draws at `draw` whatever its timestep: set_draw(t) keeps `draw`, and p_sample's update kernel reads
        it from draws() (mmd_ddpm_update_ctr_at).  A loop that runs a timestep more than once (masked_sample_loop with resampling jumps,
        masking.repaint_schedule) gives every visit a draw of its own this way."""
        prev, self.explicit = self.explicit, int(draw) & MASK
        try:
            yield self
        finally:
            self.explicit = prev

    def draws(self, batch, device):
        """device int64 [batch] filled with the draw of drawing_at(), or None outside it (the draw is then the timestep)."""
        if self.explicit is None:
            return None
        return th.full((int(batch),), self.explicit, dtype=th.int64, device=device)

    def randn(self, shape, tag, draw, device=None):
        """fp32 N(0,1) tensor of `shape` [N, ...] for stream `tag` at `draw`, rows = this source's samples (mmd_ctr_fill)."""
        return self._fill(shape, tag, draw, device, 0)

    def words(self, shape, tag, draw, device=None):
        """The raw 32-bit words behind randn(), as int32 storage (diagnosis)."""
        return self._fill(shape, tag, draw, device, 1)

    def _fill(self, shape, tag, draw, device, kind):
        if device is None:
            from . import dist_util
            device = dist_util.dev()
        if th.device(device).type != "cuda":
            raise H.MMDError("CounterNoise draws on the MI355X HIP path only (device must be a GPU); no CPU fallback")
        out = th.empty(tuple(shape), dtype=th.float32 if kind == 0 else th.int32, device=device)
        return ops.ctr_fill(out, kind, self.key(device), self.ids(out.shape[0], device), draw, tag)

    def __call__(self, like):
        H.require_cuda(like)
        if self.draw is None:
            raise H.MMDError("CounterNoise: no draw index is set (set_draw(t)); the sampling steps set it from t")
        return self.randn(like.shape, _tag_of(like), self.draw, like.device).to(like.dtype)

    def shifts(self, i, unet):
        """The window shifts of loop index i, one per shifted cross-attention block in draw_shifts order: word 0 of counter
        (j, i, 0, TAG_SHIFTS) mapped to lo + ((w (hi - lo + 1)) >> 32).  One sequence for all samples of a run."""
        F = unet.video_size[0]
        out = []
        for blk in unet._arch[0] + [unet._arch[1]] + unet._arch[2]:
            for layer in blk:
                if layer["kind"] == "cross" and layer["shift"]:
                    out.append(self.shift(len(out), i, 0, F - layer["window"]))
        return out

    def shift(self, j, i, lo, hi):
        w = philox4x32_10((j, int(i) & MASK, 0, TAG_SHIFTS), self.key_words)[0]
        return lo + ((w * (hi - lo + 1)) >> 32)

    @contextlib.contextmanager
    def shifting(self, model):
        """While active, the eager forward of the MultimodalUNet behind `model` draws its window shifts from shifts(self.draw, unet) (a
        model with a shift_source of its own keeps it)."""
        from .sampler import unwrap_unet
        unet = unwrap_unet(model)
        if unet is None or unet.shift_source is not None:
            yield
            return
        j = [0]

        def source(lo, hi):
            j[0] += 1
            return self.shift(j[0] - 1, self.draw, lo, hi)
        unet.shift_source = source
        try:
            yield
        finally:
            unet.shift_source = None


def counter_source(diffusion):
    """The diffusion's noise source if it is a CounterNoise, else None."""
    src = getattr(diffusion, "noise_source", None)
    return src if isinstance(src, CounterNoise) else None
