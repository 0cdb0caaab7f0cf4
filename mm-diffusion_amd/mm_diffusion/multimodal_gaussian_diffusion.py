"""Multimodal Gaussian diffusion (DDPM ancestral sampling / training loss) on the MI355X HIP path.

Same public surface as the reference's `GaussianDiffusion`
(/root/reference/mm_diffusion/multimodal_gaussian_diffusion.py:102-1203): enums, `get_named_beta_schedule`,
fp64 numpy tables (`betas`, `alphas_cumprod`, ... same attribute names), `q_sample`, `p_mean_variance`,
`p_sample`, `p_sample_loop(_progressive)`, `multimodal_training_losses`.

MI355X-first differences:
  * all per-step coefficient tables are uploaded ONCE as a [7, T] fp32 device table; the reference re-uploads
    ~16 fp64 tables per step (`_extract_into_tensor`, gd:1289-1303)
  * the whole epsilon -> x0 -> clamp -> posterior mean -> sample chain of p_mean_variance + p_sample is one
    fused elementwise kernel per stream (mmd_ddpm_update)
  * `p_sample_loop` captures [U-Net launch plan + both updates] into one hipGraph and replays it per step,
    refreshing only the timestep, the window shifts and the noise
  * DDIM (`ddim_sample(_loop)`) rides the same graph with mmd_ddim_update; zero-shot conditional sampling
    (`conditional_p_sample_loop`, gd:584-819) is built for both the replacement and the gradient-guided method
    (the latter differentiates the HIP training path w.r.t. the target stream's input); `masked_sample_loop` is the replacement
    method with partial masks (clip continuation, inpainting) on the DDPM or the DDIM stepper, the replacement itself one
    mmd_cond_replace launch per stream inside the step graph
  * the variational bound in bits / dim (`_vb_terms_bpd`, `_prior_bpd`, `calc_bpd_loop`, gd:1048-1092, 1213-1286) is one
    reduction kernel per stream and step (mmd_vlb_terms) that writes into device result tables; `calc_bpd_loop` replays
    [q_sample + U-Net plan + both reductions] as one hipGraph per step and reads the tables back once.  The reference's
    own multimodal `calc_bpd_loop` cannot run (it calls `.device` / `th.randn_like` on the stream dict, gd:1249-1257); here
    it is the per-stream loop over the reference's working pieces, every result keyed {"video", "audio"}
  * DDIM inversion (`ddim_encode_loop`, `ddim_decode_loop`, `ddim_interpolate`): the reverse ODE of `ddim_reverse_sample` (gd:903-953) as a
    graph-replayed loop from the clip up to a level, the DDIM loop from a level and a state the caller holds, and the spherical
    interpolation of two encoded clips (mmd_slerp) decoded at every weight; none of it is in the reference, whose reverse step raises
Not built: cond_fn (the reference's condition_mean / condition_score call `.float()` / `.shape` on the stream
dict, gd:385,403, and raise for every multimodal call); KL / RESCALED_KL in multimodal_training_losses (no terms in the
reference either, gd:1143).
"""
import enum
import math

import numpy as np
import torch as th

from . import _hip as H
from . import ops


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    """Named beta schedules (reference gd:17-41)."""
    if schedule_name == "linear":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps,
                                   lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    T = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), max_beta) for i in range(T)])


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self == LossType.KL or self == LossType.RESCALED_KL


def mean_flat(tensor):
    return tensor.mean(dim=list(range(1, len(tensor.shape))))


def _geom(x):
    """API tensor -> (F, C, HW) of the [N, F, C, HW] view the update kernels index (audio: F = 1)."""
    if x.dim() == 5:
        return x.shape[1], x.shape[2], x.shape[3] * x.shape[4]
    if x.dim() == 3:
        return 1, x.shape[1], x.shape[2]
    raise ValueError(f"expected video [N,F,C,H,W] or audio [N,C,L], got {tuple(x.shape)}")


class GaussianDiffusion:
    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type, rescale_timesteps=False):
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        self.rescale_timesteps = rescale_timesteps
        if model_mean_type == ModelMeanType.PREVIOUS_X:
            raise NotImplementedError("ModelMeanType.PREVIOUS_X is never produced by the factory (msu:225-242)")
        if model_var_type == ModelVarType.LEARNED:
            raise NotImplementedError("ModelVarType.LEARNED is never produced by the factory (msu:225-242)")

        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert len(betas.shape) == 1, "betas must be 1-D"
        assert (betas > 0).all() and (betas <= 1).all()
        self.num_timesteps = int(betas.shape[0])

        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        # noise source for sampling: callable(like_tensor) -> N(0,1) tensor; default th.randn_like (gd:453-454).  A seeded.CounterNoise makes
        # every sample a function of (seed, sample id): x_T, the per-step noise (drawn in the update kernels) and the window shifts
        self.noise_source = None
        self._dev_tables = {}

    # ------------------------------------------------------------------ device tables
    def _fixed_logvar(self):
        if self.model_var_type == ModelVarType.FIXED_SMALL:
            return self.posterior_log_variance_clipped
        return np.log(np.append(self.posterior_variance[1], self.betas[1:]))     # FIXED_LARGE (gd:288-291)

    def device_tables(self, device):
        """[7, T] fp32: sqrt_recip_ac, sqrt_recipm1_ac, post_c1, post_c2, fixed logvar, min_log, max_log; and [2, T]
        q_sample table.  fp64 -> fp32 exactly as the reference's `.float()` after indexing (gd:1300)."""
        key = str(device)
        if key not in self._dev_tables:
            tab = np.stack([self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod, self.posterior_mean_coef1,
                            self.posterior_mean_coef2, self._fixed_logvar(), self.posterior_log_variance_clipped,
                            np.log(self.betas)])
            q = np.stack([self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod])
            self._dev_tables[key] = (th.from_numpy(tab).float().to(device).contiguous(),
                                     th.from_numpy(q).float().to(device).contiguous())
        return self._dev_tables[key]

    def ddim_tables(self, device):
        """[3, T] fp32 alphas_cumprod, alphas_cumprod_prev, alphas_cumprod_next for mmd_ddim_update."""
        key = ("ddim", str(device))
        if key not in self._dev_tables:
            tab = np.stack([self.alphas_cumprod, self.alphas_cumprod_prev, self.alphas_cumprod_next])
            self._dev_tables[key] = th.from_numpy(tab).float().to(device).contiguous()
        return self._dev_tables[key]

    def jump_tables(self, jump_length, device):
        """[2, T] fp32 table of the forward jump over `jump_length` levels (masking.jump_table, computed in float64) for mmd_renoise_ctr
        and, as its memory form, mmd_q_sample."""
        from . import masking
        key = ("jump", int(jump_length), str(device))
        if key not in self._dev_tables:
            self._dev_tables[key] = th.from_numpy(masking.jump_table(self.alphas_cumprod, jump_length)).float().to(device).contiguous()
        return self._dev_tables[key]

    def _tab(self, arr, name, device):
        """fp32 device copy of one fp64 coefficient table (cached by name) for mmd_lincomb_t."""
        key = (name, str(device))
        if key not in self._dev_tables:
            self._dev_tables[key] = th.from_numpy(np.asarray(arr, dtype=np.float64)).float().to(device).contiguous()
        return self._dev_tables[key]

    def _lin(self, a, b, t, ca=None, cb=None, cs=None):
        """(ca[t] a + cb[t] b) cs[t] with per-sample table lookups, one kernel; ca/cb/cs = (name, fp64 table) or None."""
        H.require_cuda(a)
        dev = a.device
        tabs = [None if c is None else self._tab(c[1], c[0], dev) for c in (ca, cb, cs)]
        a32 = a.float().contiguous()
        b32 = None if b is None else b.float().contiguous()
        return ops.lincomb_t(a32, b32, th.empty_like(a32), tabs[0], tabs[1], tabs[2], t.to(th.int64).contiguous())

    def _extract(self, arr, name, t, shape):
        """`_extract_into_tensor` (gd:1289-1303): fp32 table values at t broadcast to `shape`."""
        v = self._tab(arr, name, t.device)[t.long()]
        return v.view(-1, *([1] * (len(shape) - 1))).expand(shape)

    def q_mean_variance(self, x_start, t):
        """gd:170-185."""
        mean = self._lin(x_start, None, t, ca=("sqrt_ac", self.sqrt_alphas_cumprod))
        variance = self._extract(1.0 - self.alphas_cumprod, "one_minus_ac", t, x_start.shape)
        log_variance = self._extract(self.log_one_minus_alphas_cumprod, "log_one_minus_ac", t, x_start.shape)
        return mean, variance, log_variance

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """gd:207-229: mean = coef1 x_0 + coef2 x_t, posterior variance and its clipped log."""
        assert x_start.shape == x_t.shape
        mean = self._lin(x_start, x_t, t, ca=("post_c1", self.posterior_mean_coef1), cb=("post_c2", self.posterior_mean_coef2))
        variance = self._extract(self.posterior_variance, "post_var", t, x_t.shape)
        logvar = self._extract(self.posterior_log_variance_clipped, "post_logvar", t, x_t.shape)
        return mean, variance, logvar

    def _predict_xstart_from_eps(self, x_t, t, eps):
        """gd:345-350."""
        assert x_t.shape == eps.shape
        return self._lin(x_t, eps, t, ca=("sqrt_recip_ac", self.sqrt_recip_alphas_cumprod),
                         cb=("neg_sqrt_recipm1_ac", -self.sqrt_recipm1_alphas_cumprod))

    def _predict_xstart_from_xprev(self, x_t, t, xprev):
        """gd:352-360: (xprev - coef2 x_t) / coef1."""
        assert x_t.shape == xprev.shape
        return self._lin(xprev, x_t, t, ca=("inv_post_c1", 1.0 / self.posterior_mean_coef1),
                         cb=("neg_c2_over_c1", -self.posterior_mean_coef2 / self.posterior_mean_coef1))

    def _predict_eps_from_xstart(self, x_t, t, pred_xstart):
        """gd:362-366: (sqrt_recip_ac x_t - x_0) / sqrt_recipm1_ac."""
        neg1 = ("neg_one", -np.ones_like(self.betas))
        return self._lin(x_t, pred_xstart, t, ca=("sqrt_recip_ac", self.sqrt_recip_alphas_cumprod), cb=neg1,
                         cs=("inv_sqrt_recipm1_ac", 1.0 / self.sqrt_recipm1_alphas_cumprod))

    def _flags(self, clip_denoised):
        return ((1 if clip_denoised else 0) | (2 if self.model_mean_type == ModelMeanType.START_X else 0) |
                (4 if self.model_var_type == ModelVarType.LEARNED_RANGE else 0))

    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    def _randn_like(self, x):
        return self.noise_source(x) if self.noise_source is not None else th.randn_like(x)

    def _counter(self):
        """The noise source if it is a seeded.CounterNoise (x_T, per-step noise and window shifts then come from its counter), else None."""
        from .seeded import counter_source
        return counter_source(self)

    def _start_noise(self, shape, tag, device):
        """x_T of one stream: the counter's X_T draw, else drawn on the CPU and moved like the reference."""
        ctr = self._counter()
        if ctr is not None:
            from .seeded import X_T
            return ctr.randn(shape, tag, X_T, device)
        return th.randn(*shape, device="cpu").to(device)

    def _x_T(self, shape, device):
        """The x_T dict of a sampling run (video first, then audio)."""
        return {"video": self._start_noise(shape["video"], 0, device), "audio": self._start_noise(shape["audio"], 1, device)}

    # ------------------------------------------------------------------ q(x_t | x_0)
    def q_sample(self, x_start, t, noise=None):
        """x_t = sqrt(ac_t) x_0 + sqrt(1-ac_t) eps (gd:187-205) as one kernel."""
        if noise is None:
            noise = self._randn_like(x_start)
        assert noise.shape == x_start.shape
        H.require_cuda(x_start)
        _, qtab = self.device_tables(x_start.device)
        out = th.empty_like(x_start, dtype=th.float32)
        ops.q_sample(x_start.float().contiguous(), noise.float().contiguous(), out, qtab, t.to(th.int64).contiguous())
        return out

    # ------------------------------------------------------------------ p(x_{t-1} | x_t)
    def _update(self, key, model_out, x, t, clip_denoised, noise=None, want=("sample",), denoised_fn=None, start_x=False):
        """Run the fused update kernel for one stream; returns a dict with the requested outputs.  denoised_fn (gd:263-268): the x_0
        prediction goes through it BEFORE the clamp - one pass of the kernel for the unclamped prediction, the caller's function on that
        tensor, then the kernel again with the processed tensor in the place of the model's mean channels, read as an x_0 prediction."""
        if denoised_fn is not None:
            raw = self._update(key, model_out, x, t, False, want=("pred_xstart",), start_x=start_x)["pred_xstart"]
            x0 = denoised_fn(raw)
            cd = 2 if x.dim() == 5 else 1
            mo2 = model_out.float().clone()
            mo2.narrow(cd, 0, x.shape[cd]).copy_(x0)
            return self._update(key, mo2, x, t, clip_denoised, noise=noise, want=want, start_x=True)
        tab, _ = self.device_tables(x.device)
        F, C, HW = _geom(x)
        xs = x.float().contiguous()
        mo = model_out.float().contiguous()
        res = {k: th.empty_like(xs) for k in want}
        flags = self._flags(clip_denoised) | (2 if start_x else 0)
        outs = dict(x0_out=res.get("pred_xstart"), mean_out=res.get("mean"), logvar_out=res.get("log_variance"))
        from .seeded import CounterNoise
        if isinstance(noise, CounterNoise):      # drawn in the kernel: counter (element, t, sample id, stream)
            src = (xs, mo, noise.key(xs.device), noise.ids(xs.shape[0], xs.device), 0 if key == "video" else 1, res.get("sample"), tab,
                   t.to(th.int64).contiguous())
            draws = noise.draws(xs.shape[0], xs.device)
            if draws is None:
                ops.ddpm_update_ctr(*src, F, C, HW, flags, **outs)
            else:                                # CounterNoise.drawing_at: the loop names the draw (resampling jumps)
                ops.ddpm_update_ctr_at(*src, draws, F, C, HW, flags, **outs)
        else:
            ops.ddpm_update(xs, mo, noise, res.get("sample"), tab, t.to(th.int64).contiguous(), F, C, HW, flags, **outs)
        return res

    def _model_out2(self, model, x, t, model_kwargs, ctr=None):
        """(video_output, audio_output) of the model at x_t; SpacedDiffusion maps the timesteps in here.  With a counter `ctr` this is
        the draw of step t, and the eager forward takes its window shifts from the counter too."""
        if ctr is None:
            return model(x["video"], x["audio"], self._scale_timesteps(t), **(model_kwargs or {}))
        ctr.set_draw(t)
        with ctr.shifting(model):
            return model(x["video"], x["audio"], self._scale_timesteps(t), **(model_kwargs or {}))

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """gd:231-343.  Returns the same nested dict ({'mean','variance','log_variance','pred_xstart','model_predict'}
        each {'video','audio'})."""
        model_kwargs = model_kwargs or {}
        B = x["video"].shape[0]
        assert t.shape == (B,)
        video_output, audio_output = model(x["video"], x["audio"], self._scale_timesteps(t), **model_kwargs)
        out = {k: {} for k in ("mean", "variance", "log_variance", "pred_xstart", "model_predict")}
        for key, mo in (("video", video_output), ("audio", audio_output)):
            r = self._update(key, mo, x[key], t, clip_denoised, want=("mean", "log_variance", "pred_xstart"), denoised_fn=denoised_fn)
            out["mean"][key], out["log_variance"][key], out["pred_xstart"][key] = r["mean"], r["log_variance"], r["pred_xstart"]
            out["variance"][key] = th.exp(r["log_variance"])
            out["model_predict"][key] = mo
        return out

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, noise=None):
        """One ancestral step (gd:415-474).  Like the reference, the `noise` argument is ignored and fresh N(0,1)
        noise is drawn for both streams (video first), also at t == 0."""
        if cond_fn is not None:
            raise NotImplementedError("cond_fn: the reference's condition_mean raises for the multimodal dict (gd:385 calls dict.float()); not built")
        ctr = self._counter()
        video_output, audio_output = self._model_out2(model, x, t, model_kwargs, ctr)
        differentiable = th.is_grad_enabled() and any(v.requires_grad for v in (video_output, audio_output, x["video"], x["audio"]))
        if ctr is not None and not differentiable:
            noise = {"video": ctr, "audio": ctr}
        else:                                # (the differentiable guided step takes the counter's values through the callable form)
            noise = {"video": self._randn_like(x["video"]), "audio": self._randn_like(x["audio"])}
        res = {"sample": {}, "pred_start": {}, "pred_noise": {"video": video_output, "audio": audio_output}}
        for key, mo in (("video", video_output), ("audio", audio_output)):
            if differentiable:          # gradient-guided conditional sampling differentiates the step (gd:795-817)
                from .train_ops import DdpmUpdateFn
                tab, _ = self.device_tables(x[key].device)
                s_, x0_ = DdpmUpdateFn.apply(x[key].float(), mo.float(), noise[key].float().contiguous(), tab,
                                             t.to(th.int64).contiguous(), self._flags(clip_denoised), _geom(x[key]))
                res["sample"][key], res["pred_start"][key] = s_, x0_
                continue
            r = self._update(key, mo, x[key], t, clip_denoised, noise=noise[key] if noise[key] is ctr else noise[key].float().contiguous(),
                             want=("sample", "pred_xstart"), denoised_fn=denoised_fn)
            res["sample"][key], res["pred_start"][key] = r["sample"], r["pred_xstart"]
        return res

    # ------------------------------------------------------------------ DDIM
    def _ddim(self, model, x, t, clip_denoised, model_kwargs, eta, reverse):
        ctr = None if reverse else self._counter()
        video_output, audio_output = self._model_out2(model, x, t, model_kwargs, ctr)
        res = {"sample": {}, "pred_xstart": {}}
        flags = self._flags(clip_denoised) | (8 if reverse else 0)
        for key, mo in (("video", video_output), ("audio", audio_output)):
            tab, _ = self.device_tables(x[key].device)
            F, C, HW = _geom(x[key])
            xs = x[key].float().contiguous()
            out, x0 = th.empty_like(xs), th.empty_like(xs)
            if ctr is not None:
                ops.ddim_update_ctr(xs, mo.float().contiguous(), ctr.key(xs.device), ctr.ids(xs.shape[0], xs.device), 0 if key == "video" else 1,
                                    out, tab, self.ddim_tables(xs.device), t.to(th.int64).contiguous(), F, C, HW, flags, eta, x0_out=x0)
                res["sample"][key], res["pred_xstart"][key] = out, x0
                continue
            noise = None if reverse else self._randn_like(xs).float().contiguous()      # drawn even when eta == 0 (gd:876-877)
            ops.ddim_update(xs, mo.float().contiguous(), noise, out, tab, self.ddim_tables(xs.device), t.to(th.int64).contiguous(),
                            F, C, HW, flags, eta, x0_out=x0)
            res["sample"][key], res["pred_xstart"][key] = out, x0
        return res

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        """One DDIM step (gd:821-901): eps re-derived from the (clipped) x_0 prediction; noise drawn video first."""
        if cond_fn is not None or denoised_fn is not None:
            raise NotImplementedError("cond_fn / denoised_fn: the reference's condition_score raises for the multimodal dict (gd:403)")
        return self._ddim(model, x, t, clip_denoised, model_kwargs, eta, False)

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0):
        """DDIM reverse ODE step x_t -> x_{t+1} (gd:903-953).  The reference indexes its own result dict the wrong way
        round (`out["video"]["pred_xstart"]`, gd:925) and raises KeyError; this computes the intended update."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        if denoised_fn is not None:
            raise NotImplementedError("denoised_fn is not supported by the fused update kernel")
        return self._ddim(model, x, t, clip_denoised, model_kwargs, 0.0, True)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                         device=None, progress=True, eta=0.0):
        final = None
        for sample in self.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                        cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, progress=progress,
                                                        eta=eta):
            final = sample
        return final

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, use_graph=True):
        """gd:989-1046 (the `noise` argument is ignored there too: x_T is always drawn on the CPU, video then audio)."""
        if cond_fn is not None or denoised_fn is not None:
            raise NotImplementedError("cond_fn / denoised_fn: see ddim_sample")
        device = self._sampling_device(device)
        x = self._x_T(shape, device)
        indices = self._indices(progress)
        stepper = self._graph_stepper(model, model_kwargs, use_graph, shape["video"][0], device, clip_denoised, update="ddim", eta=eta)
        if stepper is not None:
            stepper.load(x["video"], x["audio"])
            yield from self._replay(stepper, indices)
            return
        for i in indices:
            t = th.tensor([i] * shape["video"][0], device=device)
            with th.no_grad():
                out = self.ddim_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs, eta=eta)
            yield out["sample"]
            x = out["sample"]

    # ------------------------------------------------------------------ DDIM inversion: encode, decode from a level, interpolate
    # "Level l" (0 <= l <= T-1) is the state whose signal level is alphas_cumprod[l].  A clip is read as the level-0 state (the reference's
    # convention: ddim_reverse_sample at t = 0 reads alphas_cumprod[0]); ddim_sample_loop's x_T is the level T-1 state.  Encode step i maps
    # level i to level i + 1 (mmd_ddim_update with flag 8 at t = i), decode step i maps level i to level i - 1 (the "ddim" update at t = i;
    # step 0 ends at the sample).  Both evaluate the model at the level-i state, and with a seeded.CounterNoise both take the window shifts
    # of draw i, so an encode followed by a decode sees the same windows level by level.
    def _level(self, who, name, value, top_message=None):
        """The checked level argument `name` of `who`: an int in [1, T-1] for an encode target, [0, T-1] for a decode start."""
        T = self.num_timesteps
        lo = 1 if top_message is not None else 0
        if value is None:
            value = T - 1
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
            raise H.MMDError(f"{who}: {name} must be an integer level, got {value!r}")
        value = int(value)
        if top_message is not None and value == T:
            raise H.MMDError(f"{who}: {name} = {value} = T: {top_message}")
        if not lo <= value <= T - 1:
            raise H.MMDError(f"{who}: {name} = {value} is outside [{lo}, {T - 1}] (T = {T} levels, level l has signal alphas_cumprod[l])")
        return value

    _NO_TOP = ("alphas_cumprod_next[T-1] is 0, so that encode step would return the model's eps prediction, and no decode loop starts "
               "there (the top level is T-1)")

    def ddim_encode_indices(self, to_level=None, who="ddim_encode_loop", name="to_level"):
        """The steps an encode to level `to_level` (in [1, T-1], default T-1) runs, in order: i = 0 ... to_level - 1; step i reads
        alphas_cumprod[i] and alphas_cumprod_next[i] = alphas_cumprod[i + 1], never the 0 that pads the table's end."""
        return list(range(self._level(who, name, to_level, top_message=self._NO_TOP)))

    def ddim_decode_indices(self, from_level=None, who="ddim_decode_loop", name="from_level"):
        """The steps a decode from level `from_level` (in [0, T-1], default T-1) runs, in order: i = from_level ... 0."""
        return list(range(self._level(who, name, from_level), -1, -1))

    def _invert_state(self, who, name, model, x, device, shapes_only=False):
        """The checked {"video", "audio"} state `name` of an inversion loop as fp32 device tensors, and its device.  Nothing is moved
        for the caller: a CPU tensor is refused, as everywhere on this path.  shapes_only: check the layout against the model, no more."""
        from .sampler import unwrap_unet
        if not isinstance(x, dict) or set(x) != {"video", "audio"} or not all(th.is_tensor(v) for v in x.values()):
            raise H.MMDError(f"{who}: {name} must be a dict of tensors {{'video': [B,F,C,H,W], 'audio': [B,C,L]}}")
        v, a = x["video"], x["audio"]
        if v.dim() != 5 or a.dim() != 3 or v.shape[0] != a.shape[0] or v.shape[0] < 1:
            raise H.MMDError(f"{who}: {name} must be video [B,F,C,H,W] and audio [B,C,L] of one batch, got {tuple(v.shape)} and {tuple(a.shape)}")
        unet = unwrap_unet(model)
        if unet is not None and (list(v.shape[1:]) != list(unet.video_size) or list(a.shape[1:]) != list(unet.audio_size)):
            raise H.MMDError(f"{who}: {name} has shapes {tuple(v.shape[1:])} / {tuple(a.shape[1:])} per sample, the model takes "
                             f"{tuple(unet.video_size)} / {tuple(unet.audio_size)}")
        if shapes_only:
            return None
        for k in ("video", "audio"):
            if not x[k].is_cuda:
                raise H.MMDError(f"{who}: {name}[{k!r}] is a CPU tensor: the loop runs on the MI355X HIP path only, there is no CPU fallback")
        dev = v.device
        if a.device != dev or (device is not None and th.device(device).index not in (None, dev.index)):
            raise H.MMDError(f"{who}: {name} and device must name one GPU")
        self._sampling_device(device if device is not None else dev)
        return {"video": v.float().contiguous(), "audio": a.float().contiguous()}, dev

    @staticmethod
    def _refuse_hooks(who, denoised_fn, cond_fn):
        if denoised_fn is not None:
            raise H.MMDError(f"{who}: denoised_fn is not supported (the fused update forms the x_0 prediction inside the kernel)")
        if cond_fn is not None:
            raise H.MMDError(f"{who}: cond_fn is not supported (see ddim_sample)")

    def _encode_step(self, model, x, i, clip_denoised, model_kwargs):
        """The eager encode step i: ddim_reverse_sample at t = i; with a counter source the forward takes the window shifts of draw i."""
        import contextlib
        ctr = self._counter()
        t = th.tensor([i] * x["video"].shape[0], device=x["video"].device)
        if ctr is not None:
            ctr.set_draw(i)
        with th.no_grad(), (ctr.shifting(model) if ctr is not None else contextlib.nullcontext()):
            return self.ddim_reverse_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs)["sample"]

    def ddim_encode_loop(self, model, x_start, to_level=None, *, clip_denoised=False, model_kwargs=None, device=None, progress=False,
                         use_graph=True, lanes=None, eta=0.0, denoised_fn=None, cond_fn=None):
        """The last state of ddim_encode_loop_progressive: the level-`to_level` latent of the clip x_start."""
        final = None
        for sample in self.ddim_encode_loop_progressive(model, x_start, to_level, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                                        device=device, progress=progress, use_graph=use_graph, lanes=lanes, eta=eta,
                                                        denoised_fn=denoised_fn, cond_fn=cond_fn):
            final = sample
        return final

    def ddim_encode_loop_progressive(self, model, x_start, to_level=None, *, clip_denoised=False, model_kwargs=None, device=None,
                                     progress=False, use_graph=True, lanes=None, eta=0.0, denoised_fn=None, cond_fn=None):
        """DDIM inversion: x_start = {"video", "audio"} is read as the level-0 state and steps i = 0 ... to_level - 1 of the reverse ODE
        (gd:903-953) carry it to level `to_level` (in [1, T-1], default T-1: where ddim_sample_loop starts); the state after every step
        is yielded.  One graph replay per lane and step (sampler.GraphStepper, update="ddim_reverse") under the rule of the other loops,
        else ddim_reverse_sample step by step: the same bits.  The arguments are checked here, before the first step is asked for."""
        who = "ddim_encode_loop"
        self._refuse_hooks(who, denoised_fn, cond_fn)
        if eta != 0.0:
            raise H.MMDError(f"{who}: eta = {eta}: the reverse ODE is deterministic, only eta = 0 can be inverted")
        indices = self.ddim_encode_indices(to_level)
        x, device = self._invert_state(who, "x_start", model, x_start, device)
        stepper = self._graph_stepper(model, model_kwargs, use_graph, x["video"].shape[0], device, clip_denoised, update="ddim_reverse",
                                      lanes=lanes)
        return self._encode_steps(model, x, self._progress(indices, progress), stepper, clip_denoised, model_kwargs)

    def _encode_steps(self, model, x, indices, stepper, clip_denoised, model_kwargs):
        if stepper is not None:
            stepper.load(x["video"], x["audio"])
            yield from self._replay(stepper, indices)
            return
        for i in indices:
            x = self._encode_step(model, x, i, clip_denoised, model_kwargs)
            yield x

    def ddim_decode_loop(self, model, latent, from_level=None, *, eta=0.0, clip_denoised=True, model_kwargs=None, device=None, progress=False,
                         use_graph=True, lanes=None, denoised_fn=None, cond_fn=None):
        """The last state of ddim_decode_loop_progressive: the sample the level-`from_level` state `latent` decodes to."""
        final = None
        for sample in self.ddim_decode_loop_progressive(model, latent, from_level, eta=eta, clip_denoised=clip_denoised,
                                                        model_kwargs=model_kwargs, device=device, progress=progress, use_graph=use_graph,
                                                        lanes=lanes, denoised_fn=denoised_fn, cond_fn=cond_fn):
            final = sample
        return final

    def ddim_decode_loop_progressive(self, model, latent, from_level=None, *, eta=0.0, clip_denoised=True, model_kwargs=None, device=None,
                                     progress=False, use_graph=True, lanes=None, denoised_fn=None, cond_fn=None):
        """ddim_sample_loop_progressive on a state the caller holds: latent = {"video", "audio"} at level `from_level` (in [0, T-1],
        default T-1) runs steps i = from_level ... 0 of the "ddim" stepper (or ddim_sample eagerly) and every state is yielded.  With
        eta > 0 the noise of step i is drawn at draw i with a counter source, as in ddim_sample_loop.  From T-1 on that loop's x_T this is
        that loop, bit for bit.  The arguments are checked here, before the first step is asked for."""
        who = "ddim_decode_loop"
        self._refuse_hooks(who, denoised_fn, cond_fn)
        indices = self.ddim_decode_indices(from_level)
        x, device = self._invert_state(who, "latent", model, latent, device)
        stepper = self._graph_stepper(model, model_kwargs, use_graph, x["video"].shape[0], device, clip_denoised, update="ddim", eta=eta,
                                      lanes=lanes)
        return self._decode_steps(model, x, self._progress(indices, progress), stepper, clip_denoised, model_kwargs, eta)

    def _decode_steps(self, model, x, indices, stepper, clip_denoised, model_kwargs, eta):
        if stepper is not None:
            stepper.load(x["video"], x["audio"])
            yield from self._replay(stepper, indices)
            return
        for i in indices:
            t = th.tensor([i] * x["video"].shape[0], device=x["video"].device)
            with th.no_grad():
                x = self.ddim_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs, eta=eta)["sample"]
            yield x

    def ddim_interpolate(self, model, a, b, weights, level=None, *, clip_denoised=False, model_kwargs=None, device=None, progress=False,
                         use_graph=True, lanes=None, batch=None, denoised_fn=None, cond_fn=None):
        """Latent interpolation of two batches of clips: encode a and b to `level` (default T-1), form slerp(enc a, enc b, w) per stream
        and pair for every w in `weights` (mmd_slerp: rows that are parallel, opposite or zero take the chord), and decode each from
        `level` at eta = 0.  Returns {"video": [B, len(weights), F, C, H, W], "audio": [B, len(weights), C, L]}: entry [n, j] is pair n at
        weights[j]; w = 0 is decode(encode(a[n])), w = 1 decode(encode(b[n])).  clip_denoised applies to the encode and the decode alike.
        One encode stepper serves both encodes and one decode stepper every decode; `batch` (default B, a divisor of B) is their batch
        size, and larger inputs run through them in chunks.  Bitwise the composition ddim_encode_loop, ops.slerp, ddim_decode_loop."""
        who = "ddim_interpolate"
        self._refuse_hooks(who, denoised_fn, cond_fn)
        up = self.ddim_encode_indices(level, who, "level")
        level = len(up)
        down = self.ddim_decode_indices(level, who, "level")
        for name, x in (("a", a), ("b", b)):
            self._invert_state(who, name, model, x, device, shapes_only=True)
        try:
            lams = [float(w) for w in weights]
        except TypeError:
            raise H.MMDError(f"{who}: weights must be a sequence of numbers") from None
        if not lams or not all(math.isfinite(w) for w in lams):
            raise H.MMDError(f"{who}: weights must be a non-empty sequence of finite numbers, got {weights!r}")
        xa, device = self._invert_state(who, "a", model, a, device)
        xb, _ = self._invert_state(who, "b", model, b, device)
        B = xa["video"].shape[0]
        if xb["video"].shape[0] != B:
            raise H.MMDError(f"{who}: a and b must hold the same number of clips, got {B} and {xb['video'].shape[0]}")
        nb = B if batch is None else int(batch)
        if nb < 1 or B % nb:
            raise H.MMDError(f"{who}: batch = {batch} must be a positive divisor of the {B} pairs")
        enc = self._graph_stepper(model, model_kwargs, use_graph, nb, device, clip_denoised, update="ddim_reverse", lanes=lanes)
        dec = self._graph_stepper(model, model_kwargs, use_graph, nb, device, clip_denoised, update="ddim", lanes=lanes)
        kw = dict(clip_denoised=clip_denoised, model_kwargs=model_kwargs, use_graph=False)

        def run(stepper, x, indices):
            stepper.load(x["video"], x["audio"])
            for i in indices:
                stepper.step(i)
            return stepper.current()

        def encode(x):
            return run(enc, x, up) if enc is not None else self.ddim_encode_loop(model, x, level, **kw)

        def decode(x):
            return run(dec, x, down) if dec is not None else self.ddim_decode_loop(model, x, level, **kw)
        out = {k: th.empty((B, len(lams)) + tuple(xa[k].shape[1:]), dtype=th.float32, device=device) for k in ("video", "audio")}
        lam_dev = [th.full((nb,), w, dtype=th.float32, device=device) for w in lams]
        chunks = self._progress([slice(c, c + nb) for c in range(0, B, nb)], progress)
        try:
            for sl in chunks:
                ea = encode({k: v[sl] for k, v in xa.items()})
                eb = encode({k: v[sl] for k, v in xb.items()})
                for j, lam in enumerate(lam_dev):
                    res = decode({k: ops.slerp(ea[k], eb[k], lam) for k in ("video", "audio")})
                    for k in ("video", "audio"):
                        out[k][sl, j] = res[k]
        finally:
            for st in (enc, dec):
                if st is not None:
                    st.close()
        return out

    # ------------------------------------------------------------------ zero-shot conditional sampling (gd:584-819)
    def _sampling_device(self, device):
        if device is None:
            from . import dist_util
            device = dist_util.dev()
        if th.device(device).type != "cuda":
            raise H.MMDError("sampling runs on the MI355X HIP path only (device must be a GPU); no CPU fallback")
        return device

    def _indices(self, progress):
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        return indices

    def _graph_stepper(self, model, model_kwargs, use_graph, batch, device, clip_denoised, denoised_fn=None, update="ddpm", eta=0.0,
                       lanes=None, cond=None, jump_length=None):
        """The sampler.GraphStepper of a call whose steps can be graph-replayed - a MultimodalUNet behind `model`, no model_kwargs, no host
        callable on the x_0 prediction - else None: the caller then launches its steps eagerly."""
        from .sampler import GraphStepper, unwrap_unet
        unet = unwrap_unet(model)
        if not use_graph or unet is None or model_kwargs or denoised_fn is not None:
            return None
        return GraphStepper(self, unet, batch, device, clip_denoised, update=update, eta=eta, lanes=lanes, cond=cond, jump_length=jump_length)

    @staticmethod
    def _replay(stepper, indices, before=None, after=None, state=True):
        """Step a loaded stepper over `indices` and yield the state after every step (None without `state`); before(i) / after(i) run
        around step i.  The stepper is closed when the generator ends, is closed or is dropped."""
        try:
            for i in indices:
                if before is not None:
                    before(i)
                stepper.step(i)
                if after is not None:
                    after(i)
                yield stepper.current() if state else None
        finally:
            stepper.close()

    def conditional_p_sample_loop(self, model, shape, use_fp16, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=True, class_scale=0.):
        """class_scale == 0: replacement method; otherwise the gradient-guided method (gd:584-640)."""
        fn = self.conditional_p_sample_loop_progressive_unscale if class_scale == 0 else self.conditional_p_sample_loop_progressive_scale
        final = None
        for sample in fn(model, shape, use_fp16, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
                         model_kwargs=model_kwargs, device=device, progress=progress, class_scale=class_scale):
            final = sample
        return final

    def _cond_setup(self, shape, noise, model_kwargs, device):
        device = self._sampling_device(device)
        if noise is None:
            noise = self._x_T(shape, device)
        model_kwargs = model_kwargs if model_kwargs is not None else {}
        cond = {k: model_kwargs.pop(k) for k in ("video", "audio") if k in model_kwargs}     # popped like gd:687-691
        return device, noise, model_kwargs, cond

    def conditional_p_sample_loop_progressive_unscale(self, model, shape, use_fp16, noise=None, clip_denoised=True, denoised_fn=None,
                                                      cond_fn=None, model_kwargs=None, device=None, progress=False, class_scale=0.0,
                                                      use_graph=True):
        """Replacement method (gd:642-720): before every step the conditioning stream is overwritten with
        q_sample(condition, t, noise=<the fixed initial noise of that stream>); then one ordinary p_sample."""
        if cond_fn is not None or denoised_fn is not None:
            raise NotImplementedError("cond_fn / denoised_fn: see p_sample")
        device, noise, model_kwargs, cond = self._cond_setup(shape, noise, model_kwargs, device)
        x = dict(noise)
        B = shape["video"][0]
        stepper = self._graph_stepper(model, model_kwargs, use_graph, B, device, clip_denoised)
        if stepper is not None:
            def replace(i):
                t = th.tensor([i] * B, device=device)
                for k in cond:
                    stepper.set_x(k, self.q_sample(cond[k], t, noise=noise[k]))
            stepper.load(x["video"], x["audio"])
            yield from self._replay(stepper, self._indices(progress), before=replace)
            return
        for i in self._indices(progress):
            t = th.tensor([i] * B, device=device)
            for k in cond:
                x[k] = self.q_sample(cond[k], t, noise=noise[k])
            with th.no_grad():
                x = self.p_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs)["sample"]
            yield x

    def conditional_p_sample_loop_progressive_scale(self, model, shape, use_fp16, noise=None, clip_denoised=True, denoised_fn=None,
                                                    cond_fn=None, model_kwargs=None, device=None, progress=False, class_scale=3.0):
        """Gradient-guided method (gd:722-817).  Per step: replace the conditioning stream at t, take one differentiable
        p_sample, loss = mean_flat((sample[cond] - q_sample(cond, t-1))^2).mean() (x 2^20 when use_fp16, never unscaled -
        as in the reference), and move the target stream against d loss / d x_t[target] scaled by
        class_scale * sqrt_alphas_cumprod[i].  The U-Net backward w.r.t. its input runs on the HIP training kernels."""
        if cond_fn is not None or denoised_fn is not None:
            raise NotImplementedError("cond_fn / denoised_fn: see p_sample")
        device, noise, model_kwargs, cond = self._cond_setup(shape, noise, model_kwargs, device)
        if not cond:
            raise UnboundLocalError("conditional sampling needs model_kwargs['video'] or model_kwargs['audio'] (gd:776-786)")
        x = dict(noise)
        B = shape["video"][0]
        from .sampler import unwrap_unet
        unet = unwrap_unet(model)
        frozen = [p for p in unet.parameters() if p.requires_grad] if unet is not None else []
        for p in frozen:                 # only d/dx is needed: skip every weight-gradient kernel
            p.requires_grad_(False)
        try:
            yield from self._guided_steps(model, x, noise, cond, B, device, use_fp16, clip_denoised, model_kwargs, progress, class_scale)
        finally:
            for p in frozen:
                p.requires_grad_(True)

    def _guided_steps(self, model, x, noise, cond, B, device, use_fp16, clip_denoised, model_kwargs, progress, class_scale):
        for i in self._indices(progress):
            t = th.tensor([i] * B, device=device)
            for k, other in (("video", "audio"), ("audio", "video")):
                if k in cond:
                    condition, target = k, other
                    x[condition] = self.q_sample(cond[k], t, noise=noise[condition])
                    # at i == 0 the reference indexes its tables with t - 1 == -1, i.e. the LAST entry (gd:779,785)
                    previous_step_condition = self.q_sample(cond[k], (t - 1) % self.num_timesteps, noise=noise[condition])
            with th.enable_grad():
                none_zero_mask = (t != 0).float().view(-1, *([1] * (len(x[target].shape) - 1)))
                x[target] = x[target].detach().requires_grad_()
                out = self.p_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs)
                pred = out["sample"]
                loss = mean_flat((pred[condition] - previous_step_condition) ** 2)
                loss_scale = 2 ** 20 if use_fp16 == True else 1.       # noqa: E712 (reference compares with ==)
                grad = th.autograd.grad(loss.mean() * loss_scale, x[target])[0]
                x = {condition: x[condition], target: (pred[target] - none_zero_mask * grad * class_scale *
                                                       float(self.sqrt_alphas_cumprod[i])).detach()}
            yield x

    # ------------------------------------------------------------------ masked conditional sampling
    def masked_sample_loop(self, model, shape, known, mask=None, *, sampler="ddpm", eta=0.0, noise=None, clip_denoised=True,
                           model_kwargs=None, device=None, progress=False, paste_known=True, use_graph=True, lanes=None,
                           jump_length=None, n_resample=1):
        """The last state of masked_sample_loop_progressive."""
        final = None
        for sample in self.masked_sample_loop_progressive(model, shape, known, mask, sampler=sampler, eta=eta, noise=noise,
                                                          clip_denoised=clip_denoised, model_kwargs=model_kwargs, device=device,
                                                          progress=progress, paste_known=paste_known, use_graph=use_graph, lanes=lanes,
                                                          jump_length=jump_length, n_resample=n_resample):
            final = sample
        return final

    def masked_sample_loop_progressive(self, model, shape, known, mask=None, *, sampler="ddpm", eta=0.0, noise=None, clip_denoised=True,
                                       model_kwargs=None, device=None, progress=False, paste_known=True, use_graph=True, lanes=None,
                                       jump_length=None, n_resample=1):
        """The replacement method (gd:642-720) with partial masks, for the DDPM and the DDIM stepper.  known: {"video": [B,F,C,H,W],
        "audio": [B,C,L]}, either or both; mask: the known cells of these streams (masking.normalize has the shapes; a stream without a
        mask is known as a whole).  Before every step the known cells are set to q_sample(known, t, noise = that stream's x_T) by one
        mmd_cond_replace per stream - in front of the U-Net plan inside the step graph - then one ordinary p_sample (sampler="ddpm") or
        ddim_sample ("ddim", eta) follows, the reference's order.  With paste_known the LAST yielded state carries `known` itself on
        its known cells; the states before it are the raw step outputs.  noise: an optional x_T dict that doubles as the fixed
        conditioning noise; with a seeded.CounterNoise source x_T, the conditioning noise (regenerated in the kernel, no buffer) and the
        per-step noise all come from the counter and `noise` must be None.

        jump_length, n_resample (sampler="ddpm"): RePaint's resampling (Lugmayr et al., CVPR 2022).  The loop runs
        masking.repaint_schedule(T, jump_length, n_resample): whenever the state reaches a multiple m of jump_length with jumps left it is
        diffused forward again to level m + jump_length (one mmd_renoise_ctr per stream, or mmd_q_sample on fresh noise: video first,
        then audio) and those steps run again, n_resample times in all, so that the unknown cells are harmonised with the known ones.
        Every reverse step yields a state, a jump yields none, and the paste follows the last evaluation.  A repeated step draws noise
        and window shifts of its own (the schedule's draws).  The default, n_resample=1, is the plain loop."""
        from . import masking
        if sampler not in ("ddpm", "ddim"):
            raise H.MMDError(f"masked_sample_loop: unknown sampler {sampler!r} (ddpm or ddim)")
        sched = masking.repaint_schedule(self.num_timesteps, jump_length, n_resample)
        if sampler == "ddim" and int(n_resample) > 1:
            raise H.MMDError(f"masked_sample_loop: resampling jumps (n_resample={int(n_resample)}) ride the ddpm stepper, not ddim")
        if len(sched) == self.num_timesteps:
            sched = None                     # no jumps: the plain loop below, as it has always been
        device = self._sampling_device(device)
        cond = masking.to_device(masking.normalize(known, mask, shape), device)
        ctr = self._counter()
        if ctr is not None and noise is not None:
            raise H.MMDError("masked_sample_loop: a CounterNoise source draws x_T and the conditioning noise itself: noise must be None")
        if noise is None:
            noise = self._x_T(shape, device)
        noise = {k: noise[k].to(device).float().contiguous() for k in ("video", "audio")}
        B = shape["video"][0]
        model_kwargs = model_kwargs or {}
        stepper = self._graph_stepper(model, model_kwargs, use_graph, B, device, clip_denoised, update=sampler, eta=eta, lanes=lanes, cond=cond,
                                      jump_length=None if sched is None else int(jump_length))
        if stepper is not None:
            def paste(i):
                if paste_known and i == 0:
                    stepper.paste_known()
            stepper.load(noise["video"], noise["audio"])
            stepper.load_cond(cond, noise)
            if sched is None:
                yield from self._replay(stepper, self._indices(progress), after=paste)
            else:
                yield from self._replay_schedule(stepper, self._progress(sched, progress), paste_known)
            return
        _, qtab = self.device_tables(device)
        x = dict(noise)
        if sched is not None:
            yield from self._resampled_host_loop(model, x, noise, cond, sched, int(jump_length), B, device, clip_denoised, model_kwargs,
                                                 progress, paste_known)
            return
        for i in self._indices(progress):
            t = th.tensor([i] * B, device=device)
            x = dict(x)                      # the state yielded last, and at first x_T itself, stay as they are: a new dict, and copies below
            for k, c in cond.items():
                x[k] = x[k].clone()
                src = dict(ctr=(ctr.key(device), ctr.ids(B, device), 0 if k == "video" else 1)) if ctr is not None else dict(noise=noise[k])
                ops.cond_replace(x[k], c.known, qtab, t, mask=c.mask, **src)
            with th.no_grad():
                if sampler == "ddim":
                    x = self.ddim_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs, eta=eta)["sample"]
                else:
                    x = self.p_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs)["sample"]
            if paste_known and i == 0:
                for k, c in cond.items():
                    ops.cond_replace(x[k], c.known, None, None, mask=c.mask, coef=(1.0, 0.0))
            yield x

    @staticmethod
    def _progress(sched, progress):
        if progress:
            from tqdm.auto import tqdm
            sched = tqdm(sched)
        return sched

    @staticmethod
    def _replay_schedule(stepper, sched, paste_known):
        """Run masking.repaint_schedule's operations on a loaded stepper: a step replays the step graph at its own draw and yields the
        state, a jump replays the jump graph and yields nothing; the last operation of a schedule is step 0, after which the known cells
        are pasted.  The stepper is closed when the generator ends, is closed or is dropped."""
        try:
            for op, i, draw in sched:
                if op == "jump":
                    stepper.jump(i, draw)
                    continue
                stepper.step(i, draw=draw)
                if paste_known and i == 0:
                    stepper.paste_known()
                yield stepper.current()
        finally:
            stepper.close()

    def _resampled_host_loop(self, model, x, noise, cond, sched, jump_length, B, device, clip_denoised, model_kwargs, progress, paste_known):
        """masked_sample_loop's host loop over a schedule with jumps, launch by launch: the same operations at the same draws as the
        graph-replayed loop (a CounterNoise takes the schedule's draw through drawing_at; any other source is called in the same order)."""
        import contextlib
        ctr = self._counter()
        _, qtab = self.device_tables(device)
        jtab = self.jump_tables(jump_length, device)
        for op, i, draw in self._progress(sched, progress):
            t = th.tensor([i] * B, device=device)
            x = dict(x)                      # the state yielded last stays as it is
            if op == "jump":
                for k, tag in (("video", 0), ("audio", 1)):
                    x[k] = x[k].clone()
                    if ctr is not None:
                        ops.renoise_ctr(x[k], ctr.key(device), ctr.ids(B, device), tag, jtab, t, th.full_like(t, draw))
                    else:
                        ops.q_sample(x[k], self._randn_like(x[k]).float().contiguous(), x[k], jtab, t)
                continue
            for k, c in cond.items():
                x[k] = x[k].clone()
                src = dict(ctr=(ctr.key(device), ctr.ids(B, device), 0 if k == "video" else 1)) if ctr is not None else dict(noise=noise[k])
                ops.cond_replace(x[k], c.known, qtab, t, mask=c.mask, **src)
            with th.no_grad(), (ctr.drawing_at(draw) if ctr is not None else contextlib.nullcontext()):
                x = self.p_sample(model, x, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs)["sample"]
            if paste_known and i == 0:
                for k, c in cond.items():
                    ops.cond_replace(x[k], c.known, None, None, mask=c.mask, coef=(1.0, 0.0))
            yield x

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=True):
        final = None
        for sample in self.p_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                     denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs,
                                                     device=device, progress=progress):
            final = sample
        return final

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, use_graph=True):
        """gd:523-582.  x_T is drawn on the CPU (video, then audio) and moved to the device like the reference;
        every step then replays one captured hipGraph (U-Net plan + both fused updates).  With a denoised_fn (a host callable on the x_0
        prediction, gd:263-268) the steps are launched eagerly through p_sample."""
        if cond_fn is not None:
            raise NotImplementedError("cond_fn: see p_sample")
        device = self._sampling_device(device)
        x = self._x_T(shape, device)
        indices = self._indices(progress)
        stepper = self._graph_stepper(model, model_kwargs, use_graph, shape["video"][0], device, clip_denoised, denoised_fn=denoised_fn)
        if stepper is not None:
            stepper.load(x["video"], x["audio"])
            yield from self._replay(stepper, indices)
            return
        for i in indices:
            t = th.tensor([i] * shape["video"][0], device=device)
            with th.no_grad():
                out = self.p_sample(model, x, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, model_kwargs=model_kwargs)
            yield out["sample"]
            x = out["sample"]

    # ------------------------------------------------------------------ variational bound (bits / dim)
    def _vlb_stream(self, x_start, x_t, model_out, t, clip_denoised, geom, noise=None, tables=None, want_x0=False):
        """mmd_vlb_terms on one stream.  `tables` = (vb, xstart_mse, eps_mse) [N, T] result tables (sample n lands at column t[n]); without
        them fresh [N] vectors.  Returns (vb, xstart_mse, eps_mse or None, pred_xstart or None).  Evaluation only: a model output that
        carries a graph raises rather than yield a bound that looks like a loss and has no gradient."""
        H.require_cuda(x_start, x_t, model_out)
        if th.is_grad_enabled() and model_out.requires_grad:
            raise H.MMDError("variational bound: the model output requires grad and this evaluation is not differentiable (only the "
                             "tensor-valued _vb_terms_bpd with clip_denoised=False is) - call it under torch.no_grad()")
        tab, _ = self.device_tables(x_t.device)
        F, C, HW = geom
        x0, xt, mo = x_start.float().contiguous(), x_t.float().contiguous(), model_out.float().contiguous()
        N = x0.shape[0]
        if tables is None:
            tables = tuple(th.empty(N, dtype=th.float32, device=x0.device) for _ in range(3))
        vb, xs, em = tables
        px0 = th.empty_like(x0) if want_x0 else None
        nz = None if noise is None else noise.float().contiguous()
        ops.vlb_terms(x0, xt, mo, tab, t.to(th.int64).contiguous(), F, C, HW, self._flags(clip_denoised), vb, xstart_mse=xs,
                      eps_mse=em if nz is not None else None, noise=nz, pred_xstart=px0)
        return vb, xs, (em if nz is not None else None), px0

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """gd:1048-1092 -> {"output": {"video","audio"} [N] (KL for t > 0, decoder NLL at t == 0, bits / dim), "pred_xstart": {...}}."""
        video_output, audio_output = self._model_out2(model, x_t, t, model_kwargs)
        res = {"output": {}, "pred_xstart": {}}
        for key, mo in (("video", video_output), ("audio", audio_output)):
            vb, _, _, px0 = self._vlb_stream(x_start[key], x_t[key], mo, t, clip_denoised, _geom(x_t[key]), want_x0=True)
            res["output"][key], res["pred_xstart"][key] = vb, px0
        return res

    def _prior_bpd(self, x_start):
        """gd:1213-1229 on one stream's tensor: mean KL(q(x_T | x_0) || N(0, I)) / ln 2.  The KL kernel does it: a two-column table
        whose 'posterior' is q(x_T | x_0) (mean sqrt_ac[T-1] x_0, log-variance log(1 - ac[T-1])) against a model that predicts mean 0
        with log-variance 0, evaluated at column 1."""
        H.require_cuda(x_start)
        dev = x_start.device
        key = ("prior", str(dev))
        if key not in self._dev_tables:
            tab = np.zeros((7, 2))
            tab[1] = 1.0
            tab[2] = self.sqrt_alphas_cumprod[-1]
            tab[5] = self.log_one_minus_alphas_cumprod[-1]
            self._dev_tables[key] = th.from_numpy(tab).float().to(dev).contiguous()
        x0 = x_start.float().contiguous()
        N = x0.shape[0]
        zero = th.zeros_like(x0)
        out = th.empty(N, dtype=th.float32, device=dev)
        ops.vlb_terms(x0, zero, zero, self._dev_tables[key], th.ones(N, dtype=th.int64, device=dev), 1, 1, x0[0].numel(), 2, out)
        return out

    @staticmethod
    def _bpd_result(vb, xstart_mse, mse, prior):
        """Result tables indexed by t -> the reference's dict: it appends t = T-1 ... 0 and stacks, so column j is t = T-1-j."""
        vb, xstart_mse, mse = (a.flip(1) for a in (vb, xstart_mse, mse))
        return {"total_bpd": vb.sum(dim=1) + prior, "prior_bpd": prior, "vb": vb, "xstart_mse": xstart_mse, "mse": mse}

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, use_graph=True, lanes=None):
        """The whole bound (gd:1231-1286) on {"video","audio"}: total_bpd / prior_bpd [N] and vb / xstart_mse / mse [N, T], each as
        {"video": ..., "audio": ...}.  Per step t = T-1 ... 0: fresh noise (video first, then audio, through noise_source), x_t =
        q_sample, one model call (one window-shift draw per block through the model's shift_source), mmd_vlb_terms per stream into
        device tables; nothing comes back to the host until the caller reads the result.  With a plain MultimodalUNet the step is one
        graph replay per lane (sampler.GraphStepper, update="vlb"); use_graph=False launches the same kernels eagerly."""
        device = x_start["video"].device
        self._sampling_device(device)
        B, T = x_start["video"].shape[0], self.num_timesteps
        stepper = self._graph_stepper(model, model_kwargs, use_graph, B, device, clip_denoised, update="vlb", lanes=lanes)
        if stepper is not None:
            stepper.load_x0(x_start["video"], x_start["audio"])
            for _ in self._replay(stepper, self._indices(False), state=False):
                pass
            tabs = stepper.results()
        else:
            tabs = {k: tuple(th.zeros(B, T, dtype=th.float32, device=device) for _ in range(3)) for k in ("video", "audio")}
            for i in self._indices(False):
                t = th.tensor([i] * B, device=device)
                if self._counter() is not None:          # the callable form at this index, as the graph step does
                    self._counter().set_draw(i)
                noise = {"video": self._randn_like(x_start["video"]), "audio": self._randn_like(x_start["audio"])}
                x_t = {k: self.q_sample(x_start[k], t, noise=noise[k]) for k in ("video", "audio")}
                with th.no_grad():
                    video_output, audio_output = self._model_out2(model, x_t, t, model_kwargs)
                    for key, mo in (("video", video_output), ("audio", audio_output)):
                        self._vlb_stream(x_start[key], x_t[key], mo, t, clip_denoised, _geom(x_t[key]), noise=noise[key], tables=tabs[key])
        per = {k: self._bpd_result(*tabs[k], self._prior_bpd(x_start[k])) for k in ("video", "audio")}
        return {name: {k: per[k][name] for k in ("video", "audio")} for name in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")}

    # ------------------------------------------------------------------ training loss (forward value only for now)
    def multimodal_training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """gd:1114-1203: per-sample loss = mse_video + mse_audio (+ vb_video + vb_audio with learned-range variance; the vb term
        uses the frozen mean and clip_denoised=False, gd:1147-1174).  q_sample, the U-Net forward and the loss reductions run in
        libmmd; with autograd enabled the terms are differentiable (mmd_mse_grad / mmd_loss_terms_bwd feed the U-Net backward)."""
        model_kwargs = model_kwargs or {}
        if self.loss_type not in (LossType.MSE, LossType.RESCALED_MSE):
            raise NotImplementedError("KL / RESCALED_KL losses produce no terms in the reference either (gd:1143)")
        if noise is None:
            noise = {"video": self._randn_like(x_start["video"]), "audio": self._randn_like(x_start["audio"])}
        xt = {k: self.q_sample(x_start[k], t, noise=noise[k]) for k in ("video", "audio")}
        video_output, audio_output = model(xt["video"], xt["audio"], self._scale_timesteps(t), **model_kwargs)
        tab, _ = self.device_tables(xt["video"].device)
        learned = self.model_var_type == ModelVarType.LEARNED_RANGE
        flags = (2 if self.model_mean_type == ModelMeanType.START_X else 0) | (4 if learned else 0)
        vb_scale = self.num_timesteps / 1000.0 if self.loss_type == LossType.RESCALED_MSE else 1.0
        tgt = x_start if self.model_mean_type == ModelMeanType.START_X else noise
        t64 = t.to(th.int64).contiguous()
        term = {}
        if th.is_grad_enabled() and (video_output.requires_grad or audio_output.requires_grad):
            # differentiable loss: per-sample terms with their gradient kernels
            if learned:
                from .train_ops import LossTermsFn
                for key, mo in (("video", video_output), ("audio", audio_output)):
                    term[f"mse_{key}"], term[f"vb_{key}"] = LossTermsFn.apply(
                        mo, tgt[key].float().contiguous(), x_start[key].float().contiguous(), xt[key], tab, t64, _geom(xt[key]), flags, vb_scale)
                term["loss"] = (term["vb_video"] + term["vb_audio"]) + (term["mse_video"] + term["mse_audio"])
                return term
            from .train_ops import MseLossFn
            term["mse_video"] = MseLossFn.apply(video_output, tgt["video"])
            term["mse_audio"] = MseLossFn.apply(audio_output, tgt["audio"])
            term["loss"] = term["mse_video"] + term["mse_audio"]
            return term
        for key, mo in (("video", video_output), ("audio", audio_output)):
            F, C, HW = _geom(xt[key])
            mse, vb = ops.loss_terms(mo.float().contiguous(), tgt[key].float().contiguous(), tab, t64, F, C, HW, flags,
                                     x0=x_start[key].float().contiguous() if learned else None,
                                     xt=xt[key] if learned else None, vb_scale=vb_scale)
            if learned:
                term[f"vb_{key}"] = vb
            term[f"mse_{key}"] = mse
        # same accumulation order as the reference: (vb_video + vb_audio) then (mse_video + mse_audio)
        term["loss"] = (term["vb_video"] + term["vb_audio"] if learned else 0) + (term["mse_video"] + term["mse_audio"])
        return term
