"""Tensor-valued Gaussian diffusion for the image super-resolution stage (reference mm_diffusion/gaussian_diffusion.py:
119-795; driven by multimodal_sample_sr.py:186-253) on the MI355X HIP path.

Shares the schedule tables, the fused update kernels (mmd_ddpm_update / mmd_ddim_update, learned-range variance included)
and the helper combinations with the multimodal class; only the sampling surface differs: states are `[N, C, H, W]` tensors,
`p_sample_loop` / `ddim_sample_loop` take `noise=` and `model_kwargs=` (the SR script passes `low_res` and a noise tensor
repeated over the frames of a clip) and return the final sample tensor.

Reference behaviours kept: `p_sample_loop` hands its `noise` argument down to `p_sample`, so when a start noise is given
the SAME tensor is re-used as the per-step noise of every step (gd:547-556, 423-424); `ddim_sample` always draws fresh noise
(gd:661); `ddim_sample_loop_progressive` defaults to eta = 0.5 while `ddim_sample_loop` defaults to 0.0 (gd:725,759).
`training_losses` (gd:850-927; py_scripts/image_sr_train.py through train_util.TrainLoop) runs q_sample, the model and the MSE /
learned-range vb reductions in libmmd and is differentiable when the model output carries a grad_fn; with LossType.KL / RESCALED_KL
(`--use_kl True`, gd:872-882) the loss is the bound term itself with the mean live (mmd_vlb_terms / mmd_vlb_terms_bwd).
`_vb_terms_bpd`, `_prior_bpd` and `calc_bpd_loop` (gd:796-829, 935-1008) evaluate the variational bound in bits / dim: one reduction
kernel per step writes into device result tables, read back once at the end.
Not built: cond_fn (classifier guidance)."""
import torch as th

from . import _hip as H
from . import ops
from .multimodal_gaussian_diffusion import (GaussianDiffusion as _Base, LossType, ModelMeanType, ModelVarType,  # noqa: F401
                                            get_named_beta_schedule, betas_for_alpha_bar, mean_flat)
from .seeded import CounterNoise, TAG_IMAGE


def _geom4(x):
    if x.dim() == 4:
        return 1, x.shape[1], x.shape[2] * x.shape[3]
    raise ValueError(f"expected an image batch [N,C,H,W], got {tuple(x.shape)}")


class GaussianDiffusion(_Base):
    """Same constructor / tables as the multimodal class (gd:119-170)."""

    def _model_out(self, model, x, t, model_kwargs):
        out = model(x, self._scale_timesteps(t), **(model_kwargs or {}))
        return out.float().contiguous()

    def _upd(self, model_output, x, t, clip_denoised, noise, want):
        tab, _ = self.device_tables(x.device)
        F, C, HW = _geom4(x)
        xs = x.float().contiguous()
        res = {k: th.empty_like(xs) for k in want}
        outs = dict(x0_out=res.get("pred_xstart"), mean_out=res.get("mean"), logvar_out=res.get("log_variance"))
        if isinstance(noise, CounterNoise):      # drawn in the kernel: counter (element, t, sample id, TAG_IMAGE)
            ops.ddpm_update_ctr(xs, model_output, noise.key(xs.device), noise.ids(xs.shape[0], xs.device), TAG_IMAGE, res.get("sample"), tab,
                                t.to(th.int64).contiguous(), F, C, HW, self._flags(clip_denoised), **outs)
        else:
            ops.ddpm_update(xs, model_output, noise, res.get("sample"), tab, t.to(th.int64).contiguous(), F, C, HW, self._flags(clip_denoised),
                            **outs)
        return res

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """gd:230-328 -> {'mean', 'variance', 'log_variance', 'pred_xstart'} tensors."""
        if denoised_fn is not None:
            raise NotImplementedError("denoised_fn is not supported by the fused update kernel")
        H.require_cuda(x)
        assert t.shape == (x.shape[0],)
        mo = self._model_out(model, x, t, model_kwargs)
        r = self._upd(mo, x, t, clip_denoised, None, ("mean", "log_variance", "pred_xstart"))
        r["variance"] = th.exp(r["log_variance"])
        return r

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, noise=None):
        """gd:400-449: fresh N(0,1) noise unless a noise tensor is handed in."""
        if cond_fn is not None or denoised_fn is not None:
            raise NotImplementedError("cond_fn / denoised_fn are not built for the SR stage")
        H.require_cuda(x)
        mo = self._model_out(model, x, t, model_kwargs)
        if noise is None:
            ctr = self._counter()
            noise = self._randn_like(x) if ctr is None else ctr
            if ctr is not None:
                ctr.set_draw(t)
        r = self._upd(mo, x, t, clip_denoised, noise if isinstance(noise, CounterNoise) else noise.float().contiguous(), ("sample", "pred_xstart"))
        return {"sample": r["sample"], "pred_xstart": r["pred_xstart"]}

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, device=None,
                      progress=True, cond_range=[0, 1000]):
        final = None
        for sample in self.p_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                     cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, progress=progress,
                                                     cond_range=cond_range):
            final = sample
        return final["sample"]

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                  device=None, progress=False, cond_range=[0, 1000]):
        if cond_fn is not None:
            raise NotImplementedError("cond_fn is not built for the SR stage")
        device = self._sampling_device(device)
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else self._start_noise(shape, TAG_IMAGE, device)
        for i in self._indices(progress):
            t = th.tensor([i] * shape[0], device=device)
            with th.no_grad():
                out = self.p_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs=model_kwargs, noise=noise)
            yield out
            img = out["sample"]

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, eta=0.0):
        """gd:626-674."""
        if cond_fn is not None or denoised_fn is not None:
            raise NotImplementedError("cond_fn / denoised_fn are not built for the SR stage")
        H.require_cuda(x)
        mo = self._model_out(model, x, t, model_kwargs)
        tab, _ = self.device_tables(x.device)
        F, C, HW = _geom4(x)
        xs = x.float().contiguous()
        out, x0 = th.empty_like(xs), th.empty_like(xs)
        ctr = self._counter()
        if ctr is not None:
            ctr.set_draw(t)
            ops.ddim_update_ctr(xs, mo, ctr.key(xs.device), ctr.ids(xs.shape[0], xs.device), TAG_IMAGE, out, tab, self.ddim_tables(xs.device),
                                t.to(th.int64).contiguous(), F, C, HW, self._flags(clip_denoised), eta, x0_out=x0)
            return {"sample": out, "pred_xstart": x0}
        noise = self._randn_like(xs).float().contiguous()
        ops.ddim_update(xs, mo, noise, out, tab, self.ddim_tables(xs.device), t.to(th.int64).contiguous(), F, C, HW, self._flags(clip_denoised),
                        eta, x0_out=x0)
        return {"sample": out, "pred_xstart": x0}

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, device=None,
                         progress=False, eta=0.0):
        final = None
        for sample in self.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                                        cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, progress=progress, eta=eta):
            final = sample
        return final["sample"]

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                     device=None, progress=False, eta=0.5):
        device = self._sampling_device(device if device is not None else next(model.parameters()).device)
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else (th.randn(*shape, device=device) if self._counter() is None else self._start_noise(shape, TAG_IMAGE, device))
        for i in self._indices(progress):
            t = th.tensor([i] * shape[0], device=device)
            with th.no_grad():
                out = self.ddim_sample(model, img, t, clip_denoised=clip_denoised, cond_fn=cond_fn, model_kwargs=model_kwargs, eta=eta)
            yield out
            img = out["sample"]

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None):
        """gd:850-927 -> per-sample {"loss", "mse"[, "vb"]}: MSE / RESCALED_MSE with fixed or learned-range variance (the vb term sees the
        mean prediction detached and clip_denoised=False, gd:887-901; RESCALED_MSE scales it by num_timesteps / 1000); KL / RESCALED_KL
        -> {"loss"} alone (RESCALED_KL times num_timesteps)."""
        H.require_cuda(x_start)
        if self.loss_type.is_vb():          # gd:872-882: the bound term itself, mean live, clip off
            if noise is None:
                noise = self._randn_like(x_start)
            xt = self.q_sample(x_start, t, noise=noise)
            loss = self._vb_terms_bpd(model, x_start, xt, t, clip_denoised=False, model_kwargs=model_kwargs)["output"]
            return {"loss": loss * self.num_timesteps if self.loss_type == LossType.RESCALED_KL else loss}
        if noise is None:
            noise = self._randn_like(x_start)
        xt = self.q_sample(x_start, t, noise=noise)
        mo = self._model_out(model, xt, t, model_kwargs)      # SpacedDiffusion maps the timesteps in there; fp32, keeps the grad_fn
        tab, _ = self.device_tables(xt.device)
        learned = self.model_var_type == ModelVarType.LEARNED_RANGE
        flags = (2 if self.model_mean_type == ModelMeanType.START_X else 0) | (4 if learned else 0)
        vb_scale = self.num_timesteps / 1000.0 if self.loss_type == LossType.RESCALED_MSE else 1.0
        tgt = (x_start if self.model_mean_type == ModelMeanType.START_X else noise).float().contiguous()
        x0 = x_start.float().contiguous()
        t64 = t.to(th.int64).contiguous()
        F, C, HW = _geom4(xt)
        N = xt.shape[0]
        terms = {}
        if th.is_grad_enabled() and mo.requires_grad:
            if learned:
                from .train_ops import LossTermsFn
                terms["mse"], terms["vb"] = LossTermsFn.apply(mo.reshape(N, 1, 2 * C, HW), tgt.reshape(N, 1, C, HW), x0.reshape(N, 1, C, HW),
                                                              xt.reshape(N, 1, C, HW), tab, t64, (F, C, HW), flags, vb_scale)
            else:
                from .train_ops import MseLossFn
                terms["mse"] = MseLossFn.apply(mo, tgt)
        else:
            mo = mo.float().contiguous()
            mse, vb = ops.loss_terms(mo.reshape(N, 1, -1, HW), tgt.reshape(N, 1, C, HW), tab, t64, F, C, HW, flags,
                                     x0=x0.reshape(N, 1, C, HW) if learned else None, xt=xt.reshape(N, 1, C, HW) if learned else None,
                                     vb_scale=vb_scale)
            terms["mse"] = mse
            if learned:
                terms["vb"] = vb
        terms["loss"] = terms["mse"] + terms["vb"] if "vb" in terms else terms["mse"]
        return terms

    # ------------------------------------------------------------------ variational bound (bits / dim)
    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """gd:796-829 -> {"output" [N] (KL for t > 0, decoder NLL at t == 0, bits / dim), "pred_xstart"}.  Differentiable w.r.t. the model
        output (mean and variance channels) when it carries a grad_fn; that needs clip_denoised=False, as training_losses uses it.
        To EVALUATE with the default clip_denoised=True, call it under torch.no_grad(): a model with trainable parameters called with
        autograd on runs its training walk and its output requires grad, and the clipped bound then raises (the gradient through the
        clamp is not built, and a detached value in its place would be a silent fallback)."""
        H.require_cuda(x_start, x_t)
        mo = self._model_out(model, x_t, t, model_kwargs)
        F, C, HW = _geom4(x_t)
        N = x_t.shape[0]
        if th.is_grad_enabled() and mo.requires_grad:
            if clip_denoised:
                raise NotImplementedError("_vb_terms_bpd: the gradient through the clipped x_0 prediction is not built: evaluate under "
                                          "torch.no_grad(), or pass clip_denoised=False for a differentiable bound")
            from .train_ops import VlbTermsFn
            tab, _ = self.device_tables(x_t.device)
            vb, px0 = VlbTermsFn.apply(mo.reshape(N, 1, -1, HW), x_start.float().reshape(N, 1, C, HW).contiguous(),
                                       x_t.float().reshape(N, 1, C, HW).contiguous(), tab, t.to(th.int64).contiguous(), (F, C, HW),
                                       self._flags(False))
            return {"output": vb, "pred_xstart": px0.reshape(x_t.shape)}
        vb, _, _, px0 = self._vlb_stream(x_start, x_t, mo, t, clip_denoised, (F, C, HW), want_x0=True)
        return {"output": vb, "pred_xstart": px0}

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None):
        """gd:953-1008 -> total_bpd / prior_bpd [N], vb / xstart_mse / mse [N, T] (column j is t = T-1-j, the reference's stacking order).
        Per step: fresh noise through noise_source, q_sample, the model, mmd_vlb_terms into device tables - no host sync in the loop."""
        H.require_cuda(x_start)
        device, N, T = x_start.device, x_start.shape[0], self.num_timesteps
        tabs = tuple(th.zeros(N, T, dtype=th.float32, device=device) for _ in range(3))
        geom = _geom4(x_start)
        for i in self._indices(False):
            t = th.tensor([i] * N, device=device)
            if self._counter() is not None:          # the callable form at this index
                self._counter().set_draw(i)
            noise = self._randn_like(x_start)
            x_t = self.q_sample(x_start, t, noise=noise)
            with th.no_grad():
                mo = self._model_out(model, x_t, t, model_kwargs)
                self._vlb_stream(x_start, x_t, mo, t, clip_denoised, geom, noise=noise, tables=tabs)
        return self._bpd_result(*tabs, self._prior_bpd(x_start))

    # the multimodal dict-valued entry points do not apply to the tensor-valued process
    def multimodal_training_losses(self, *a, **kw):
        raise NotImplementedError("tensor-valued diffusion: use the multimodal class for {'video','audio'} states")

    conditional_p_sample_loop = multimodal_training_losses

    def ddim_encode_loop(self, *a, **kw):
        raise H.MMDError("DDIM inversion (ddim_encode_loop, ddim_decode_loop, ddim_interpolate and their progressive forms) is built for the "
                         "multimodal {'video','audio'} process only: the tensor-valued SR stage has no inversion loop")

    ddim_encode_loop_progressive = ddim_decode_loop = ddim_decode_loop_progressive = ddim_interpolate = ddim_encode_loop
