"""Training loop of the image super-resolution stage on the MI355X HIP path (reference mm_diffusion/train_util.py:34-330 as driven
by py_scripts/image_sr_train.py:38-58): `self.data` yields `(low_res, batch, sr, cond)`, `run_step(batch, cond)` runs the
microbatched forward / backward of `diffusion.training_losses(model, batch, t, model_kwargs=cond)` (cond carries `low_res`), AdamW,
EMA copies, lr anneal, `modelNNNNNN.pt` / `ema_<rate>_NNNNNN.pt` / `optNNNNNN.pt` checkpoints with the reference's keys, and resume.

Everything but the batch handling is multimodal_train_util.TrainLoop (flat fp32 parameter / gradient / moment buffers, one-kernel
AdamW + EMA, one all-reduce per step, bf16 activations without loss scaling, the on-device non-finite skip / norm logging /
clipping of `guard_nonfinite` and `max_grad_norm`); this class only replaces what depends on the batch
being one image tensor instead of a {"video", "audio"} dict.

Deviation from the reference, on purpose: its `forward_backward` returns from INSIDE the microbatch loop (train_util.py:380), so
with `microbatch < batch_size` only the first microbatch ever contributes a gradient.  Here every microbatch contributes and each is
weighted by its share of the batch (the reference's `loss / scale`, scale = batch / microbatch); with the shipped `--microbatch -1`
(one microbatch) the two agree.  The periodic sample dump (`save_sr`) writes a png grid of [low_res upsampled | sample | target]
rows when PIL is importable and is skipped with a log line otherwise; wandb (`use_db`) is not built.
"""
import os

import torch as th
import torch.distributed as dist

from . import dist_util, logger
from .multimodal_train_util import (TrainLoop as _MultimodalTrainLoop, find_ema_checkpoint, find_resume_checkpoint,  # noqa: F401
                                    finite_pairs, get_blob_logdir, log_loss_dict, parse_resume_step_from_filename)
from .resample import LossAwareSampler


class TrainLoop(_MultimodalTrainLoop):
    log_stream_norms = False      # one image stream: no grad_norm_v / grad_norm_a

    def __init__(self, *, model, diffusion, data, batch_size, microbatch, ema_rate, log_interval, save_interval, resume_checkpoint,
                 lr=0, t_lr=1e-4, train_type=None, save_type="png", use_fp16=False, fp16_scale_growth=1e-3, schedule_sampler=None,
                 weight_decay=0.0, lr_anneal_steps=0, class_cond=False, use_db=False, sample_fn="ddpm", audio_fps=16000, num_classes=0,
                 save_row=8, guard_nonfinite=True, max_grad_norm=0.0):
        if class_cond:
            raise NotImplementedError("class-conditional SR training is not built")
        self.train_type = train_type
        self._last = None          # (low_res, batch, sr) of the latest step, for the sample dump
        super().__init__(model=model, diffusion=diffusion, data=data, batch_size=batch_size, microbatch=microbatch, ema_rate=ema_rate,
                         log_interval=log_interval, save_interval=save_interval, resume_checkpoint=resume_checkpoint, lr=lr, t_lr=t_lr,
                         save_type=save_type, use_fp16=use_fp16, fp16_scale_growth=fp16_scale_growth, schedule_sampler=schedule_sampler,
                         weight_decay=weight_decay, lr_anneal_steps=lr_anneal_steps, class_cond=class_cond, use_db=use_db,
                         sample_fn=sample_fn, num_classes=num_classes, save_row=save_row, audio_fps=audio_fps, use_graph=False,
                         guard_nonfinite=guard_nonfinite, max_grad_norm=max_grad_norm)

    def run_loop(self):
        while not self.lr_anneal_steps or self.step + self.resume_step < self.lr_anneal_steps:
            low_res, batch, sr, cond = next(self.data)
            self._last = (low_res, batch, sr)
            self.run_step(batch, cond)
            if self.step % self.log_interval == 0:
                logger.dumpkvs()
            if self.step % self.save_interval == 0:
                self.save()
                if "low_res" in cond:
                    self.save_sr()
                if os.environ.get("DIFFUSION_TRAINING_TEST", "") and self.step > 0:
                    return
            self.step += 1
        if (self.step - 1) % self.save_interval != 0:       # save the last checkpoint if it wasn't already saved
            self.save()

    def forward_backward(self, batch, cond):
        dev = dist_util.dev()
        batch = batch.to(dev)
        cond = {k: v.to(dev) for k, v in cond.items()}
        n = batch.shape[0]
        losses = None
        for i in range(0, n, self.microbatch):
            micro = batch[i:i + self.microbatch]
            micro_cond = {k: v[i:i + self.microbatch] for k, v in cond.items()}
            ts, weights = self.schedule_sampler.sample(micro.shape[0], dev)
            losses = self.diffusion.training_losses(self.model, micro, ts, model_kwargs=micro_cond)
            if isinstance(self.schedule_sampler, LossAwareSampler):
                self.schedule_sampler.update_with_local_losses(*finite_pairs(ts, losses["loss"].detach()))
            loss = (losses["loss"] * weights).mean() * (micro.shape[0] / n)
            log_loss_dict(self.diffusion, ts, {k: v * weights for k, v in losses.items()})
            if i + self.microbatch >= n:                      # last microbatch: gradient buckets are reduced while it is still running
                self.opt.arm_overlap()
            loss.backward()                                   # accumulates straight into the flat gradient buffer
        return losses

    def save_video(self):
        raise NotImplementedError("the SR loop dumps samples with save_sr()")

    def save_sr(self):
        """Sample dump of the latest batch (reference train_util.py save_sr): super-resolve its low_res images from the first EMA copy
        with `sample_fn` (dpm_solver / dpm_solver++: 50-evaluation multistep order 2 like the reference; ddim; else the DDPM loop) and write `<sample_fn>_samples_steps<N>.png`, one row [low_res | sample | target]
        per image.  The master parameters are swapped out and back, never overwritten."""
        try:
            import PIL  # noqa: F401
        except ImportError:
            logger.log("save_sr: PIL is not importable, sample dump skipped")
            return None
        if self._last is None:
            return None
        dev = dist_util.dev()
        low_res, batch, sr = self._last
        k = max(1, min(batch.shape[0], self.save_row))
        low, hr, up = low_res[:k].to(dev), batch[:k], sr[:k]
        was_training = self.model.training
        keep = None
        if self.opt.ema_params:
            keep = self.opt.flat.clone()
            self.opt.flat.copy_(self.opt.ema_params[0])
            self._params_changed()
        self.model.eval()
        try:
            with th.no_grad():
                if self.sample_fn in ("dpm_solver", "dpm_solver++"):      # the script's default: 50 evaluations (reference save_sr)
                    from .dpm_solver_plus import DPM_Solver
                    solver = DPM_Solver(model=self.model, alphas_cumprod=th.tensor(self.diffusion.alphas_cumprod, dtype=th.float32),
                                        predict_x0=self.sample_fn == "dpm_solver++", model_kwargs={"low_res": low})
                    sample = solver.sample(th.randn(*hr.shape).to(dev), steps=50, order=2, skip_type="time_uniform", method="multistep")
                else:                                                     # "ddim", else the DDPM loop over every timestep of the diffusion
                    fn = self.diffusion.ddim_sample_loop if self.sample_fn == "ddim" else self.diffusion.p_sample_loop
                    sample = fn(self.model, tuple(hr.shape), clip_denoised=True, model_kwargs={"low_res": low}, device=dev, progress=False)
        finally:
            if keep is not None:
                self.opt.flat.copy_(keep)
                self._params_changed()
            self.model.train(was_training)
        path = os.path.join(logger.get_dir(), f"{self.sample_fn}_samples_steps{self.step}.png")
        if dist_util.rank() == 0:
            from .common import save_png
            rows = th.cat([up.float().cpu(), sample.float().cpu(), hr.float().cpu()], dim=3)          # [k, 3, L, 3L]
            grid = th.cat(list(rows), dim=1)                                                          # [3, k*L, 3L]
            save_png(((grid + 1) * 127.5).clamp(0, 255).to(th.uint8).permute(1, 2, 0).numpy(), path)
            logger.log(f"{k} has sampled -> {path}")
        if dist.is_initialized():
            dist.barrier()
        return path
