#!/usr/bin/env python3
"""One training step of the shipped image super-resolution configuration (ssh_scripts/image_sr_train.sh: 64 -> 256, 192 channels, 4 heads,
2 ResBlocks per level, attention at ds 8 / 16 / 32, learned sigma, FiLM; 311.0 M parameters), timed eager and warm:
diffusion.training_losses forward + backward + flat AdamW / EMA at per-GPU batch --batch (6 in the script), bf16 activations.

    python tools/sr_train_bench.py [--batch 6] [--steps 10] [--warmup 3] [--dtype bf16] [--no-breakdown] [--guard {0,1}]

--guard 1 times the step with the on-device step guard (FlatAdamW(guard=True): mmd_sumsq_chunks + mmd_step_control +
mmd_adamw_step_guarded in place of mmd_adamw_step); 0, the default, is the unguarded step.  For an A/B run both arms in one job, one
process per arm; the breakdown lists the three launches by name.

Prints one JSON line: median / min / max step time over --steps steps (each step fenced by a device synchronize), images per second,
and - from ONE extra step in which every libmmd entry point is bracketed by HIP events on the launch stream - the time per entry point
(all of its kernels together), largest first, with the remainder of the step (torch's own small kernels: casts, pads, the
Bernoulli mask, autograd's gradient sums) as `other`.  The bracketed step serialises nothing that was parallel (one launch stream), but it
pays two event records per launch, so its total is reported separately and the table is given as shares."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))

import torch  # noqa: E402

SHIPPED = dict(large_size=256, small_size=64, sr_num_channels=192, sr_num_heads=4, sr_num_res_blocks=2, sr_attention_resolutions="8,16,32",
               sr_learn_sigma=True, sr_resblock_updown=True, sr_use_scale_shift_norm=True)


class EntryTimer:
    """Brackets every H.call(name, ..., stream) with two HIP events; totals per entry point after one synchronize."""

    def __init__(self):
        from mm_diffusion import _hip as H
        self.H, self.orig, self.spans, self.free = H, H.call, [], []

    def _event(self):
        e = ctypes.c_void_p()
        self.orig("mmd_event_create", ctypes.byref(e))
        return e

    def __enter__(self):
        H = self.H
        skip = ("mmd_event_", "mmd_graph_", "mmd_stream_")

        def call(name, *args):
            if name.startswith(skip):
                return self.orig(name, *args)
            st = H.stream_handle()
            a, b = self._event(), self._event()
            self.orig("mmd_event_record", a, st)
            out = self.orig(name, *args)
            self.orig("mmd_event_record", b, st)
            self.spans.append((name, a, b))
            return out
        H.call = call
        return self

    def __exit__(self, *exc):
        self.H.call = self.orig

    def totals(self):
        torch.cuda.synchronize()
        out, ms = {}, ctypes.c_float()
        for name, a, b in self.spans:
            self.orig("mmd_event_elapsed_ms", a, b, ctypes.byref(ms))
            t = out.setdefault(name, [0.0, 0])
            t[0] += ms.value
            t[1] += 1
            self.H.lib().mmd_event_destroy(a)
            self.H.lib().mmd_event_destroy(b)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--no-breakdown", action="store_true")
    ap.add_argument("--guard", type=int, choices=[0, 1], default=0)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    from mm_diffusion import logger, script_util as su
    from mm_diffusion.optim import FlatAdamW
    from mm_diffusion.synth import synth_tensor
    logger.set_quiet(True)
    dev = torch.device("cuda")
    d = su.image_sr_model_and_diffusion_defaults()
    d.update(SHIPPED)
    d.update(use_fp16=(args.dtype == "bf16"))
    model, diff = su.image_sr_create_model_and_diffusion(**d)
    model.load_state_dict({k: synth_tensor(k, v.shape) for k, v in model.state_dict().items()})
    model.to(dev).train()
    nparam = sum(p.numel() for p in model.parameters())
    opt = FlatAdamW(model.parameters(), lr=1e-4, weight_decay=0.0, ema_rates=[0.9999], pack_dtype=model.dtype, guard=bool(args.guard))
    g = torch.Generator().manual_seed(4321)
    torch.manual_seed(4321)
    B, L, S = args.batch, d["large_size"], d["small_size"]
    x0 = (torch.rand(B, 3, L, L, generator=g) * 2 - 1).to(dev)
    low = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev)

    def one_step():
        t = torch.randint(0, diff.num_timesteps, (B,), generator=g).to(dev)
        opt.zero_grad()
        terms = diff.training_losses(model, x0, t, model_kwargs={"low_res": low})
        loss = terms["loss"].mean()
        opt.arm_overlap()
        loss.backward()
        opt.all_reduce_grads()
        opt.step()
        return loss

    for _ in range(args.warmup):
        one_step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        loss = one_step()
        torch.cuda.synchronize()
        times.append(1000.0 * (time.perf_counter() - t0))
    med = statistics.median(times)
    res = {"metric": "SR training step (training_losses fwd + bwd + AdamW/EMA), 64 -> 256, eager", "ms_per_step_median": med,
           "ms_per_step_min": min(times), "ms_per_step_max": max(times), "steps": args.steps, "warmup": args.warmup, "batch": B, "guard": args.guard,
           "images_per_s": 1000.0 * B / med, "dtype": args.dtype, "parameters_M": nparam / 1e6, "loss_finite": bool(torch.isfinite(loss)),
           "peak_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30, "data": "synthetic", "weights": "key-seeded synthetic (mm_diffusion.synth)"}
    if not args.no_breakdown:
        t0 = time.perf_counter()
        with EntryTimer() as et:
            one_step()
            tot = et.totals()
        wall = 1000.0 * (time.perf_counter() - t0)
        inside = sum(v[0] for v in tot.values())
        table = {k: {"ms": round(v[0], 3), "calls": v[1], "share": round(v[0] / wall, 4)} for k, v in sorted(tot.items(), key=lambda kv: -kv[1][0])}
        table["other"] = {"ms": round(wall - inside, 3), "calls": None, "share": round((wall - inside) / wall, 4)}
        res["breakdown"] = {"bracketed_step_ms": wall, "entries": table,
                            "note": "one extra step, every libmmd entry point between two HIP events on the launch stream; `other` = the step's "
                                    "wall time outside them (torch's own kernels, host gaps, the event records themselves)"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
