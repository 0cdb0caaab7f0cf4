#!/usr/bin/env python3
"""Masked sampling with resampling jumps against the plain masked loop of the same build: ms per network evaluation.

    python tools/repaint_bench.py [--out profiles/repaint.txt] [--repeats 10]

One process, the two arms alternating call by call (a same-call comparison: both see the same clocks and neighbours).  Configuration:
the base model, bf16, batch 4, timestep_respacing="50", clip continuation from 4 known frames (masking.prefix_masks), CounterNoise(42),
graph replay with the default lanes.
    plain       masked_sample_loop(...)                                   50 evaluations
    resampled   masked_sample_loop(..., jump_length=10, n_resample=2)     90 evaluations + 4 jumps
Per arm one warm-up call (it captures the graphs), then `repeats` timed calls; the figure is the call's time (host clock around a device
synchronise) over its evaluations, and the median over the repeats.  The resampled arm's figure carries its jumps - one element-wise launch
per stream per jump - and the second graph's launches.  Synthetic weights: the figure says nothing about what resampling does to a clip."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
sys.path.insert(0, ROOT)

B, RESPACING, FRAMES, JUMP, RESAMPLE = 4, "50", 4, 10, 2
ARMS = {"plain": {}, "resampled": dict(jump_length=JUMP, n_resample=RESAMPLE)}


def median(v):
    s = sorted(v)
    return 0.5 * (s[(len(s) - 1) // 2] + s[len(s) // 2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repaint.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("repaint_bench needs a MI355X: a timing without one says nothing")
    from bench import FULL
    from mm_diffusion import logger, masking, multimodal_script_util as msu
    from mm_diffusion.seeded import CounterNoise
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    fl = msu.model_and_diffusion_defaults()
    fl.update(FULL)
    fl.update(use_fp16=True, timestep_respacing=RESPACING)
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.to("cuda").eval()
    diff.noise_source = CounterNoise(42)
    shape = {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}
    g = torch.Generator().manual_seed(1)
    known = {k: (0.5 * torch.randn(*shape[k], generator=g)).cuda() for k in shape}
    masks = masking.prefix_masks(fl["video_size"], fl["audio_size"], FRAMES)
    evals = {a: sum(op == "step" for op, _, _ in masking.repaint_schedule(diff.num_timesteps, kw.get("jump_length"), kw.get("n_resample", 1)))
             for a, kw in ARMS.items()}

    def call(arm):
        t0 = time.perf_counter()
        out = diff.masked_sample_loop(model, shape, known, masks, device=torch.device("cuda"), **ARMS[arm])
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0) / evals[arm], out
    ms, finite = {a: [] for a in ARMS}, {}
    for a in ARMS:
        call(a)
    for _ in range(args.repeats):
        for a in ARMS:
            t, out = call(a)
            ms[a].append(t)
            finite[a] = bool(torch.isfinite(out["video"]).all() and torch.isfinite(out["audio"]).all())
    lines = [f"tools/repaint_bench.py: one process, arms alternating, {args.repeats} repeats; base model, bf16, batch {B}, timestep_respacing={RESPACING}, "
             f"{FRAMES} known frames, CounterNoise(42), graph replay; resampled = jump_length={JUMP}, n_resample={RESAMPLE}"]
    for a in ARMS:
        lines.append(f"{a:10s} {evals[a]:3d} evaluations  ms/eval " + " ".join(f"{v:7.3f}" for v in ms[a]) + f"   finite {finite[a]}")
    p, r = median(ms["plain"]), median(ms["resampled"])
    lines.append(f"median ms per evaluation: plain {p:.3f}, resampled {r:.3f} ({100 * (r / p - 1):+.2f} %); spread (max - min) plain "
                 f"{max(ms['plain']) - min(ms['plain']):.3f}, resampled {max(ms['resampled']) - min(ms['resampled']):.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
