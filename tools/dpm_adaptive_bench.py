#!/usr/bin/env python3
"""Adaptive DPM-Solver++: the eager host loop (DPM_Solver.sample(method="adaptive"), one scalar read-back per trial step) against the
graph-replayed one with the controller on the device (DPM_Solver.sample_graph_adaptive).  One call, one fresh process per arm, every arm
under its own time limit; the call ends at the first arm that fails or runs out of time.

    python tools/dpm_adaptive_bench.py [--out profiles/dpm_adaptive_graph.txt] [--repeats 2]

Configuration: the base (Landscape) model, batch 2, bf16, and the reference sampling script's settings for `--sample_fn dpm_solver++` -
predict_x0=True, thresholding=True, order=2, method="adaptive" with the default tolerances.  Every arm starts from the same x_T and the
same window-shift stream.  Per arm one warm-up call (it also captures the graphs), then `repeats` timed calls (host clock around a
device synchronise).  Nothing is profiled here.
    eager         sample(order=2, method="adaptive")
    batch_poll1   sample_graph_adaptive(control="batch", poll=1)     the reference's step rule, a status read per trial step
    batch_poll4   sample_graph_adaptive(control="batch", poll=4)
    sample        sample_graph_adaptive(control="sample"), default lanes and poll: every sample its own step size
Reported per arm: trial steps replayed, accepted steps (per sample), network evaluations, wall time, ms per evaluation, host reads.
No ratio is evaluated: the weights are synthetic, and the number of trial steps an adaptive solver takes on a random-weight model says
nothing about a trained one - only the ms per evaluation and the host reads carry over."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
sys.path.insert(0, ROOT)

ARMS = {"eager": None, "batch_poll1": dict(control="batch", poll=1), "batch_poll4": dict(control="batch", poll=4), "sample": dict(control="sample")}
BATCH = 2


def run_arm(arm, repeats):
    import random
    import torch
    from bench import FULL
    from mm_diffusion import logger, multimodal_script_util as msu
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    fl = msu.model_and_diffusion_defaults()
    fl.update(FULL)
    fl.update(use_fp16=True)
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.to("cuda").eval()
    solver = DPM_Solver(model=model, alphas_cumprod=torch.tensor(diff.alphas_cumprod, dtype=torch.float32), predict_x0=True, thresholding=True)
    runs = []
    for i in range(repeats + 1):
        rng = random.Random(99)
        model.shift_source = lambda lo, hi: rng.randint(lo, hi)
        torch.manual_seed(99)
        x_T = {"video": torch.randn(BATCH, *fl["video_size"], device="cuda"), "audio": torch.randn(BATCH, *fl["audio_size"], device="cuda")}
        nfe = solver.nfe
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            if ARMS[arm] is None:
                out, stats = solver.sample(x_T, order=2, method="adaptive"), None
            else:
                out, stats = solver.sample_graph_adaptive(x_T, return_stats=True, **ARMS[arm])
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        evals = solver.nfe - nfe
        if i == 0:
            continue      # the warm-up call
        runs.append({"trials": evals // 2, "accepted": stats["accepted"].tolist() if stats else None, "evals": evals, "wall_s": wall,
                     "ms_per_eval": 1000 * wall / evals, "host_reads": stats["host_reads"] if stats else evals // 2,
                     "finite": bool(torch.isfinite(out["video"]).all() and torch.isfinite(out["audio"]).all())})
    return runs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", default=None, choices=list(ARMS), help="run one arm in this process and print its JSON line (the driver starts these)")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpm_adaptive_graph.txt"))
    ap.add_argument("--arm-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.arm:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("dpm_adaptive_bench needs a MI355X: a timing without one says nothing")
        print("RESULT " + json.dumps({"arm": args.arm, "result": run_arm(args.arm, args.repeats)}))
        return 0
    results = {}
    for arm in ARMS:
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--repeats", str(args.repeats)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=args.arm_timeout)
        except subprocess.TimeoutExpired:
            print(f"{arm}: no result within {args.arm_timeout} s - stopping here", flush=True)
            return 124
        text = p.stdout.decode(errors="replace")
        got = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:      # a fault in one arm ends the call: nothing more is started on the device
            print(f"{arm}: exit {p.returncode}\n{text[-2000:]}", flush=True)
            return p.returncode or 1
        results[arm] = json.loads(got[-1][7:])["result"]
        print(f"{arm}: {json.dumps(results[arm])}", flush=True)
    lines = ["tools/dpm_adaptive_bench.py: one call, one process per arm, %d timed calls after a warm-up; base model, batch %d, bf16, predict_x0, "
             "thresholding, order 2, default tolerances; same x_T and shift stream in every arm" % (args.repeats, BATCH)]
    for arm in ARMS:
        for r in results[arm]:
            acc = "-" if r["accepted"] is None else "/".join(str(a) for a in r["accepted"])
            lines.append(f"{arm:12s} trials {r['trials']:4d}  accepted {acc:>9s}  evals {r['evals']:4d}  wall {r['wall_s']:7.3f} s  "
                         f"ms/eval {r['ms_per_eval']:7.3f}  host reads {r['host_reads']:4d}  finite {r['finite']}")
    lines.append("synthetic weights: the trial and evaluation counts of a random-weight model say nothing about a trained one; no ratio is evaluated")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
