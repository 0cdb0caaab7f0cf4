#!/usr/bin/env python3
"""Single-step DPM-Solver loop: the eager host loop (DPM_Solver.sample(method="singlestep")) against the graph-replayed one
(DPM_Solver.sample_graph_singlestep).  One call, one fresh process per arm, every arm under its own time limit; the call ends at the first
arm that fails or runs out of time.

    python tools/dpm_single_bench.py [--out profiles/dpm_single_graph.txt] [--repeats 3]

Configuration: the base model, bf16, and the reference sampling script's call - noise prediction, steps=20, order=3, skip_type="logSNR",
method="singlestep" (20 network evaluations) - at batch 2 and 4.  Per arm one warm-up call, then `repeats` timed calls; the figure is ms
per network evaluation (host clock around a device synchronise).  Nothing is profiled here.
    eager   sample(...)
    graph   sample_graph_singlestep(...)
The rule evaluated at the end: at both batch sizes the graph arm's median is not above the eager arm's median plus
the eager arm's own spread (max - min) in this call."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
sys.path.insert(0, ROOT)

ARMS = ("eager", "graph")
BATCHES = (2, 4)
CALL = dict(steps=20, order=3, skip_type="logSNR", method="singlestep")


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
    solver = DPM_Solver(model=model, alphas_cumprod=torch.tensor(diff.alphas_cumprod, dtype=torch.float32))
    nfe = solver.singlestep_tables(**CALL)["rows"]
    res = {}
    for B in BATCHES:
        random.seed(99)
        torch.manual_seed(99)

        def call():
            x_T = {"video": torch.randn(B, *fl["video_size"], device="cuda"), "audio": torch.randn(B, *fl["audio_size"], device="cuda")}
            with torch.no_grad():
                return solver.sample(x_T, **CALL) if arm == "eager" else solver.sample_graph_singlestep(x_T, **CALL)
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            ms.append(1000 * (time.perf_counter() - t0) / nfe)
        res[f"batch{B}"] = {"ms_per_eval": ms, "finite": bool(torch.isfinite(out["video"]).all())}
    return res


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", default=None, choices=ARMS, help="run one arm in this process and print its JSON line (the driver starts these)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpm_single_graph.txt"))
    ap.add_argument("--arm-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.arm:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("dpm_single_bench needs a MI355X: a timing without one says nothing")
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
    lines = ["tools/dpm_single_bench.py: one call, one process per arm, %d repeats; base model, bf16, noise prediction, %s" %
             (args.repeats, ", ".join(f"{k}={v}" for k, v in CALL.items()))]
    for arm in ARMS:
        for key, r in results[arm].items():
            lines.append(f"{arm:6s} {key:7s} ms/eval " + " ".join(f"{v:7.3f}" for v in r["ms_per_eval"]) + f"   finite {r['finite']}")
    held = True
    for B in BATCHES:
        old, new = results["eager"][f"batch{B}"]["ms_per_eval"], results["graph"][f"batch{B}"]["ms_per_eval"]
        spread = max(old) - min(old)
        ok = median(new) <= median(old) + spread
        held = held and ok
        lines.append(f"rule batch {B}: graph median {median(new):.3f} ms, eager median {median(old):.3f} ms, spread of eager {spread:.3f} ms -> "
                     f"{'holds' if ok else 'FAILS'}")
    lines.append(f"acceptance condition (graph median <= eager median + eager spread at both batch sizes): {'held' if held else 'NOT held'}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
