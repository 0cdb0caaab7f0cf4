#!/usr/bin/env python3
"""DPM-Solver++ multistep loop: the eager host loop (DPM_Solver.sample, mmd_abs_quantile) against the graph-replayed one
(DPM_Solver.sample_graph), and the two quantile selections alone.  One call, one fresh process per arm, every arm under its own time limit.

    python tools/dpm_graph_bench.py [--out profiles/dpm_graph.txt] [--repeats 3]

Loop arms (bench.py --mode dpm's configuration: base model, bf16, predict_x0 + thresholding, order 2, logSNR, 50 evaluations), batch 2
and 4, `repeats` timed calls each after one warm-up call; the figure is ms per network evaluation (host clock around a device
synchronise):
    eager        sample(method="multistep")
    graph-multi  sample_graph, quantile by the multi-workgroup selection (mmd_dpmpp_x0's fused level 0 + mmd_dpmpp_select)
    graph-block  sample_graph, quantile by mmd_abs_quantile
Selection arms, the base model's stream sizes (video 16 x 3 x 64 x 64, audio 1 x 25600), batch 1 / 2 / 4, `repeats` repeats of 200 calls
each between device events; the figure is microseconds per call:
    select-block mmd_abs_quantile            select-multi mmd_dpmpp_select from scratch (all three levels + final)
    select-fused mmd_dpmpp_select with level 0 done (what the recorded step adds to mmd_dpmpp_x0)
The rule of ISSUE / DESIGN.md section 7 is evaluated at the end: the stepper keeps the multi-workgroup selection unless it is slower than
mmd_abs_quantile at the video size, batch 2, by more than the spread (max - min) of the old kernel's repeats in this call."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
sys.path.insert(0, ROOT)

LOOP_ARMS = ("eager", "graph-multi", "graph-block")
SELECT_ARMS = ("select-block", "select-multi", "select-fused")
SIZES = {"video": 16 * 3 * 64 * 64, "audio": 25600}
NFE = 50


def loop_arm(arm, repeats):
    import random
    import torch
    from bench import FULL
    from mm_diffusion import logger, multimodal_script_util as msu, sampler
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
    if arm != "eager":
        sampler.DPMPP_SELECT = arm.split("-")[1]
    res = {}
    for B in (2, 4):
        random.seed(99)
        torch.manual_seed(99)

        def call():
            x_T = {"video": torch.randn(B, *fl["video_size"], device="cuda"), "audio": torch.randn(B, *fl["audio_size"], device="cuda")}
            with torch.no_grad():
                if arm == "eager":
                    return solver.sample(x_T, steps=NFE, order=2, skip_type="logSNR", method="multistep")
                return solver.sample_graph(x_T, steps=NFE, order=2, skip_type="logSNR")
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            ms.append(1000 * (time.perf_counter() - t0) / NFE)
        res[f"batch{B}"] = {"ms_per_eval": ms, "finite": bool(torch.isfinite(out["video"]).all())}
    return res


def select_arm(arm, repeats, calls=200):
    import torch
    from mm_diffusion import ops
    res = {}
    for name, per in SIZES.items():
        for N in (1, 2, 4):
            g = torch.Generator().manual_seed(N)
            x = torch.randn(N, per, generator=g).cuda()
            out, ws = torch.empty(N, device="cuda"), ops.dpmpp_workspace(N, "cuda")
            tab = torch.tensor([[1.0], [0.0], [0.0], [0.0], [0.0], [0.0]], device="cuda")
            k = torch.zeros(N, dtype=torch.int64, device="cuda")
            x0 = torch.empty_like(x)

            def once():
                if arm == "select-block":
                    ops.abs_quantile(x, 0.995, out=out)
                elif arm == "select-multi":
                    ops.dpmpp_select(x, 0.995, out, ws)
                else:
                    ops.dpmpp_select(x0, 0.995, out, ws, level0_done=True)

            def fill():      # level 0 as the recorded step provides it (outside the timed window of select-fused)
                if arm == "select-fused":
                    ops.dpmpp_x0(x, x, x0, tab, k, 1, 1, 1, per, hist=ws)
            for _ in range(10):
                fill()
                once()
            torch.cuda.synchronize()
            us = []
            for _ in range(repeats):
                total = 0.0
                if arm == "select-fused":      # one event pair per call: the fill between the calls is not timed
                    for _ in range(calls):
                        fill()
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        once()
                        b.record()
                        b.synchronize()
                        total += a.elapsed_time(b)
                else:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        once()
                    b.record()
                    b.synchronize()
                    total = a.elapsed_time(b)
                us.append(1000 * total / calls)
            res[f"{name}_batch{N}"] = {"us_per_call": us, "value": [float(v) for v in out.cpu()]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, help="run one arm in this process and print its JSON line (the driver starts these)")
    ap.add_argument("--arms", default=",".join(SELECT_ARMS + LOOP_ARMS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpm_graph.txt"))
    ap.add_argument("--arm-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.arm:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("dpm_graph_bench needs a MI355X: a timing without one says nothing")
        res = loop_arm(args.arm, args.repeats) if args.arm in LOOP_ARMS else select_arm(args.arm, args.repeats)
        print("RESULT " + json.dumps({"arm": args.arm, "result": res}))
        return 0
    results, lines = {}, []
    for arm in args.arms.split(","):
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
    lines.append("tools/dpm_graph_bench.py: one call, one process per arm, %d repeats" % args.repeats)
    for arm in SELECT_ARMS:
        for key, r in results.get(arm, {}).items():
            us = r["us_per_call"]
            lines.append(f"{arm:13s} {key:13s} us/call " + " ".join(f"{v:8.2f}" for v in us) + f"   q0.995 {r['value']}")
    for arm in LOOP_ARMS:
        for key, r in results.get(arm, {}).items():
            lines.append(f"{arm:13s} {key:13s} ms/eval " + " ".join(f"{v:7.3f}" for v in r["ms_per_eval"]) + f"   finite {r['finite']}")
    if "select-block" in results and "select-multi" in results:
        old, new = results["select-block"]["video_batch2"]["us_per_call"], results["select-multi"]["video_batch2"]["us_per_call"]
        spread = max(old) - min(old)
        med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
        keep = med(new) <= med(old) + spread
        lines.append(f"rule (video size, batch 2): multi {med(new):.2f} us, block {med(old):.2f} us, spread of block {spread:.2f} us -> "
                     f"the stepper records the {'multi-workgroup selection' if keep else 'old kernel (mmd_abs_quantile)'}")
        same = all(results["select-block"][k]["value"] == results["select-multi"][k]["value"] for k in results["select-block"])
        lines.append(f"both selections return the same values on every shape: {same}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
