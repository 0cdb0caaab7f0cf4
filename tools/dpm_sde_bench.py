#!/usr/bin/env python3
"""SDE-DPM-Solver++ graph loop (DPM_Solver.sample_graph_sde) against the deterministic multistep loop (sample_graph) in the same call, and
the update launches alone.  One call, one fresh process per arm, every arm under its own time limit.

    python tools/dpm_sde_bench.py [--out profiles/dpm_sde_graph.txt] [--repeats 3]

Loop arms (bench.py --mode dpm's configuration: base model, bf16, predict_x0, order 2, logSNR, 50 evaluations, batch 2), one process per
thresholding setting ("loop-thr", "loop-plain"); inside it, for the noise from a seeded.CounterNoise and from buffers, one warm-up call
of each loop and then `repeats` timed calls of each, ALTERNATING deterministic / stochastic; the figure is ms per network evaluation (host
clock around a device synchronise).  The yardstick of the stochastic loop is the deterministic line next to it: box-to-box spread
exceeds one update kernel's cost.
Update arm ("update"): the base model's stream sizes (video 16 x 3 x 64 x 64, audio 1 x 25600), batch 2, `repeats` repeats of 200 calls
between device events, microseconds per call: mmd_dpmpp_update, mmd_dpmpp_sde_update (noise in memory), mmd_dpmpp_sde_update_ctr on a
second-order row, and mmd_ddpm_update / mmd_ddpm_update_ctr for the expectation
    stochastic evaluation = deterministic evaluation + about what mmd_ddpm_update_ctr costs over mmd_ddpm_update, per stream
(the streams' updates run side by side on two streams, so the sum over the streams is an upper estimate), which the last lines state."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
sys.path.insert(0, ROOT)

LOOP_ARMS = ("loop-thr", "loop-plain")
ARMS = ("update",) + LOOP_ARMS
GEOM = {"video": (16, 3, 64 * 64), "audio": (1, 1, 25600)}
NFE, BATCH = 50, 2


def med(v):
    return sorted(v)[len(v) // 2]


def loop_arm(arm, repeats):
    import random
    import torch
    from bench import FULL
    from mm_diffusion import logger, multimodal_script_util as msu
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    from mm_diffusion.seeded import CounterNoise
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    fl = msu.model_and_diffusion_defaults()
    fl.update(FULL)
    fl.update(use_fp16=True)
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.to("cuda").eval()
    ac = torch.tensor(diff.alphas_cumprod, dtype=torch.float32)
    # one solver per loop: each keeps its own stepper, so the alternating calls replay and never re-capture
    solvers = {kind: DPM_Solver(model=model, alphas_cumprod=ac, predict_x0=True, thresholding=(arm == "loop-thr")) for kind in ("det", "sde")}
    shape = {"video": (BATCH, *fl["video_size"]), "audio": (BATCH, *fl["audio_size"])}
    res = {}
    for noise in ("counter", "buffer"):
        random.seed(99)
        torch.manual_seed(99)

        def call(kind):
            kw = dict(steps=NFE, order=2, skip_type="logSNR")
            if noise == "counter":
                kw.update(shape=shape, noise_source=CounterNoise(7))
            else:
                kw.update(x_T={k: torch.randn(*shape[k], device="cuda") for k in ("video", "audio")})
            fn = solvers[kind].sample_graph if kind == "det" else solvers[kind].sample_graph_sde
            with torch.no_grad():
                return fn(**kw)
        for kind in ("det", "sde"):
            call(kind)
        torch.cuda.synchronize()
        ms = {"det": [], "sde": []}
        finite = {}
        for _ in range(repeats):
            for kind in ("det", "sde"):
                t0 = time.perf_counter()
                out = call(kind)
                torch.cuda.synchronize()
                ms[kind].append(1000 * (time.perf_counter() - t0) / NFE)
                finite[kind] = bool(torch.isfinite(out["video"]).all() and torch.isfinite(out["audio"]).all())
        res[noise] = {"ms_per_eval": ms, "finite": finite}
    return res


def update_arm(repeats, calls=200):
    import torch
    from mm_diffusion import ops
    N = BATCH
    res = {}
    for name, (F, C, HW) in GEOM.items():
        g = torch.Generator().manual_seed(3)
        x, m0, m1, z = (torch.randn(N, F, C, HW, generator=g).cuda() for _ in range(4))
        tab = torch.tensor([[1.0], [0.0], [0.61], [1.325], [-0.4417], [1.0]], device="cuda")      # one second-order row
        cz = torch.tensor([0.4262], device="cuda")
        k = torch.zeros(N, dtype=torch.int64, device="cuda")
        T = 4
        tables = torch.rand(7, T, generator=g).cuda() * 0.5 + 0.25
        t = torch.ones(N, dtype=torch.int64, device="cuda")
        key = torch.tensor([7, 0], dtype=torch.int32, device="cuda")
        ids = torch.arange(N, dtype=torch.int64, device="cuda")
        tag = 0 if name == "video" else 1
        # every launch works on scratch copies of its own: the in-place ones would otherwise run x off to infinity over the repeats
        xs, ms_, out = x.clone(), m1.clone(), torch.empty_like(x)
        launches = {
            "dpmpp_update": lambda: ops.dpmpp_update(xs, m0, ms_, tab, k, F, C, C, HW),
            "dpmpp_sde_update": lambda: ops.dpmpp_sde_update(xs, m0, ms_, tab, cz, k, F, C, C, HW, noise=z),
            "dpmpp_sde_update_ctr": lambda: ops.dpmpp_sde_update(xs, m0, ms_, tab, cz, k, F, C, C, HW, ctr=(key, ids, tag)),
            "ddpm_update": lambda: ops.ddpm_update(x, m0, z, out, tables, t, F, C, HW, 0),
            "ddpm_update_ctr": lambda: ops.ddpm_update_ctr(x, m0, key, ids, tag, out, tables, t, F, C, HW, 0),
        }
        for fn in launches.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        us = {n: [] for n in launches}
        for _ in range(repeats):
            for n, fn in launches.items():      # alternating: every repeat visits every launch
                xs.copy_(x)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    fn()
                b.record()
                b.synchronize()
                us[n].append(1000 * a.elapsed_time(b) / calls)
        res[name] = us
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, help="run one arm in this process and print its JSON line (the driver starts these)")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpm_sde_graph.txt"))
    ap.add_argument("--arm-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.arm:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("dpm_sde_bench needs a MI355X: a timing without one says nothing")
        res = loop_arm(args.arm, args.repeats) if args.arm in LOOP_ARMS else update_arm(args.repeats)
        print("RESULT " + json.dumps({"arm": args.arm, "result": res}))
        return 0
    results = {}
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
    lines = [f"tools/dpm_sde_bench.py: one call, one process per arm, {args.repeats} repeats; base model bf16, batch {BATCH}, order 2, logSNR, {NFE} evaluations"]
    fmt = lambda v: " ".join(f"{a:8.3f}" for a in v)      # noqa: E731
    extra = None
    if "update" in results:
        for name, us in results["update"].items():
            for n, v in us.items():
                lines.append(f"update      {name:6s} {n:22s} us/call {fmt(v)}")
        u = results["update"]
        extra = {n: sum(med(u[s][n + "_ctr"]) - med(u[s][n]) for s in u) for n in ("ddpm_update",)}
        extra["sde_ctr"] = sum(med(u[s]["dpmpp_sde_update_ctr"]) - med(u[s]["dpmpp_update"]) for s in u)
        extra["sde_mem"] = sum(med(u[s]["dpmpp_sde_update"]) - med(u[s]["dpmpp_update"]) for s in u)
        lines.append(f"update      summed over the two streams, medians: ddpm_update_ctr - ddpm_update {extra['ddpm_update']:.2f} us; "
                     f"dpmpp_sde_update_ctr - dpmpp_update {extra['sde_ctr']:.2f} us; dpmpp_sde_update - dpmpp_update {extra['sde_mem']:.2f} us")
    for arm in LOOP_ARMS:
        for noise, r in results.get(arm, {}).items():
            det, sde = r["ms_per_eval"]["det"], r["ms_per_eval"]["sde"]
            lines.append(f"{arm:11s} {noise:8s} sample_graph      ms/eval {fmt(det)}   finite {r['finite']['det']}")
            lines.append(f"{arm:11s} {noise:8s} sample_graph_sde  ms/eval {fmt(sde)}   finite {r['finite']['sde']}")
            d, spread = 1000 * (med(sde) - med(det)), 1000 * (max(det) - min(det))
            line = f"{arm:11s} {noise:8s} stochastic - deterministic, medians: {d:+.1f} us per evaluation; spread of the deterministic repeats {spread:.1f} us"
            if extra is not None:
                exp = extra["sde_ctr"] if noise == "counter" else extra["sde_mem"]
                line += (f"; expected about {extra['ddpm_update']:.1f} us (ddpm_update_ctr over ddpm_update) - the isolated launches differ by {exp:.1f} us"
                         + ("" if noise == "counter" else " plus two normal_() fills per evaluation on the buffer path"))
            lines.append(line)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
