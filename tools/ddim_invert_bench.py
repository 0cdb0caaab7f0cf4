#!/usr/bin/env python3
"""DDIM inversion: the encode loop on the graph path against its eager launches, mmd_slerp alone, and the round-trip error of the tiny
model.  One call, one fresh process per arm, every arm under its own time limit.

    python tools/ddim_invert_bench.py [--out profiles/ddim_invert.txt] [--repeats 3]

Encode arm ("encode"): the base model (bench.py's FULL configuration, bf16, batch 2, respaced to 25 levels, CounterNoise): one warm-up call
of ddim_encode_loop_progressive on each path, then `repeats` timed calls of each, ALTERNATING graph / eager (host clock around a device
synchronise after every state).  A call builds its stepper, and the graph path captures it in its first step, so the first step is
reported apart from the mean of the 23 that follow.
Slerp arm ("slerp"): mmd_slerp at the base model's latent sizes (video 16 x 3 x 64 x 64, audio 1 x 25600), batch 1 and 2, `repeats`
repeats between device events of (a) 200 calls issued from Python and (b) one replay of a torch.cuda.graph that holds 50 calls, which
leaves the host's dispatch out: microseconds per call (both launches) and, for (b), the bytes a call has to move (a and b twice, out
once) per second.
Round-trip arm ("roundtrip"): the tiny model with synthetic weights, fp32, batch 2: rel-L2 of decode(encode(x)) against x per stream at 8
and at 50 levels (clip_denoised off on both legs).  With untrained weights there is no yardstick for it; the figures are recorded, not
judged.  The same with the head convolutions zeroed (the model returns 0) checks the mechanics instead: the round trip is then
x / sqrt(alphas_cumprod[0]) - the clip is read as the level-0 state and decode step 0 divides by sqrt(alphas_cumprod[0]) - and the
figure is the rel-L2 against that.  Generation quality is not assessed."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
sys.path.insert(0, ROOT)

ARMS = ("slerp", "roundtrip", "encode")
LATENTS = {"video": 16 * 3 * 64 * 64, "audio": 1 * 25600}
TINY = dict(video_size=[8, 3, 16, 16], audio_size=[1, 512], num_channels=64, num_head_channels=32, num_res_blocks=1, channel_mult="1,2,3,4",
            resblock_updown=True)
BATCH, LEVELS = 2, 25


def med(v):
    return sorted(v)[len(v) // 2]


def _build(over, respacing, bf16):
    from mm_diffusion import logger, multimodal_script_util as msu
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    fl = msu.model_and_diffusion_defaults()
    fl.update(over)
    fl.update(use_fp16=bf16, timestep_respacing=respacing)
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.to("cuda").eval()
    return fl, model, diff


def _clips(fl, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return {"video": (torch.randn(BATCH, *fl["video_size"], generator=g) * 0.5).cuda(), "audio": (torch.randn(BATCH, *fl["audio_size"], generator=g) * 0.5).cuda()}


def encode_arm(repeats):
    import torch
    from bench import FULL
    from mm_diffusion.seeded import CounterNoise
    fl, model, diff = _build(FULL, str(LEVELS), True)
    diff.noise_source = CounterNoise(7)
    x = _clips(fl, 1)
    steps = diff.num_timesteps - 1

    def call(use_graph):
        """-> (last state, ms of the first step incl. the stepper's construction and capture, mean ms of the later steps)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        marks, out = [], None
        for out in diff.ddim_encode_loop_progressive(model, x, use_graph=use_graph):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())
        return out, 1000 * (marks[0] - t0), 1000 * (marks[-1] - marks[0]) / (len(marks) - 1)
    ref = {g: call(g)[0] for g in (True, False)}
    same = all(torch.equal(ref[True][k], ref[False][k]) for k in ("video", "audio"))
    ms = {"graph": {"first": [], "later": []}, "eager": {"first": [], "later": []}}
    for _ in range(repeats):
        for name, g in (("graph", True), ("eager", False)):
            _, first, later = call(g)
            ms[name]["first"].append(first)
            ms[name]["later"].append(later)
    return {"ms": ms, "steps": steps, "bitwise_equal": same, "finite": bool(all(torch.isfinite(v).all() for v in ref[True].values()))}


def slerp_arm(repeats, calls=200):
    import torch
    from mm_diffusion import ops
    res = {}
    for name, per in LATENTS.items():
        for N in (1, 2):
            g = torch.Generator().manual_seed(3)
            a, b = (torch.randn(N, per, generator=g).cuda() for _ in range(2))
            lam = torch.full((N,), 0.3, device="cuda")
            out, ws = torch.empty_like(a), ops.slerp_workspace(N, per, "cuda")
            for _ in range(10):
                ops.slerp(a, b, lam, out=out, ws=ws)
            torch.cuda.synchronize()
            inner = 50
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(inner):
                    ops.slerp(a, b, lam, out=out, ws=ws)
            graph.replay()
            torch.cuda.synchronize()
            us, us_graph = [], []
            for _ in range(repeats):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                for _ in range(calls):
                    ops.slerp(a, b, lam, out=out, ws=ws)
                e1.record()
                graph.replay()
                e2.record()
                e2.synchronize()
                us.append(1000 * e0.elapsed_time(e1) / calls)
                us_graph.append(1000 * e1.elapsed_time(e2) / inner)
            res[f"{name} N={N}"] = {"us_per_call": us, "us_per_call_in_graph": us_graph, "bytes": 20 * N * per,
                                    "workgroups_per_launch": N * (ws.numel() // (3 * N))}
    return res


def roundtrip_arm():
    import torch
    from mm_diffusion.seeded import CounterNoise
    res = {}
    for levels in (8, 50):
        fl, model, diff = _build(TINY, str(levels), False)
        diff.noise_source = CounterNoise(7)
        x = _clips(fl, 2)
        lat = diff.ddim_encode_loop(model, x)
        back = diff.ddim_decode_loop(model, lat, clip_denoised=False)
        res[str(levels)] = {k: float((back[k] - x[k]).double().norm() / x[k].double().norm()) for k in ("video", "audio")}
        res[str(levels)]["finite"] = bool(all(torch.isfinite(v).all() for v in back.values()))
        res[str(levels)]["latent_rms"] = {k: float(lat[k].double().pow(2).mean().sqrt()) for k in ("video", "audio")}
        for name, p in model.named_parameters():          # the model returns exactly 0: the loops' own arithmetic is what is left
            if name.startswith(("video_out.2.", "audio_out.2.")):
                p.data.zero_()
        model.load_state_dict(model.state_dict())         # (repacks the weights the engines hold)
        back = diff.ddim_decode_loop(model, diff.ddim_encode_loop(model, x), clip_denoised=False)
        s0 = float(diff.alphas_cumprod[0]) ** 0.5
        res[str(levels)]["zero_head"] = {k: float((back[k].double() - x[k].double() / s0).norm() / (x[k].double() / s0).norm()) for k in ("video", "audio")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, help="run one arm in this process and print its JSON line (the driver starts these)")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddim_invert.txt"))
    ap.add_argument("--arm-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.arm:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("ddim_invert_bench needs a MI355X: a timing without one says nothing")
        with torch.no_grad():
            res = {"encode": lambda: encode_arm(args.repeats), "slerp": lambda: slerp_arm(args.repeats), "roundtrip": roundtrip_arm}[args.arm]()
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
    lines = [f"tools/ddim_invert_bench.py: one call, one process per arm, {args.repeats} repeats"]
    fmt = lambda v: " ".join(f"{a:8.3f}" for a in v)      # noqa: E731
    for name, r in results.get("slerp", {}).items():
        u = med(r["us_per_call_in_graph"])
        lines.append(f"slerp       {name:12s} us/call from Python {fmt(r['us_per_call'])}   inside a graph of 50 {fmt(r['us_per_call_in_graph'])}   "
                     f"{r['workgroups_per_launch']:4d} workgroups per launch, {r['bytes'] / 1e6:.2f} MB per call -> {r['bytes'] / u / 1e3:.1f} GB/s "
                     "at the in-graph median (two launches)")
    for levels, r in results.get("roundtrip", {}).items():
        lines.append(f"roundtrip   tiny model, synthetic weights, fp32, {int(levels):3d} levels: rel-L2 of decode(encode(x)) - x: video {r['video']:.3e} "
                     f"audio {r['audio']:.3e}   finite {r['finite']}   latent rms video {r['latent_rms']['video']:.3f} audio {r['latent_rms']['audio']:.3f}"
                     "   (recorded, not judged: untrained weights)")
        lines.append(f"roundtrip   the same with the head convolutions zeroed, {int(levels):3d} levels: rel-L2 against x / sqrt(alphas_cumprod[0]): video "
                     f"{r['zero_head']['video']:.3e} audio {r['zero_head']['audio']:.3e}")
    if "encode" in results:
        r = results["encode"]
        g, e = r["ms"]["graph"], r["ms"]["eager"]
        lines.append(f"encode      base model bf16, batch {BATCH}, {LEVELS} levels, {r['steps']} steps per call: graph and eager bitwise equal {r['bitwise_equal']}, "
                     f"finite {r['finite']}")
        for name, v in (("graph", g), ("eager", e)):
            lines.append(f"encode      {name}  first step (stepper" + (" + capture" if name == "graph" else "") + f") ms {fmt(v['first'])}   later steps ms/step {fmt(v['later'])}")
        lines.append(f"encode      later steps, eager / graph at the medians: {med(e['later']) / med(g['later']):.2f}; the graph path's first step costs "
                     f"{(med(g['first']) - med(e['first'])) / med(g['later']):.1f} replayed steps more than the eager one's")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
