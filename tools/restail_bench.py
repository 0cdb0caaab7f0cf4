#!/usr/bin/env python3
"""Micro-benchmark of mmd_res_tail (ResBlock out conv + 1x1 skip conv in one streamed launch) against the launches it replaces on
the channel-changing blocks of the base model below ds1 (video 16384 / 4096 / 1024 and audio 6400 / 1600 / 400 rows per sample, 256 /
384 / 512 channels into the out conv) and the audio ds1 block with a 512-channel skip input, bf16, batch 2 and 4.

    python tools/restail_bench.py [--reps 12] [--batches 2,4]

Arms, one process each (the parent only starts them and compares):
    two    today's launches: conv_gemm for the skip tensor, then the out conv with it as residual - gn_conv1x1 where ops.gn_fusable says
           so, gn_apply + conv_gemm otherwise (what the engine runs with MMD_TAIL_STREAM=0)
    fused  mmd_res_tail with the out-conv norm inside the launch
    pre    gn_apply, then mmd_res_tail with a null affine
An arm's launches of a shape are captured into ONE hipGraph and replayed between two HIP events, cache-cold: a 768 MB memset between
replays, outside the event pair, evicts L2 and the Infinity Cache as bench.graph_replay_ms does.  Per shape: median (min .. max) of
the repetitions of every arm, whether an arm wins by more than the slower arm's min-max spread, and whether the arms stored the same
bits (SHA-1 of Y and of the statistics records)."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))

DEEP = {"ds2": (256, (128, 384, 512, 640)), "ds4": (384, (256, 640, 768, 896)), "ds8": (512, (384, 896, 1024))}
ROWS = {"video": {"ds2": 16384, "ds4": 4096, "ds8": 1024}, "audio": {"ds2": 6400, "ds4": 1600, "ds8": 400}}
ARMS = ("two", "fused", "pre")


def shapes(batches):
    out = []
    for N in batches:
        for chain in ("video", "audio"):
            for lvl, (K1, K2s) in DEEP.items():
                out += [(f"{chain} {lvl}", ROWS[chain][lvl], K1, K2, N) for K2 in K2s]
        out.append(("audio ds1", 25600, 128, 512, N))
    return out


def run_arm(arm, reps, batches):
    import torch
    from mm_diffusion import _hip as H, ops
    BF = torch.bfloat16
    lib = H.lib()
    side = H.Stream(torch.device("cuda"))
    flush = torch.empty(768 << 20, dtype=torch.uint8, device="cuda")
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        H.call("mmd_event_create", ctypes.byref(e))
    res = []
    for name, rows, K1, K2, N in shapes(batches):
        M, COUT = N * rows, K1
        g = torch.Generator(device="cuda").manual_seed(rows + K2 + N)
        h = (torch.randn(M, K1, device="cuda", generator=g) * 1.4 + 0.3).to(BF)
        xw = torch.randn(M, K2, device="cuda", generator=g).to(BF)
        w = (torch.randn(COUT, K1, device="cuda", generator=g) * K1 ** -0.5).to(BF)
        ws = (torch.randn(COUT, K2, device="cuda", generator=g) * K2 ** -0.5).to(BF)
        b, bs = torch.randn(COUT, device="cuda", generator=g), torch.randn(COUT, device="cuda", generator=g)
        geom = ops.Geom.per_sample(N, rows)
        ga, gb = ops.gn_stats(h, torch.ones(K1, device="cuda"), torch.zeros(K1, device="cuda"), geom)
        y = torch.full((M, COUT), float("nan"), device="cuda", dtype=BF)
        sk = torch.empty(M, COUT, device="cuda", dtype=BF)
        hn = torch.empty(M, K1, device="cuda", dtype=BF)
        rec = torch.zeros(M // 64, COUT // 4, 2, device="cuda") if rows % 64 == 0 else None      # (records only on whole 64-row samples)
        plan = []
        with ops.recording(plan):
            if arm == "two":
                ops.conv_gemm(xw, ws, bs, out=sk)
                if ops.gn_fusable(geom, K1, COUT, h, rec, act=True):
                    ops.gn_conv1x1(h, ga, gb, geom, True, w, b, residual=sk, out=y, stats=rec)
                else:
                    ops.conv_gemm(ops.gn_apply(h, ga, gb, geom, act=True, out=hn), w, b, residual=sk, out=y, stats=rec)
            else:
                assert ops.res_tail_ok(h, xw, COUT, geom, rec, y)
                if arm == "fused":
                    ops.res_tail(h, ga, gb, geom, True, w, b, xw, ws, bs, out=y, stats=rec)
                else:
                    ops.res_tail(ops.gn_apply(h, ga, gb, geom, act=True, out=hn), None, None, geom, True, w, b, xw, ws, bs, out=y, stats=rec)
        st = side.torch.cuda_stream
        side.torch.wait_stream(torch.cuda.current_stream())
        for fn, args, nm, *_ in plan:                    # warm-up (function attributes) outside the capture
            assert fn(*args, st) == 0, nm
        torch.cuda.synchronize()
        with H.capture(st) as cap:
            for fn, args, nm, *_ in plan:
                assert fn(*args, st) == 0, nm
        cur = H.stream_handle()
        ts = []
        for _ in range(reps):
            flush.zero_()
            lib.mmd_event_record(ev[0], cur)
            H.call("mmd_graph_launch", cap.exec, cur)
            lib.mmd_event_record(ev[1], cur)
            torch.cuda.synchronize()
            ms = ctypes.c_float()
            H.call("mmd_event_elapsed_ms", ev[0], ev[1], ctypes.byref(ms))
            ts.append(ms.value * 1000)
        H.retire("graph", cap.exec)
        ts.sort()
        digest = hashlib.sha1(y.view(torch.int16).cpu().numpy().tobytes() + (rec.cpu().numpy().tobytes() if rec is not None else b"")).hexdigest()
        res.append(dict(shape=[name, rows, K1, K2, N], labels=[e[3][0] for e in plan], med=ts[len(ts) // 2], min=ts[0], max=ts[-1], sha1=digest))
    print("ARM " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--batches", default="2,4")
    ap.add_argument("--arm", choices=ARMS, help="(internal) run one arm in this process")
    a = ap.parse_args()
    batches = [int(v) for v in a.batches.split(",")]
    if a.arm:
        return run_arm(a.arm, a.reps, batches)
    out = {}
    for arm in ARMS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--reps", str(a.reps), "--batches", a.batches],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"arm {arm} failed ({r.returncode}):\n{r.stderr[-3000:]}")
        out[arm] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ARM ")][-1][4:])
    print(f"# {a.reps} cache-cold graph replays per arm and shape, us: median (min .. max); WIN = median gain over `two` above the slower arm's spread")
    fmt = lambda r: f"{r['med']:6.1f} ({r['min']:6.1f} .. {r['max']:6.1f})"
    for two, fu, pre in zip(out["two"], out["fused"], out["pre"]):
        name, rows, K1, K2, N = two["shape"]
        verdict = []
        for arm in (fu, pre):
            slower = two if two["med"] >= arm["med"] else arm
            gain, spread = two["med"] - arm["med"], slower["max"] - slower["min"]
            verdict.append(f"{gain:+6.1f} {'WIN ' if gain > spread else ('LOSS' if -gain > spread else 'tie ')}")
        print(f"{name} b{N}: M={N * rows:6d} K={K1}+{K2:<4d} | two[{len(two['labels'])}] {fmt(two)} | fused {fmt(fu)} {verdict[0]} | "
              f"pre {fmt(pre)} {verdict[1]} | bitwise fused {two['sha1'] == fu['sha1']} pre {two['sha1'] == pre['sha1']}", flush=True)
    print("# (audio ds1: `two` fuses its norm at 128 channels and folds its records per 32-row fragment; behind gn_apply - the `pre` arm - the fold is "
          "the two-fragment one, so the engine never runs that mode there)")


if __name__ == "__main__":
    main()
