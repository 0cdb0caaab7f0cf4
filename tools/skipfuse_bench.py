#!/usr/bin/env python3
"""Micro-benchmark of mmd_gn_conv1x1_skip (ResBlock out conv + 1x1 skip conv in one launch) against the two launches it replaces
(mmd_conv_gemm for the skip tensor, mmd_gn_conv1x1_stats with it as residual) on the ds1 shapes of the base model, bf16:
video 65536 and audio 25600 rows per sample, 128 channels into the out conv, 256 / 384 into the skip conv, batch 2 and 4.

    python tools/skipfuse_bench.py [--reps 12]

One process per arm (the parent only starts them and compares).  An arm's launches are captured into ONE hipGraph and replayed
between two HIP events, cache-cold: a 768 MB memset between replays, outside the event pair, evicts L2 and the Infinity Cache as
bench.graph_replay_ms does.  Per shape: median / min / max of the repetitions of both arms, the time ratio beside the byte ratio of
the algorithmic HBM traffic, whether the fused launch wins by more than the two-launch arm's min-max spread, and whether the two
arms stored the same bits (SHA-1 of Y and of the statistics records)."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))

SHAPES = [(name, rows, K2, N) for N in (2, 4) for name, rows in (("video", 65536), ("audio", 25600)) for K2 in (256, 384)]
K1 = COUT = 128


def run_arm(arm, reps):
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
    for name, rows, K2, N in SHAPES:
        M = N * rows
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
        rec = torch.zeros(M // 64, COUT // 4, 2, device="cuda")
        plan = []
        with ops.recording(plan):
            if arm == "two":
                ops.conv_gemm(xw, ws, bs, out=sk)
                ops.gn_conv1x1(h, ga, gb, geom, True, w, b, residual=sk, out=y, stats=rec)
            else:
                assert ops.skip_fusable(h, xw, COUT, geom, rec, y)
                ops.gn_conv1x1_skip(h, ga, gb, geom, True, w, b, xw, ws, bs, out=y, stats=rec)
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
        digest = hashlib.sha1(y.view(torch.int16).cpu().numpy().tobytes() + rec.cpu().numpy().tobytes()).hexdigest()
        res.append(dict(shape=[name, rows, K2, N], labels=[e[3][0] for e in plan], bytes=sum(e[3][2] for e in plan), med=ts[len(ts) // 2], min=ts[0],
                        max=ts[-1], sha1=digest))
    print("ARM " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--arm", choices=["two", "fused"], help="(internal) run one arm in this process")
    a = ap.parse_args()
    if a.arm:
        return run_arm(a.arm, a.reps)
    out = {}
    for arm in ("two", "fused"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--reps", str(a.reps)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"arm {arm} failed ({r.returncode}):\n{r.stderr[-3000:]}")
        out[arm] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ARM ")][-1][4:])
    print(f"# {a.reps} cache-cold graph replays per arm and shape, us: median (min .. max)")
    for two, one in zip(out["two"], out["fused"]):
        name, rows, K2, N = two["shape"]
        spread = two["max"] - two["min"]
        wins = two["med"] - one["med"] > spread
        print(f"{name} batch {N}: M={N * rows:6d} K={K1}+{K2} N={COUT} | two launches {two['med']:6.1f} ({two['min']:6.1f} .. {two['max']:6.1f}) | "
              f"fused {one['med']:6.1f} ({one['min']:6.1f} .. {one['max']:6.1f}) | time ratio {one['med'] / two['med']:.2f}, byte ratio "
              f"{one['bytes'] / two['bytes']:.2f} | gain {two['med'] - one['med']:5.1f} us vs spread {spread:4.1f} us: {'WIN' if wins else 'not shown'} | "
              f"bitwise {two['sha1'] == one['sha1']}", flush=True)


if __name__ == "__main__":
    main()
