#!/usr/bin/env python3
"""Isolated times of the bf16 MFMA attention backward pair (mmd_attn_bwd_mfma: dQ kernel + dK/dV kernel) on self-attention shapes,
HIP events on the launch stream, warm, average of --reps back-to-back calls.

    python tools/attn_bwd_bench.py [--batch 6] [--reps 20]

Default shapes: the SR U-Net's attentions (4 heads of width 192 on 64 / 256 tokens, 4 heads of width 96 on 1024 tokens) and, as context,
the existing width-128 instance at the same token count and head count.  For the split of the pair into its two kernels run the same
command under `rocprofv3 --kernel-trace --stats`."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
import torch  # noqa: E402
from mm_diffusion import _hip as H, ops  # noqa: E402

SHAPES = [("sr ds32 T=64", 64, 4, 192), ("sr ds16 T=256", 256, 4, 192), ("context T=256", 256, 4, 128), ("context T=64", 64, 4, 128),
          ("sr ds8 T=1024", 1024, 4, 96)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        H.call("mmd_event_create", ctypes.byref(e))
    st = H.stream_handle()
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, T, heads, ch in SHAPES:
        C, rows = heads * ch, a.batch * T
        qkv = torch.randn(rows, 3 * C, device="cuda", generator=g).to(torch.bfloat16)
        do = torch.randn(rows, C, device="cuda", generator=g).to(torch.bfloat16)
        out = torch.empty(rows, C, device="cuda", dtype=torch.bfloat16)
        lse = torch.empty(rows * heads, device="cuda", dtype=torch.float32)
        dqkv = torch.empty_like(qkv)
        ops.attn_lse(qkv, qkv, out, lse, heads, ch, a.batch, 1, T, T, T, T, 1)
        run = lambda: ops.attn_bwd_mfma(qkv, qkv, out, do, dqkv, 0, dqkv, C, 2 * C, lse, heads, ch, a.batch, 1, T, T, T, T, 1)   # noqa: E731
        for _ in range(3):
            run()
        H.call("mmd_event_record", ev[0], st)
        for _ in range(a.reps):
            run()
        H.call("mmd_event_record", ev[1], st)
        torch.cuda.synchronize()
        ms = ctypes.c_float()
        H.call("mmd_event_elapsed_ms", ev[0], ev[1], ctypes.byref(ms))
        us = ms.value / a.reps * 1e3
        flops = 10.0 * a.batch * T * T * C          # S, dP, dV, dK, dQ: five T x T x ch products per head
        print(f"{name:16s} batch {a.batch} heads {heads} width {ch:3d}: {us:8.1f} us per backward pair, {flops / us / 1e6:6.1f} TFLOP/s algorithmic")
    for e in ev:
        H.lib().mmd_event_destroy(e)


if __name__ == "__main__":
    main()
