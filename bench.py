#!/usr/bin/env python3
"""Benchmark of the MI355X-native MM-Diffusion denoising hot path.

    python bench.py --gpus N --steps K --warmup W
    (N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...)

One "step" = one DDPM p_sample (coupled U-Net forward + fused ancestral update of both streams) of the per-GPU
batch, replayed from one captured hipGraph.  Workload = BASELINE.json configs[1]: Landscape base model
(133.68 M params), 250-step respacing, batch 4 per GPU, 16x3x64x64 video + 1x25600 audio, bf16 activations /
GEMM operands with fp32 statistics and accumulation, synthetic inputs and key-seeded synthetic weights.
Batch shards over ranks with NO data-path collective (independent trajectories) -> weak scaling.

Prints ONE JSON line (rank 0).  `value` = video+audio pair denoising steps per second, whole job
(= steps/s x global batch); `ms_per_step` = milliseconds of one timed step (--steps of them are timed; --mode dpm / sr:
one step = one whole sampling call, `ms_per_eval` = per network evaluation).

A plain run sets up, warms up, times the steps and prints the line.  --full adds the side measurements:
`roofline` = the dominant kernel (bf16 implicit-GEMM conv) timed live with HIP events on the launch stream, the
per-kernel breakdown and the graded kernels; `cpu_baseline` = the oracle (CPU restatement, kind "port") timed on
the host cores (--mode train: the conv weight-gradient roofline).

--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (float32, 64 MB at most; an array
that does not fit is replaced by a fixed seeded sample of its elements).  Inputs, weights and noise are seeded, so
two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "mm-diffusion_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FULL = dict(video_size=[16, 3, 64, 64], audio_size=[1, 25600], num_channels=128, num_head_channels=64,
            num_res_blocks=2, resblock_updown=True)
MFMA_BF16_PEAK_TFLOPS = 2500.0     # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F32_PEAK_TFLOPS = 157.3
HBM_PEAK_GBS = 8000.0
MODEL_FLOPS_PER_PAIR = 1328.8e9    # conv 1133.0 G + attention matmuls 195.8 G
DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: every tensor of `arrays` as <path>/<name>.npy in float32, in order.  One that does not fit in what is left of
    the 64 MB budget is replaced by a fixed sample of its flattened elements (positions drawn from a CPU generator seeded with 0,
    sorted), as many as fit."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    left = DUMP_BUDGET_BYTES
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() * 4 > left:
            idx = torch.randint(t.numel(), (left // 4 // len(arrays),), generator=torch.Generator().manual_seed(0)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        a = t.float().cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), a)
        left -= a.nbytes


def build(dtype_flag, respacing, batch, device):
    from mm_diffusion import logger, multimodal_script_util as msu
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    fl = msu.model_and_diffusion_defaults()
    fl.update(FULL)
    fl.update(use_fp16=(dtype_flag == "bf16"), timestep_respacing=respacing)
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.to(device).eval()
    return fl, model, diff


def kernel_breakdown(stepper, reps=3, detail=False, by_tag=False):
    """Per-kernel time of one step measured with HIP events on the launch stream (eager replay of the plan)."""
    from mm_diffusion import _hip as H
    import ctypes
    lib = H.lib()
    stream = H.stream_handle()
    plan = [e for e in (stepper.eng.plan_f32 if stepper.use_f32 else stepper.eng.plan) + stepper.update_plan if e[0] is not None]
    evs = []
    for _ in range(len(plan) + 1):
        e = ctypes.c_void_p()
        H.call("mmd_event_create", ctypes.byref(e))
        evs.append(e)
    agg = {}
    for rep in range(reps):
        torch.cuda.synchronize()
        lib.mmd_event_record(evs[0], stream)
        for i, (fn, args, name, meta, _sid, _tag) in enumerate(plan):
            rc = fn(*args, stream)
            assert rc == 0, name
            lib.mmd_event_record(evs[i + 1], stream)
        torch.cuda.synchronize()
        ms = ctypes.c_float()
        for i, (fn, args, name, meta, _sid, _tag) in enumerate(plan):
            H.call("mmd_event_elapsed_ms", evs[i], evs[i + 1], ctypes.byref(ms))
            label, flops, nbytes = meta
            if by_tag:
                if not _tag:
                    continue
                a = agg.setdefault(_tag, dict(ms=0.0, calls=0, flops=0, bytes=0, attn_ms=0.0, attn_flops=0))
                a["ms"] += ms.value
                a["calls"] += 1
                a["flops"] += flops
                a["bytes"] += nbytes
                if label.startswith("attn_fwd"):
                    a["attn_ms"] += ms.value
                    a["attn_flops"] += flops
                continue
            if not detail:
                label = label.split("[")[0]
            else:
                label += "@a" if _sid == 1 else "@v"
            a = agg.setdefault(label, dict(ms=0.0, calls=0, flops=0, bytes=0))
            a["ms"] += ms.value
            a["calls"] += 1
            a["flops"] += flops
            a["bytes"] += nbytes
    for e in evs:
        lib.mmd_event_destroy(e)
    for a in agg.values():
        for k in a:
            a[k] /= reps
    return agg


def graph_replay_ms(stepper, entries, reps=12, flush_bytes=768 << 20):
    """GPU time of a run of plan launches replayed as ONE hipGraph between two HIP events on the launch stream, cache-cold: the eager
    replay of kernel_breakdown() is paced by the Python host for launches shorter than ~10 us (two ctypes calls per launch), a graph is
    not; a 768 MB memset between replays (outside the event pair) evicts L2 and the 256 MB Infinity Cache, so the tensors come from HBM
    as they do inside the step.  Returns (median ms, min ms)."""
    import ctypes
    from mm_diffusion import _hip as H
    lib = H.lib()
    side = stepper.eng.side
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    for fn, args, name, *_ in entries:                 # warm-up on the capture stream (function attributes)
        assert fn(*args, side.cuda_stream) == 0, name
    torch.cuda.synchronize()
    with H.capture(side.cuda_stream) as cap:
        for fn, args, name, *_ in entries:
            assert fn(*args, side.cuda_stream) == 0, name
    flush = torch.empty(flush_bytes, dtype=torch.uint8, device="cuda")
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        H.call("mmd_event_create", ctypes.byref(e))
    st = H.stream_handle()
    out = []
    for _ in range(reps):
        flush.zero_()
        lib.mmd_event_record(ev[0], st)
        H.call("mmd_graph_launch", cap.exec, st)
        lib.mmd_event_record(ev[1], st)
        torch.cuda.synchronize()
        ms = ctypes.c_float()
        H.call("mmd_event_elapsed_ms", ev[0], ev[1], ctypes.byref(ms))
        out.append(ms.value)
    for e in ev:
        lib.mmd_event_destroy(e)
    H.retire("graph", cap.exec)
    out.sort()
    return out[len(out) // 2], out[0]


def build_id():
    """Hash of the kernel sources + launch-plan code: ties a profiles/pmc_traffic.json to the build it was measured on."""
    import hashlib
    h = hashlib.sha1()
    base = os.path.join(ROOT, "mm-diffusion_amd")
    files = sorted(os.path.join(base, "csrc", f) for f in os.listdir(os.path.join(base, "csrc")) if f.endswith((".hip", ".h")))
    files += [os.path.join(base, "mm_diffusion", f) for f in ("engine.py", "ops.py", "sampler.py")]
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def cpu_baseline(fl, seconds_budget=30.0):
    """The oracle (oracle/*.py, CPU restatement of the reference path, kind "port") on the host cores, BASELINE.md section 3's protocol:
    fp32, x_T from CPU seed 0, `timestep_respacing="2"`, ONE warm-up p_sample step, then the TWO timed steps of the 2-step loop
    (timesteps [999, 0]) at batch 1; then, while the ~30 s budget lasts, one timed step at batch 4 (SURVEY 8d asks for N = 1 and N = 4;
    two would take 30 s on their own).  Threads: BASELINE.md says os.cpu_count(), which on the GPU box is 256 - torch's CPU kernels
    oversubscribe badly on this model (256 threads: 688 s per step; 64: 6.1 s; 16: ~2.5 s), so the warm-up step is run on 16 and on
    32 threads and the faster setting does the timed steps (`threads_tried`, `cores` = the threads actually used)."""
    from oracle import diffusion_ref as dref, unet_ref as uref
    from mm_diffusion.synth import synth_tensor
    from mm_diffusion import multimodal_script_util as msu
    import random
    ncpu = os.cpu_count() or 1
    model, _ = msu.create_model_and_diffusion(**{**fl, "use_fp16": False})
    sd = {k: synth_tensor(k, v.shape) for k, v in model.state_dict().items()}
    del model
    om = uref.OracleModel(sd, fl)
    S = dref.Schedule(respacing="2")
    torch.manual_seed(0)
    random.seed(0)
    t_all = time.perf_counter()
    x1 = {"video": torch.randn(1, *fl["video_size"]), "audio": torch.randn(1, *fl["audio_size"])}
    tried = {}
    for th_ in (16, 32):                                        # warm-up steps double as the thread probe (the first also warms the allocator,
        if th_ > ncpu and tried:                                # the thread pool and the oneDNN primitive caches: it is the slower of its kind)
            continue
        torch.set_num_threads(min(th_, ncpu))
        if not tried:
            dref.p_sample(S, om, x1, torch.tensor([1]))         # the untimed warm-up step
        t0 = time.perf_counter()
        dref.p_sample(S, om, x1, torch.tensor([1]))
        tried[min(th_, ncpu)] = round(time.perf_counter() - t0, 3)
    cores = min(tried, key=tried.get)
    torch.set_num_threads(cores)
    t0 = time.perf_counter()                                    # the two timed steps of the 2-step loop
    x = dref.p_sample(S, om, x1, torch.tensor([1]))
    x = dref.p_sample(S, om, x, torch.tensor([0]))
    out = {1: (time.perf_counter() - t0) / 2}
    if time.perf_counter() - t_all < seconds_budget:            # bounded sample: one more timed step, at batch 4
        x = {"video": torch.randn(4, *fl["video_size"]), "audio": torch.randn(4, *fl["audio_size"])}
        t0 = time.perf_counter()
        x = dref.p_sample(S, om, x, torch.tensor([0] * 4))
        out[4] = time.perf_counter() - t0
    best_b = max(out, key=lambda b: b / out[b])
    return {"value": best_b / out[best_b], "unit": "pair-steps/s", "cores": cores, "kind": "port", "threads_tried": tried,
            "pair_steps_per_s_batch1": 1 / out[1], "pair_steps_per_s_batch4": (4 / out[4]) if 4 in out else None,
            "sample": f"1 warm-up + the 2 timed p_sample steps of the 2-step loop at batch 1 ({out[1]:.1f} s per step)" +
                      (f" and one timed step at batch 4 ({out[4]:.1f} s)" if 4 in out else "") +
                      f" of the Landscape base model, fp32, oracle/unet_ref.py on {cores} host threads (of {ncpu}; probed 16 / 32: more threads are slower); value = the better batch"}


def wgrad_roofline(B, device):
    """The training step's dominant kernel family - the conv weight gradients (their share of the step's kernel time comes from the
    tracked rocprofv3 trace of this command, profiles/kernel_stats_train.json / r04_train_step_kernel_stats.txt) - measured live with HIP events on the launch stream, on the video 3x3 / k=3 / 1x1 layer shapes of the step at this
    batch size: algorithmic flops (2 M Cout Cin taps) / average launch time against the dense bf16 MFMA peak."""
    import ctypes
    from mm_diffusion import _hip as H, ops
    F, HW = 16, 64
    shapes = [("3x3 ds1 128->128", B * F * HW * HW, 128, 128, ops.TAPS_SPATIAL, (B * F, HW, HW)), ("k3t ds1 128->128", B * F * HW * HW, 128, 128, ops.TAPS_TEMPORAL, (F, HW * HW, 1)),
              ("1x1 ds1 128->128", B * F * HW * HW, 128, 128, ops.TAPS_1, (1, 1, 1)), ("3x3 ds2 256->256", B * F * HW * HW // 4, 256, 256, ops.TAPS_SPATIAL, (B * F, HW // 2, HW // 2)),
              ("3x3 ds4 384->384", B * F * HW * HW // 16, 384, 384, ops.TAPS_SPATIAL, (B * F, HW // 4, HW // 4)), ("3x3 ds8 512->512", B * F * HW * HW // 64, 512, 512, ops.TAPS_SPATIAL, (B * F, HW // 8, HW // 8))]
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        H.call("mmd_event_create", ctypes.byref(e))
    st = H.stream_handle()
    per, flops, us = {}, 0.0, 0.0
    g = torch.Generator(device=device).manual_seed(0)
    for name, M, Cin, Cout, taps, dims in shapes:
        x = torch.randn(M, Cin, device=device, generator=g).to(torch.bfloat16)
        dy = torch.randn(M, Cout, device=device, generator=g).to(torch.bfloat16)
        dW, db = torch.zeros(Cout, Cin * len(taps), device=device), torch.zeros(Cout, device=device)
        ops.conv_wgrad(dy, x, dW, db, taps, dims)
        H.call("mmd_event_record", ev[0], st)
        for _ in range(3):
            ops.conv_wgrad(dy, x, dW, db, taps, dims)
        H.call("mmd_event_record", ev[1], st)
        torch.cuda.synchronize()
        ms = ctypes.c_float()
        H.call("mmd_event_elapsed_ms", ev[0], ev[1], ctypes.byref(ms))
        t = ms.value / 3 * 1e3
        fl = 2.0 * M * Cout * Cin * len(taps)
        per[name] = {"us": round(t, 1), "TFLOPs": round(fl / t / 1e6, 1)}
        flops += fl
        us += t
        del x, dy, dW, db
    for e in ev:
        H.lib().mmd_event_destroy(e)
    ach = flops / us / 1e6
    # how much of the step's kernel time the family is: from the rocprofv3 kernel trace of this command (profiles/kernel_stats_train.json,
    # tools/round_profile.sh), when that profile was taken on THIS build
    share = share_note = None
    try:
        with open(os.path.join(ROOT, "profiles", "kernel_stats_train.json")) as f:
            ks = json.load(f)
        if ks.get("build_id") == build_id():
            tot = sum(v["total_us"] for v in ks["kernels"].values())
            share = sum(v["total_us"] for k, v in ks["kernels"].items() if "wgrad" in k or "colsum" in k) / max(tot, 1e-9)
            share_note = f"profiles/kernel_stats_train.json ({ks.get('command')})"
        else:
            share_note = f"profiles/kernel_stats_train.json is from build {ks.get('build_id')}, this is {build_id()}: not used"
    except Exception:
        pass
    return {"kernel": "conv_wgrad (wgrad_tr_bf16 / wgrad128_bf16 + colsum)", "bound": "mfma", "achieved": ach, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": ach / MFMA_BF16_PEAK_TFLOPS, "traffic": None, "per_shape": per, "share_of_step_kernel_time": share, "share_source": share_note,
            "note": "launch-weighted over six layer shapes of the step at this batch size, HIP events on the launch stream"}


def train_bench(args, world, rank, device):
    """BASELINE configs[3]: multimodal_training_losses step (forward + backward + flat AdamW/EMA, gradient all-reduce when
    world > 1) of the AIST++/Landscape base model, per-GPU batch --batch, bf16 activations, dropout 0.1, t ~ U{0..999}."""
    import random
    import torch.distributed as dist
    from mm_diffusion import logger, multimodal_script_util as msu
    from mm_diffusion.optim import FlatAdamW
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    fl = msu.model_and_diffusion_defaults()
    fl.update(FULL)
    fl.update(use_fp16=(args.dtype == "bf16"), dropout=0.1)
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.to(device).train()
    opt = FlatAdamW(model.parameters(), lr=1e-4, weight_decay=0.0, ema_rates=[0.9999], pack_dtype=model.dtype)
    g = torch.Generator().manual_seed(4321 + rank)
    random.seed(4321 + rank)
    torch.manual_seed(4321 + rank)
    B = args.batch
    x0 = {"video": (torch.rand(B, *fl["video_size"], generator=g) * 2 - 1).to(device),
          "audio": (torch.rand(B, *fl["audio_size"], generator=g) * 2 - 1).to(device)}

    gstep = None
    if not args.no_graph:         # forward + backward replayed from one captured graph (mm_diffusion/train_graph.py)
        from mm_diffusion.train_graph import GraphedTrainStep
        gstep = GraphedTrainStep(model, diff, opt, x0)

    last = {}                     # the loss terms of the latest step (--dump-outputs)

    def one_step():
        t = torch.randint(0, diff.num_timesteps, (B,), generator=g).to(device)
        if gstep is not None:
            last["terms"] = gstep.step(x0, t)
            return last["terms"]["loss"].mean()
        opt.zero_grad()
        last["terms"] = diff.multimodal_training_losses(model, x0, t)
        loss = last["terms"]["loss"].mean()
        opt.arm_overlap()             # world > 1: gradient buckets are all-reduced on a side stream while the backward is still running
        loss.backward()
        opt.all_reduce_grads()
        opt.step()
        return loss

    for _ in range(args.warmup):
        one_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = one_step()
    host_elapsed = time.perf_counter() - t0          # launch-side time (python + HIP enqueue) before the final drain
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"loss": last["terms"]["loss"], "params": opt.flat})
    roof = None
    if rank == 0 and args.full and not args.no_breakdown:
        roof = wgrad_roofline(B, device)
    if rank == 0:
        print(json.dumps({
            "metric": "training steps/sec (multimodal_training_losses fwd+bwd+AdamW, video+audio pairs)", "value": args.steps * B * world / elapsed,
            "unit": "pair-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic", "ranks_seen": args.ranks_seen,
            "config": {"workload": f"BASELINE configs[3]: base model training step, per-GPU batch {B}, dropout 0.1, flat-buffer gradient all-reduce, "
                                   f"{'eager' if gstep is None else 'graph-captured forward+backward'}",
                       "global_batch": B * world, "loss": float(loss), "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9},
            "host_ms_per_step": 1000 * host_elapsed / args.steps, "roofline": roof,
            "model_tflops": 3 * MODEL_FLOPS_PER_PAIR * B * args.steps / elapsed / 1e12}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def dpm_bench(args, world, rank, device):
    """BASELINE configs[4], base-model half: DPM-Solver++ (predict_x0 + dynamic thresholding), multistep order 2, 50 network
    evaluations per sample batch (the script's literal 'adaptive' method has a data-dependent NFE, so NFE is fixed here as
    SURVEY 8d prescribes), per-GPU batch --batch.  A "step" is one network evaluation + its solver update."""
    import random
    import torch.distributed as dist
    from mm_diffusion import logger, multimodal_script_util as msu
    from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    fl = msu.model_and_diffusion_defaults()
    fl.update(FULL)
    fl.update(use_fp16=(args.dtype == "bf16"))
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.to(device).eval()
    random.seed(99 + rank)
    torch.manual_seed(99 + rank)
    B, NFE = args.batch, 50
    solver = DPM_Solver(model=model, alphas_cumprod=torch.tensor(diff.alphas_cumprod, dtype=torch.float32), predict_x0=True, thresholding=True)

    def one_sample():
        x_T = {"video": torch.randn(B, *fl["video_size"], device=device), "audio": torch.randn(B, *fl["audio_size"], device=device)}
        return solver.sample(x_T, steps=NFE, order=2, skip_type="logSNR", method="multistep")

    for _ in range(max(1, args.warmup)):
        one_sample()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = one_sample()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"video": out["video"], "audio": out["audio"]})
    if rank == 0:
        evals = args.steps * NFE
        print(json.dumps({
            "metric": "denoising steps/sec (video+audio pair), DPM-Solver++ multistep-2, 50 NFE", "value": evals * B * world / elapsed,
            "unit": "pair-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000 * elapsed / args.steps,
            "ms_per_eval": 1000 * elapsed / evals,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic", "ranks_seen": args.ranks_seen,
            "config": {"workload": f"BASELINE configs[4] (base-model half): DPM-Solver++ 50 NFE, per-GPU batch {B}; one timed step = one full "
                                   f"{NFE}-evaluation sample() call", "global_batch": B * world, "seconds_per_sample_batch": elapsed / args.steps,
                       "finite": bool(torch.isfinite(out["video"]).all())}}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def sr_bench(args, world, rank, device):
    """BASELINE configs[4], SR half: the shipped 64 -> 256 super-resolution U-Net (192 channels, mult (1,1,2,2,4,4), attention at
    ds 8/16/32, learned sigma; ssh_scripts/multimodal_sample_sr.sh:10-13,20) sampled with DDIM-25 on the 16 frames of --batch clips
    (N = 16 * batch images of 256 x 256), start noise repeated over the frames of a clip like multimodal_sample_sr.py:191-196."""
    import torch.distributed as dist
    from mm_diffusion import logger, script_util as su
    from mm_diffusion.synth import synth_init_
    logger.set_quiet(True)
    d = su.image_sr_model_and_diffusion_defaults()
    d.update(large_size=256, small_size=64, sr_num_channels=192, sr_num_heads=4, sr_num_res_blocks=2, sr_attention_resolutions="8,16,32",
             sr_resblock_updown=True, sr_use_scale_shift_norm=True, sr_learn_sigma=True, use_fp16=(args.dtype == "bf16"),
             sr_timestep_respacing="ddim25")
    model, diff = su.image_sr_create_model_and_diffusion(**d)
    synth_init_(model)
    model.to(device).eval()
    torch.manual_seed(7 + rank)
    B, Fr = args.batch, 16
    low = (torch.rand(B * Fr, 3, 64, 64) * 2 - 1).to(device)

    def one_clip_batch():
        noise = torch.randn(B, 3, 256, 256, device=device).repeat_interleave(Fr, dim=0)
        return diff.ddim_sample_loop(model, (B * Fr, 3, 256, 256), clip_denoised=True, model_kwargs={"low_res": low}, noise=noise, device=device)

    for _ in range(max(1, args.warmup)):
        one_clip_batch()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = one_clip_batch()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"frames": out})
    if rank == 0:
        evals = args.steps * diff.num_timesteps
        print(json.dumps({
            "metric": "SR denoising steps/sec (256x256 frames), DDIM-25", "value": evals * B * Fr * world / elapsed, "unit": "frame-steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000 * elapsed / args.steps,
            "ms_per_eval": 1000 * elapsed / evals, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic", "ranks_seen": args.ranks_seen,
            "config": {"workload": f"BASELINE configs[4] (SR half): ImageSuperResModel 64->256, {B} clip(s) x 16 frames per GPU, DDIM-25; one timed step "
                                   "= one full 25-evaluation ddim_sample_loop", "global_batch": B * world, "seconds_per_clip_batch": elapsed / args.steps,
                       "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9, "finite": bool(torch.isfinite(out).all())}}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-exec this command line as N ranks of one node through
    torch.distributed.run (one process per GPU, 127.0.0.1 rendezvous on a free port; the reference's launch model is
    `mpiexec -n N python ...`, ssh_scripts/multimodal_sample_sr.sh:16-28).  Rank 0's JSON line is this process's stdout.
    With fewer visible GPUs than ranks the ranks share devices over gloo (RCCL refuses duplicate devices): a functional
    smoke run of the multi-rank path, flagged in the JSON line (`backend`)."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if torch.cuda.is_available() and torch.cuda.device_count() < n:
        env.setdefault("MMD_DIST_BACKEND", "gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4, help="per-GPU batch (BASELINE configs[1]: 4)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--respacing", default="250")
    ap.add_argument("--mode", default="sample", choices=["sample", "train", "dpm", "sr"],
                    help="sample = headline DDPM step (default); train = configs[3]; dpm = configs[4] base-model half (DPM-Solver++ 50 NFE); sr = configs[4] SR half (DDIM-25 on 256x256 frames)")
    ap.add_argument("--full", action="store_true",
                    help="also the side measurements after the timed steps: per-kernel breakdown, roofline and graded kernels (sample mode), "
                         "the CPU baseline (sample mode, one rank), the conv weight-gradient roofline (train mode)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--no-graph", action="store_true", help="eager launches from the host instead of the captured hipGraph (train mode; sample mode: an A/B switch)")
    ap.add_argument("--no-breakdown", action="store_true", help="with --full: leave out the breakdown / roofline")
    ap.add_argument("--lanes", type=int, default=0, help="batch lanes of the sampling step (0 = the sampler's default; sampler.GraphStepper)")
    ap.add_argument("--breakdown-out", default="", help="with --full: file for the per-launch-shape HIP-event breakdown (sample mode)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all; rank 0)")
    ap.add_argument("--as-rank", type=int, default=0,
                    help="single-process run with the seeds of rank R of a multi-rank job (tests: rank r's trajectory is that of a lone process seeded 1234 + r)")
    ap.add_argument("--dump-final", default="", help="directory: every rank saves its final sample as rank<r>.pt (sample mode)")
    ap.add_argument("--launch-check", action="store_true",
                    help="only bring the ranks up, all-reduce a one per rank and print {n_gpus, ranks_seen, backend}: the self-launch / rendezvous "
                         "path without any GPU work (CPU test of `python bench.py --gpus N`)")
    args = ap.parse_args()
    if args.breakdown_out and not args.full:
        ap.error("--breakdown-out is part of the breakdown: it needs --full")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args.gpus)          # plain `python bench.py --gpus N`: spawn the N ranks ourselves
    import torch.distributed as dist
    from mm_diffusion import dist_util
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist_util.setup_dist()
    rank = dist_util.rank()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}")
    ranks_seen = 1
    if world > 1:          # the collective backend really spans `world` ranks: all-reduce of ones (goes into the JSON line)
        ones = torch.ones(1, device=dist_util.dev() if torch.cuda.is_available() else "cpu")
        dist.all_reduce(ones)
        ranks_seen = int(ones.item())
    args.ranks_seen, args.backend = ranks_seen, (dist.get_backend() if world > 1 else None)
    if args.launch_check:
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": world, "ranks_seen": ranks_seen, "backend": args.backend}))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a MI355X (no CPU fallback for the product path)")
    device = dist_util.dev()
    if args.mode == "dpm":
        return dpm_bench(args, world, rank, device)
    if args.mode == "sr":
        return sr_bench(args, world, rank, device)
    if args.mode == "train":
        return train_bench(args, world, rank, device)

    fl, model, diff = build(args.dtype, args.respacing, args.batch, device)
    from mm_diffusion.sampler import GraphStepper
    import random
    seed_rank = rank if world > 1 else args.as_rank
    random.seed(1234 + seed_rank)
    torch.manual_seed(1234 + seed_rank)
    stepper = GraphStepper(diff, model, args.batch, device, clip_denoised=True, lanes=args.lanes or None, use_graph=not args.no_graph)
    stepper.load(torch.randn(args.batch, *fl["video_size"]).to(device), torch.randn(args.batch, *fl["audio_size"]).to(device))
    T = diff.num_timesteps
    idx = T - 1

    def one_step():
        nonlocal idx
        stepper.step(idx)
        idx = idx - 1 if idx > 0 else T - 1

    for _ in range(args.warmup):
        one_step()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    cur = stepper.current()
    finite = bool(torch.isfinite(cur["video"]).all() and torch.isfinite(cur["audio"]).all())
    if args.dump_final:
        os.makedirs(args.dump_final, exist_ok=True)
        torch.save({k: v.cpu() for k, v in cur.items()}, os.path.join(args.dump_final, f"rank{seed_rank}.pt"))
    gather_ms = None
    if world > 1:          # the ONE collective of batch-sharded sampling: the terminal all-gather of the samples (mtu:424-431), timed apart
        fence()
        tg = time.perf_counter()
        gv, ga = dist_util.all_gather_samples(cur["video"]), dist_util.all_gather_samples(cur["audio"])
        fence()
        gather_ms = 1000.0 * (time.perf_counter() - tg)
        assert gv.shape[0] == args.batch * world and ga.shape[0] == args.batch * world
    if args.dump_outputs:  # before anything replays the plan again: x_{t-1} of both streams and the U-Net's prediction of the last step
        outs = {"video": cur["video"], "audio": cur["audio"],
                "eps_video": torch.cat([e.out_video for e in stepper.engs]), "eps_audio": torch.cat([e.out_audio for e in stepper.engs])}
        outs = {k: dist_util.all_gather_samples(v) for k, v in outs.items()}       # whole job (identity on one rank)
        if rank == 0:
            dump_outputs(args.dump_outputs, outs)

    global_batch = args.batch * world
    steps_per_s = args.steps / elapsed
    res = {
        "metric": "denoising steps/sec (video+audio pair), 16x64x64 / 25600",
        "value": steps_per_s * global_batch, "unit": "pair-steps/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1000.0 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: Landscape base model (133.68M params), DDPM p_sample, "
                               f"timestep_respacing={args.respacing}, per-GPU batch {args.batch}, 16x3x64x64 video + 1x25600 audio",
                   "global_batch": global_batch, "batch_steps_per_s": steps_per_s, "parallelism": f"batch-sharded x{world}, no in-loop collective",
                   "weights": "key-seeded synthetic (mm_diffusion.synth)", "graph_replay": not args.no_graph, "batch_lanes": stepper.lanes, "finite": finite, "terminal_all_gather_ms": gather_ms,
                   "ranks_seen": args.ranks_seen, "backend": args.backend},
        "model_tflops": steps_per_s * args.batch * MODEL_FLOPS_PER_PAIR / 1e12,
    }
    timed_lanes = stepper.lanes
    if rank == 0 and args.full and not args.no_breakdown:
        if stepper.lanes > 1:      # per-kernel accounting on the unsplit batch-N plan (the shapes BASELINE.md grades), one stream, in order
            stepper = GraphStepper(diff, model, args.batch, device, clip_denoised=True, lanes=1)
        agg = kernel_breakdown(stepper)
        total_ms = sum(a["ms"] for a in agg.values())
        dom = max(agg, key=lambda k: agg[k]["ms"])
        a = agg[dom]
        peak = MFMA_BF16_PEAK_TFLOPS if args.dtype == "bf16" else MFMA_F32_PEAK_TFLOPS
        ach = a["flops"] / (a["ms"] * 1e-3) / 1e12
        traffic = traffic_note = None
        try:       # HBM bytes per launch from the rocprofv3 PMC passes of this same command (profiles/, separate --pmc runs,
            #        tools/round_profile.sh); only accepted when it was measured on THIS build of the kernels + launch plan
            with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
                pt = json.load(f)
            if pt.get("build_id") == build_id():
                traffic = pt.get(dom)
            else:
                traffic_note = f"profiles/pmc_traffic.json is from build {pt.get('build_id')}, this is {build_id()}: not used"
        except Exception:
            pass
        # the same kernel family's average launch INSIDE the profiled step (profiles/kernel_stats.json: rocprofv3 --kernel-trace of this
        # command, tools/round_profile.sh; both launch streams busy, caches as the step leaves them) - the isolated HIP-event replay
        # above flatters a launch by up to 15 %.  Reported beside `frac` (`frac_in_step`) when the profile is of THIS build.
        in_step_ms = in_step_note = None
        try:
            import re
            with open(os.path.join(ROOT, "profiles", "kernel_stats.json")) as f:
                ks = json.load(f)
            pat = {"conv_gemm<bf16,strip>": r"conv1x1_strip(_res)?_kernel<\d+, \d+, \d+, 0, \d+>", "gn_conv1x1<bf16,strip>": r"conv1x1_strip(_res)?_kernel<\d+, \d+, \d+, [12], \d+>",
                   "conv_gemm<bf16,128glds>": r"conv_gemm_glds_kernel<.*, 2, (true|false)>", "conv_gemm<bf16,128ring>": r"conv_gemm_glds_kernel<.*, 4, (true|false)>",
                   "attn_fwd": r"attn_(dma|mfma|stage)_kernel", "vconv2d1d<bf16,gn>": r"vconv2d1d_kernel<[12]>", "gn_conv_gemm<bf16,256halo>": r"conv_gemm_halo16_kernel<true>"}.get(dom)
            if ks.get("build_id") != build_id():
                in_step_note = f"profiles/kernel_stats.json is from build {ks.get('build_id')}, this is {build_id()}: not used"
            elif pat:
                hit = [v for k, v in ks["kernels"].items() if re.search(pat, k)]
                if hit:
                    in_step_ms = sum(v["total_us"] for v in hit) / max(sum(v["calls"] for v in hit), 1) / 1e3
        except Exception:
            pass
        # which roof binds the dominant kernel: its arithmetic intensity against the ridge (MFMA peak / HBM peak = 312 flop/B in bf16)
        ridge = peak * 1e12 / (HBM_PEAK_GBS * 1e9)
        ai = a["flops"] / max(a["bytes"], 1)
        bound, unit = "mfma", "TFLOP/s"
        if ai < ridge:             # HBM-side kernel (elementwise, or a short-K GEMM): price the algorithmic bytes against 8 TB/s
            bound, unit, ach, peak = "hbm", "GB/s", a["bytes"] / (a["ms"] * 1e-3) / 1e9, HBM_PEAK_GBS
        iso_ms = a["ms"] / max(a["calls"], 1)
        ach_iso = ach                          # from the isolated HIP-event replay of this run
        # per-launch algorithmic work / the in-step launch time; with batch lanes the traced step's launches carry 1 / lanes of the work
        # of the (unsplit) plan the breakdown replays
        ach_step = ach * iso_ms / in_step_ms / timed_lanes if in_step_ms else None
        ach = ach_iso      # round 6: `frac` / `achieved` are THIS run's measurement; the in-step figure from the committed profile is a labelled side figure
        mfma_peak = MFMA_BF16_PEAK_TFLOPS if args.dtype == "bf16" else MFMA_F32_PEAK_TFLOPS
        res["roofline"] = {"kernel": dom, "bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
                           "frac_isolated": ach_iso / peak, "frac_in_step": (ach_step / peak) if ach_step is not None else None,
                           "frac_note": "frac = frac_isolated = this run's HIP-event replay of the family's launches on the launch stream; frac_in_step = the same work over the family's average launch inside the profiled step (profiles/kernel_stats.json: rocprofv3 kernel trace of this command, used only when its build id matches)",
                           "mfma_frac_of_peak_in_step": (a["flops"] / max(a["calls"], 1) / timed_lanes / (in_step_ms * 1e-3) / 1e12 / mfma_peak) if in_step_ms else None,
                           "avg_launch_ms_in_step": in_step_ms, "in_step_batch_lanes": timed_lanes, "avg_launch_ms_in_step_note": in_step_note or ("rocprofv3 kernel trace of this command, profiles/kernel_stats.json" if in_step_ms else "no profile of this build: frac is from the isolated replay"),
                           "arithmetic_intensity_flop_per_B": ai, "ridge_flop_per_B": ridge,
                           "mfma_frac_of_peak": a["flops"] / (a["ms"] * 1e-3) / 1e12 / (MFMA_BF16_PEAK_TFLOPS if args.dtype == "bf16" else MFMA_F32_PEAK_TFLOPS),
                           "traffic": traffic, "traffic_note": traffic_note, "launches_per_step": a["calls"], "avg_launch_ms": iso_ms,
                           "algorithmic_gflop_per_launch": a["flops"] / max(a["calls"], 1) / 1e9,
                           "algorithmic_MB_per_launch": a["bytes"] / max(a["calls"], 1) / 1e6,
                           "hbm_frac_of_8TBs": a["bytes"] / (a["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                           "share_of_step": a["ms"] / total_ms}
        res["kernel_ms_per_step"] = {k: round(v["ms"], 4) for k, v in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])}
        hb = {k: v for k, v in agg.items() if v["flops"] == 0 and v["bytes"] > 0}
        if hb:
            res["hbm_kernels_gbs"] = {k: round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) for k, v in hb.items()}
        # the two kernels BASELINE.md grades (batch 4, bf16): fused video ResBlock ds=1 128->128 and RS cross-attention ds=2
        tags = kernel_breakdown(stepper, reps=3, by_tag=True)
        rb, xa = tags.get("input_blocks.1.0:video"), tags.get("input_blocks.4.1:cross")
        if rb and xa:
            E = args.batch * 16 * 128 * 64 * 64 * 2          # one ds=1 activation tensor in bytes (bf16)
            # the ResBlock's launches as one hipGraph, cache-cold (its two ~4 us finalize launches are host-paced in the eager replay)
            rb_eager_ms = rb["ms"]
            ent = [e for e in (stepper.eng.plan_f32 if stepper.use_f32 else stepper.eng.plan) if e[0] is not None and e[5] == "input_blocks.1.0:video"]
            try:
                rb["ms"], rb_min = graph_replay_ms(stepper, ent)
            except Exception as ex:       # keep the eager figure, say why
                rb_min = None
                res.setdefault("notes", []).append(f"graded ResBlock: graph replay failed ({ex}); ms is the eager HIP-event replay")
            res["graded"] = {
                "video_resblock_ds1_128to128": {
                    "ms": rb["ms"], "ms_min": rb_min, "ms_eager_hip_events": rb_eager_ms,
                    "how": "median of 12 cache-cold replays of the block's launches as one hipGraph, HIP events on the launch stream (eager per-launch events: ms_eager_hip_events)",
                    "launches": rb["calls"], "min_traffic_MB": 6 * E / 1e6,
                    "hbm_GBs_at_min_traffic": 6 * E / (rb["ms"] * 1e-3) / 1e9, "frac_of_8TBs": 6 * E / (rb["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "TFLOPs": rb["flops"] / (rb["ms"] * 1e-3) / 1e12, "frac_of_mfma_peak": rb["flops"] / (rb["ms"] * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS},
                "rs_cross_attention_ds2": {
                    "block_ms": xa["ms"], "attn_kernels_ms": xa["attn_ms"], "attn_GFLOP": xa["attn_flops"] / 1e9,
                    "attn_TFLOPs": xa["attn_flops"] / (xa["attn_ms"] * 1e-3) / 1e12,
                    "frac_of_mfma_peak": xa["attn_flops"] / (xa["attn_ms"] * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS}}
        if args.breakdown_out:
            det = kernel_breakdown(stepper, reps=2, detail=True)
            with open(args.breakdown_out, "w") as f:
                json.dump(dict(sorted(det.items(), key=lambda kv: -kv[1]["ms"])), f, indent=1)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(fl)
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
