#!/usr/bin/env python3
"""Diagnostic (GPU): the launch plan of a model's engine as text, one line per plan entry, with every pointer in a canonical form - so
that two versions of the package can be compared byte for byte (same calls, same arguments, same streams, same buffer reuse).

    plan_dump.py --out DIR [--package DIR]       every arm of ARMS, each in a fresh process under its own time limit; stops at the
                                                 first failure; prints one line per arm: arm, plan entries, _pick_tile calls, sha256
    plan_dump.py --arm NAME --out FILE [--package DIR]       one arm in this process
    plan_dump.py --only stepper- --out DIR [--package DIR]   the arms whose name contains the text (here: the stepper arms)

--package: the directory that holds the `mm_diffusion` package to dump (default: mm-diffusion_amd of this tree).  A package copied
elsewhere without a library next to it uses this tree's libmmd.so (MMD_LIB).  Only model._engines, eng.plan, eng.plan_f32, eng.pools
and ops._pick_tile are used.  ops.AUTOTUNE is switched off (a timing-based tile choice is not repeatable); the candidate lists of every
_pick_tile call are logged and compared instead.

The stepper arms (STEPPER_ARMS, tiny configuration in fp32) dump the plans a sampling stepper records around the U-Net plan instead:
sampler.GraphStepper built directly, sampler.DpmppStepper as DPM_Solver.sample_graph leaves it in solver._stepper.  Only st.engs,
st.use_f32, st.pre_plans, st.update_plans and getattr(st, "final_plans", []) are read; pointers are canonical against the pools of every
lane's engine."""
import argparse
import ctypes
import hashlib
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARM_TIMEOUT = 240           # seconds per arm: model build + one forward of the largest configuration takes well under a minute


def _arm(config, dtype, batch, **env):
    return dict(config=config, dtype=dtype, batch=batch, env=env)


ARMS = {
    "full-bf16-b1": _arm("full", "bf16", 1),
    "full-bf16-b2": _arm("full", "bf16", 2),
    "full-bf16-b4": _arm("full", "bf16", 4),
    "full-fp32-b1": _arm("full", "fp32", 1),
    "mid-bf16-b2": _arm("mid", "bf16", 2),
    "full-fp32-b1-MMD_GN_EPILOGUE=2": _arm("full", "fp32", 1, MMD_GN_EPILOGUE="2"),
}
for _k, _v in [("MMD_TCONV", "0"), ("MMD_HALO_GN", "0"), ("MMD_VCONV_FUSED", "0"), ("MMD_ACONV", "0"), ("MMD_TATTN_FUSED", "0"),
               ("MMD_TATTN_PRE", "0"), ("MMD_GN_GROUP", "0"), ("MMD_GN_SMALL", "0"), ("MMD_GN_EPILOGUE", "0"), ("MMD_UP_LOWRES", "0"),
               ("MMD_RESAMPLE_STATS", "0"), ("MMD_SKIP_FUSE", "0"), ("MMD_TAIL_STREAM", "0"), ("MMD_CROSS_SERIAL", "0"), ("MMD_HEAD_GEMM", "0"), ("MMD_EMB_AUX", "0"),
               ("MMD_GEMM_STRIP", "0"), ("MMD_GEMM_STRIP", "base"), ("MMD_GEMM_HALO", "0"), ("MMD_GEMM_HALO", "1"), ("MMD_HALO16", "0"),
               ("MMD_GEMM_RING", "0")]:
    ARMS[f"full-bf16-b2-{_k}={_v}"] = _arm("full", "bf16", 2, **{_k: _v})


def _st(kind, batch, lanes, **kw):
    return dict(kind=kind, batch=batch, lanes=lanes, kw=kw, env={})


STEPPER_ARMS = {
    "stepper-ddpm": _st("graph", 2, 1, update="ddpm"),
    "stepper-ddim": _st("graph", 2, 1, update="ddim", eta=0.5),
    "stepper-vlb": _st("graph", 2, 1, update="vlb"),
    "stepper-ddpm-ctr": _st("graph", 4, 2, update="ddpm", ctr=True),
    "stepper-ddim-ctr": _st("graph", 4, 2, update="ddim", eta=0.5, ctr=True),
    "stepper-ddpm-cond": _st("graph", 2, 1, update="ddpm", cond=("video", "audio+mask")),
    "stepper-ddim-cond-ctr": _st("graph", 4, 2, update="ddim", eta=0.5, ctr=True, cond=("audio",)),
    "stepper-ddpm-rescale": _st("graph", 2, 1, update="ddpm", rescale=True),
    "stepper-dpmpp-x0-thr-multi": _st("dpmpp", 2, 1, predict_x0=True, thresholding=True, select="multi"),
    "stepper-dpmpp-x0-thr-block": _st("dpmpp", 2, 1, predict_x0=True, thresholding=True, select="block"),
    "stepper-dpmpp-eps-denoise": _st("dpmpp", 4, 2, predict_x0=False, denoise=True),
    "stepper-dpmpp-x0-cond-ctr": _st("dpmpp", 2, 1, predict_x0=True, ctr=True, cond=("video", "audio+mask")),
}


def _canon(spans):
    """canon(x) for plan arguments: pointers into `spans` ((lo, hi, name) of the pool blocks) by block and offset, other pointers by
    order of appearance, handles as such."""
    ext = {}

    def canon(x):
        if isinstance(x, ctypes.Array):
            return "[" + ",".join(str(int(e)) for e in x) + "]"
        if isinstance(x, ctypes.c_void_p):
            return "handle"
        if isinstance(x, int) and not isinstance(x, bool):
            for lo, hi, name in spans:
                if lo <= x < hi:
                    return f"{name}+{x - lo}"
            if x > (1 << 32):
                return f"ext{ext.setdefault(x, len(ext))}"
        return repr(x)
    return canon


def _plan_lines(pname, plan, canon):
    lines = []
    for i, (fn, args, name, meta, sid, tag) in enumerate(plan):
        if fn is None:
            lines.append(f"{pname} {i} sync {args[0]} {args[1]}")
        else:
            lines.append(f"{pname} {i} {name} sid={sid} tag={tag!r} meta={meta!r} args=(" + ", ".join(canon(x) for x in args) + ")")
    return lines


def _setup(package):
    if not os.path.exists(os.path.join(package, "lib", "libmmd.so")):
        os.environ.setdefault("MMD_LIB", os.path.join(ROOT, "mm-diffusion_amd", "lib", "libmmd.so"))
    sys.path.insert(0, package)
    sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump_stepper(arm, package, out):
    """One stepper arm in this process."""
    _setup(package)
    import torch
    from helpers import flags
    from mm_diffusion import masking, sampler
    from mm_diffusion import multimodal_script_util as msu
    from mm_diffusion.seeded import CounterNoise
    from mm_diffusion.synth import synth_init_

    a = STEPPER_ARMS[arm]
    kw, B = dict(a["kw"]), a["batch"]
    fl = flags("tiny", use_fp16=False, rescale_timesteps=bool(kw.pop("rescale", False)))
    model, diff = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.cuda().eval()
    shape = {"video": (B, *fl["video_size"]), "audio": (B, *fl["audio_size"])}
    ctr = CounterNoise(1234) if kw.pop("ctr", False) else None
    known, mask = {}, {}
    for c in kw.pop("cond", ()):
        k = c.split("+")[0]
        known[k] = torch.zeros(shape[k], device="cuda")
        if c.endswith("+mask"):
            mask[k] = masking.prefix_masks(fl["video_size"], fl["audio_size"], 3)[k]
    random.seed(5)
    if a["kind"] == "graph":
        diff.noise_source = ctr
        cond = masking.normalize(known, mask or None, shape) if known else None
        st = sampler.GraphStepper(diff, model, B, torch.device("cuda"), lanes=a["lanes"], cond=cond, **kw)
    else:
        from mm_diffusion.multimodal_dpm_solver_plus import DPM_Solver
        sampler.DPMPP_SELECT = kw.pop("select", sampler.DPMPP_SELECT)
        solver = DPM_Solver(model=model, alphas_cumprod=torch.tensor(diff.alphas_cumprod, dtype=torch.float32), predict_x0=kw.pop("predict_x0"),
                            thresholding=kw.pop("thresholding", False))
        torch.manual_seed(5)
        solver.sample_graph(shape=shape, steps=3, order=2, lanes=a["lanes"], noise_source=ctr, known=known or None, mask=mask or None, **kw)
        st = solver._stepper[1]
    canon = _canon([(b.data_ptr(), b.data_ptr() + b.numel(), f"lane{r}.pool{si}.{bi}")
                    for r, e in enumerate(st.engs) for si, p in enumerate(e.pools) for bi, b in enumerate(p.all)])
    lines = [f"arm {arm}", f"lanes {len(st.engs)} use_f32 {bool(st.use_f32)}"]
    for pname in ("pre_plans", "update_plans", "final_plans"):
        plans = getattr(st, pname, [])
        lines.append(f"{pname} {len(plans)}")
        for r, plan in enumerate(plans):
            lines += _plan_lines(f"{pname}[{r}]", plan, canon)
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(f"{arm} entries={len(lines) - 5} sha256={hashlib.sha256(text.encode()).hexdigest()}", flush=True)


def dump(arm, package, out):
    """One arm in this process (the environment of the arm is already set)."""
    if arm in STEPPER_ARMS:
        return dump_stepper(arm, package, out)
    _setup(package)
    import torch
    from helpers import flags, inputs
    from mm_diffusion import multimodal_script_util as msu
    from mm_diffusion import ops
    from mm_diffusion.synth import synth_init_

    ops.AUTOTUNE = False
    picks = []
    pick = ops._pick_tile

    def logged(key, launch, M, Cout, candidates=(64, 128, 129), **kw):
        picks.append((key, tuple(candidates)))
        return pick(key, launch, M, Cout, candidates, **kw)

    ops._pick_tile = logged
    a = ARMS[arm]
    fl = flags(a["config"], use_fp16=a["dtype"] == "bf16")
    model, _ = msu.create_model_and_diffusion(**fl)
    synth_init_(model)
    model.cuda().eval()
    B = a["batch"]
    v, au = inputs(fl, B, 3)
    random.seed(5)
    with torch.no_grad():
        model(v.cuda(), au.cuda(), torch.tensor([17, 400, 3, 999][:B]).cuda())
    eng = next(iter(model._engines.values()))
    canon = _canon([(r.data_ptr(), r.data_ptr() + r.numel(), f"pool{si}.{bi}") for si, p in enumerate(eng.pools) for bi, r in enumerate(p.all)])
    lines = [f"arm {arm}"]
    for si, p in enumerate(eng.pools):
        lines.append(f"pool{si} " + " ".join(str(r.numel()) for r in p.all))
    for pname in ("plan", "plan_f32"):
        lines += _plan_lines(pname, getattr(eng, pname), canon)
    for i, (key, cands) in enumerate(picks):
        lines.append(f"pick {i} {key!r} {cands!r}")
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(f"{arm} entries={len(eng.plan)} picks={len(picks)} sha256={hashlib.sha256(text.encode()).hexdigest()}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.join(ROOT, "mm-diffusion_amd"))
    ap.add_argument("--arm", default="")
    ap.add_argument("--only", default="", help="run the arms whose name contains this text")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    package = os.path.abspath(args.package)
    if args.arm:
        dump(args.arm, package, args.out)
        return 0
    os.makedirs(args.out, exist_ok=True)
    for arm, a in {**ARMS, **STEPPER_ARMS}.items():
        if args.only not in arm:
            continue
        env = dict(os.environ)
        env.update(a["env"])
        cmd = ["timeout", "-k", "10", str(ARM_TIMEOUT), sys.executable, os.path.abspath(__file__), "--package", package, "--arm", arm,
               "--out", os.path.join(args.out, arm + ".txt")]
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            print(f"{arm}: exit status {rc} - stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
