#!/usr/bin/env python3
"""Build libmmd.so (the C-ABI HIP library) for gfx950 with hipcc, in-tree.

    python mm-diffusion_amd/build.py [--force]

Output: mm-diffusion_amd/lib/libmmd.so (git-ignored; it travels to the GPU box with the snapshot).
hipcc cross-compiles gfx950 without a GPU present.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "lib", "libmmd.so")
SOURCES = ["mmd_core.hip", "mmd_gemm.hip", "mmd_vconv.hip", "mmd_tattn.hip", "mmd_tconv.hip", "mmd_aconv.hip", "mmd_rtail.hip", "mmd_norm.hip", "mmd_attn.hip", "mmd_misc.hip", "mmd_edge.hip", "mmd_diffusion.hip", "mmd_dpm.hip", "mmd_adapt.hip", "mmd_wgrad.hip", "mmd_gn_bwd.hip", "mmd_optim.hip", "mmd_attn_bwd.hip", "mmd_attn_bwd_mfma.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-result", "-Wno-inline-asm"]
FLAGS += os.environ.get("MMD_EXTRA_CXXFLAGS", "").split()      # ablation builds (tools/*_bench.py), never set for the product
# The library is built WITHOUT the packed-fp32 VALU instructions (v_pk_add_f32 / v_pk_fma_f32 / v_pk_mul_f32).  Measured on MI355X
# (round 3, tools/determinism_mini.py): gn_small_kernel's packed accumulations came out slightly wrong in lanes 48-63 (high register of
# the pair) whenever its waves shared a SIMD with the OTHER stream's GroupNorm+SiLU-in-the-loader GEMM (v_exp / v_rcp heavy) - 200 of
# 200 concurrent graph replays differed, 0 of 900 with the kernel compiled without packed fp32; nothing in the kernel's own ISA is
# wrong.  Library-wide the switch costs nothing (denoising step 12.07 -> 12.02 ms: the hot loops are MFMA / LDS / issue bound), so no
# kernel is left exposed.  tests/test_round3_gpu.py::test_graph_replays_are_bitwise_repeatable_* guards it.
NO_PACKED_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FLAGS += NO_PACKED_F32


def _stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(SRC, f) for f in os.listdir(SRC)] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def _llvm_bin():
    """Directory of llvm-objdump: LLVM_BIN, else next to the clang the hipcc in use drives (`hipcc --print-prog-name`), else the stock
    ROCm location.  A missing objdump is a clear error, not a bare FileNotFoundError at the end of a ten-minute build."""
    cands = [os.environ.get("LLVM_BIN")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        out = subprocess.run([hipcc, "--print-prog-name=llvm-objdump"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=60).stdout.decode().strip()
        if out and os.path.isabs(out):
            cands.append(os.path.dirname(out))
    except (OSError, subprocess.SubprocessError):
        pass
    cands += [os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin"), "/opt/rocm/lib/llvm/bin"]
    for d in cands:
        if d and os.path.exists(os.path.join(d, "llvm-objdump")):
            return d
    raise RuntimeError("build check: llvm-objdump not found (looked in %s); set LLVM_BIN to the LLVM bin directory of the ROCm toolchain"
                       % ", ".join(str(d) for d in cands if d))


def _code_objects(path, td):
    """Unbundle the fat binary `path` (the library or one object) into the directory `td`; returns the paths of its gfx950 code objects
    in bundle order.  `llvm-objdump --offloading` writes every bundle next to its input (one gfx950 code object per source file)."""
    lib = os.path.join(td, os.path.basename(path))
    os.symlink(os.path.abspath(path), lib)
    subprocess.check_call([os.path.join(_llvm_bin(), "llvm-objdump"), "--offloading", lib], cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = [f for f in os.listdir(td) if f.startswith(os.path.basename(path) + ".") and f.endswith("gfx950")]
    return [os.path.join(td, f) for f in sorted(cos, key=lambda f: (len(f), f))]      # lib.so.2.* before lib.so.10.*


def _check_no_packed_f32(path):
    """Disassemble the device code of the linked library and refuse it if any packed-fp32 VALU instruction survived: the feature
    string above is an internal clang spelling, and a compiler that stops recognising it for the DEVICE pass would bring the
    instructions - and the wrong GroupNorm statistics - back without a word."""
    import re
    import tempfile
    llvm = _llvm_bin()
    with tempfile.TemporaryDirectory() as td:
        cos = _code_objects(path, td)
        if len(cos) < len(SOURCES) - 1:          # (mmd_core.hip has no kernels)
            raise RuntimeError("build check: expected >= %d gfx950 code objects in %s, found %d" % (len(SOURCES) - 1, path, len(cos)))
        asm = ""
        for f in cos:
            asm += subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--mcpu=gfx950", f],
                                  stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.decode(errors="replace")
    n_mfma = len(re.findall(r"\bv_mfma_", asm))
    bad = re.findall(r"\bv_pk_(?:add|mul|fma)_f32\b", asm)
    if n_mfma == 0:
        raise RuntimeError("build check: the disassembly of %s shows no v_mfma instruction - the check looked at the wrong object" % path)
    if bad:
        raise RuntimeError("build check: %d packed-fp32 instruction(s) (%s ...) in %s: the device pass ignored %s" %
                           (len(bad), bad[0], path, " ".join(NO_PACKED_F32)))


def _check_strip_asm(obj):
    """The pipelined row-strip GEMM keeps in-flight residual rows in v[248:255] of kernels limited to 248 allocatable VGPRs; refuse the
    build if any compiler-generated instruction of those kernels names one of the registers (tools/strip_asm_check.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("strip_asm_check", os.path.join(os.path.dirname(HERE), "tools", "strip_asm_check.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    chk.LLVM = _llvm_bin()
    n, bad = chk.check(chk.disassemble(obj))
    if n == 0 or bad:
        raise RuntimeError("build check: conv1x1_strip_res_kernel: %d kernels checked, %d violations%s" % (n, len(bad), (": " + bad[0]) if bad else ""))


def build(force=False, verbose=True):
    if not force and not _stale():
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    for s in SOURCES:
        o = os.path.join(HERE, "lib", s.replace(".hip", ".o"))
        objs.append(o)
        cmd = [hipcc, *FLAGS, "-c", os.path.join(SRC, s), "-o", o]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode()))
        # The x86 HOST pass of the same command does not know the AMDGPU feature and says so once per file: that line is filtered from
        # the printout.  Whether the DEVICE pass honoured the flag is decided by the disassembly check below, not by compiler chatter.
        lines = out.decode().splitlines()
        text = "\n".join(ln for ln in lines if "'-packed-fp32-ops' is not a recognized feature" not in ln).strip()
        if verbose and text:
            print(text)
    tmp = OUT + ".tmp"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp, *objs]
    try:
        subprocess.check_call(cmd)
        _check_no_packed_f32(tmp)            # raises: no half-checked library is left under the product's name ...
        _check_strip_asm(os.path.join(HERE, "lib", "mmd_gemm.o"))
        os.replace(tmp, OUT)
    finally:
        if os.path.exists(tmp):              # ... and no rejected one next to it
            os.remove(tmp)
    if verbose:
        print("built", OUT)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
