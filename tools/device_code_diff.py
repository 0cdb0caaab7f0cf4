#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libmmd kernel by kernel: a change that must not reach device code (a host-side refactor
under csrc/) is checked on a machine without a GPU.

    python tools/device_code_diff.py [--by-name] OLD NEW        OLD / NEW: a libmmd.so, or a directory of objects (mmd_*.o)

The code objects are paired in bundle order (the library: link order; a directory: by file name).  Per pair: the set of symbols, the
disassembly of every symbol (compared by name, not by position) and the resource metadata of every kernel must be equal.  File hashes
are not compared: a code object embeds its source path.  Exit status 1 if anything differs.

--by-name: for a change that moves kernels between source files.  The symbols and the metadata of ALL code objects of a build are
pooled and compared by name - the demangled name without its parameter list, so a kernel whose argument types changed still meets its
old self; a kernel that differs is listed with its VGPRs, SGPRs, LDS, scratch and instruction count on both sides."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mmd_build", os.path.join(ROOT, "mm-diffusion_amd", "build.py"))
build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build)
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".max_flat_workgroup_size")


def _run(tool, *args):
    return subprocess.run([os.path.join(build._llvm_bin(), tool), *args], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.decode(errors="replace")


def _bare(demangled):
    """'void k<float, 2>(P, float const*)' -> 'void k<float, 2>': the text in front of the parameter list"""
    if not demangled.endswith(")"):
        return demangled
    depth = 0
    for i in range(len(demangled) - 1, -1, -1):
        depth += {")": 1, "(": -1}.get(demangled[i], 0)
        if depth == 0:
            return demangled[:i]
    return demangled


def code_objects(path, td, by_name=False):
    """-> [(label, {symbol: disassembly lines}, {kernel: metadata tuple})] of the gfx950 code objects of a library or a directory of objects"""
    files = [path] if os.path.isfile(path) else sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".o"))
    out = []
    for i, f in enumerate(files):
        sub = os.path.join(td, str(i))
        os.mkdir(sub)
        for j, co in enumerate(build._code_objects(f, sub)):
            syms, cur = {}, None
            header = re.compile(r"^[0-9a-f]* ?<(.*)>:$")
            names = {}
            if by_name:          # mangled -> bare demangled name: the same headers in the same order, read with objdump's demangler
                plain = [m.group(1) for m in map(header.match, _run("llvm-objdump", "-d", "--mcpu=gfx950", co).split("\n")) if m]
                dem = [m.group(1) for m in map(header.match, _run("llvm-objdump", "-d", "-C", "--mcpu=gfx950", co).split("\n")) if m]
                assert len(plain) == len(dem)
                names = {a: _bare(b) for a, b in zip(plain, dem)}
            for line in _run("llvm-objdump", "-d", "--mcpu=gfx950", "--no-leading-addr", "--no-show-raw-insn", co).split("\n"):
                m = header.match(line)
                if m:
                    cur = syms.setdefault(names.get(m.group(1), m.group(1)), [])
                elif cur is not None and line.strip() not in ("", "..."):          # "...": zero padding up to the next symbol's alignment
                    cur.append(re.sub(r"// [0-9A-F]+:", "//", line.strip()))      # the address moves with the kernel's place in the object
            meta = {}
            for entry in re.split(r"\n  - ", _run("llvm-readelf", "--notes", co))[1:]:
                name = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
                if name:
                    meta[names.get(name.group(1), name.group(1))] = tuple(re.search(r"^\s+\%s:\s+(\d+)" % k, entry, re.M).group(1) for k in META)
            if by_name:
                for k, v in syms.items():
                    while v and v[-1].split()[0] in ("s_code_end", "s_nop"):      # the padding behind the last kernel of an object: not the kernel's
                        v.pop()
                    syms[k] = [re.sub(r" <[^>]*\+0x[0-9a-f]+>$", "", ln) for ln in v]      # a branch comment names the (mangled) kernel
            out.append(("%s#%d" % (os.path.basename(f), j), syms, meta))
    return out


def pooled(cos):
    """One (label, symbols, metadata) over all code objects of a build; a name defined in two of them (an instantiation local to each)
    keeps every definition, in bundle order; the metadata kept for such a name is that of the last object that defines it (libmmd's
    kernel names are unique across its source files)."""
    syms, meta = {}, {}
    for _, s, m in cos:
        for k, v in s.items():
            syms.setdefault(k, []).extend(v)
        meta.update(m)
    return [("all code objects", syms, meta)]


def main():
    args = [a for a in sys.argv[1:] if a != "--by-name"]
    by_name = len(args) != len(sys.argv) - 1
    if len(args) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        old, new = code_objects(args[0], ta, by_name), code_objects(args[1], tb, by_name)
    if by_name:
        old, new = pooled(old), pooled(new)
    bad = 0
    if len(old) != len(new) or not old:
        print("code objects: %d in OLD, %d in NEW" % (len(old), len(new)))
        return 1
    for (label, sa, ma), (_, sb, mb) in zip(old, new):
        diffs = ["only in OLD: " + s for s in sorted(set(sa) - set(sb))] + ["only in NEW: " + s for s in sorted(set(sb) - set(sa))]
        diffs += ["disassembly differs: " + s for s in sorted(set(sa) & set(sb)) if sa[s] != sb[s]]
        diffs += ["metadata differs: %s %s -> %s" % (k, ma[k], mb[k]) for k in sorted(set(ma) & set(mb)) if ma[k] != mb[k]]
        if by_name:          # old -> new resources of every kernel named above
            for k in sorted(k for k in set(ma) & set(mb) if sa.get(k) != sb.get(k) or ma[k] != mb[k]):
                diffs.append("    %s: " % k + ", ".join("%s %s -> %s" % (n, a, b) for n, a, b in zip(("vgpr", "sgpr", "lds", "scratch"), ma[k], mb[k])) +
                             ", instructions %d -> %d" % (len(sa.get(k, ())), len(sb.get(k, ()))))
        if set(ma) != set(mb):
            diffs.append("kernel metadata entries differ: %s" % sorted(set(ma) ^ set(mb)))
        print("%-22s %4d kernels %5d symbols %8d disassembly lines: %s" %
              (label, len(ma), len(sa), sum(len(v) for v in sa.values()), "identical" if not diffs else "%d DIFFERENCES" % len(diffs)))
        for d in diffs:
            print("    " + d)
        bad += len(diffs)
    print("%d code objects, %d kernels, %d differences" % (len(old), sum(len(m) for _, _, m in old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
