"""What the compiler made of the inline-asm arithmetic chains, per kernel, from the sources.

Cross-compiles the library's .hip files device-only for gfx950 (`hipcc -S`, no GPU needed) and
prints per kernel: VALU instructions, v_mad_u64_u32 among them, `s_nop` (the wait state the compiler
pads an asm statement with when the next instruction reads a VGPR it wrote), asm statements, and
the register figures of the compiler's own summary (NumVgprs, NumAgprs, ScratchSize, Occupancy).
These are static counts of straight-line bodies; it counts nothing else.

Usage: python tools/isa_chains.py [--csrc DIR] [--jobs N] [--match SUBSTRING ...] [FILE.hip ...]
  --csrc   the tree to compile (default: this checkout's csrc; another checkout's for a comparison)
  --match  print only kernels whose demangled name holds one of the substrings
profiles/r08/isa_parent.txt and isa_this.txt are its output for the parent commit and this tree."""
import argparse
import collections
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "midnight-bls12-381-cuda_amd", "csrc")
FIELDS = ("valu", "v_mad_u64_u32", "s_nop", "asm", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")


def hipcc():
    cand = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cand if os.path.exists(cand) else shutil.which("hipcc")


def compile_asm(src, includes, arch="gfx950"):
    """gfx950 assembly text of one .hip file"""
    cmd = [hipcc(), f"--offload-arch={arch}", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", "-", src]
    cmd += ["-I" + i for i in includes]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def count_kernels(asm):
    """{kernel symbol: {field: count}} over the kernels (.amdhsa_kernel entries) of an assembly text"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out = {}
    sym = None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and not m.group(1).startswith(".L"):
            sym = m.group(1) if m.group(1) in kernels else None
            if sym:
                out[sym] = collections.Counter()
            continue
        if sym is None:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end"):
            continue
        if t.startswith(";;#ASMSTART"):
            out[sym]["asm"] += 1
            continue
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", t)
        if m:
            out[sym][m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                sym = None  # the summary's last figure of interest: the next label opens another function
            continue
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("v_"):
            out[sym]["valu"] += 1
        if op == "v_mad_u64_u32":
            out[sym]["v_mad_u64_u32"] += 1
        if op == "s_nop":
            out[sym]["s_nop"] += 1
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    d = r.stdout.splitlines() if r.returncode == 0 else names
    return dict(zip(names, d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--match", nargs="*", default=[])
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    if not hipcc():
        sys.exit("hipcc not found")
    files = a.files or sorted(glob.glob(os.path.join(a.csrc, "*.hip")))
    inc = [a.csrc, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(a.csrc))), "include")]
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        texts = list(ex.map(lambda f: compile_asm(f, inc), files))
    print(f"{'kernel':<72} " + " ".join(f"{f:>13}" if f == "v_mad_u64_u32" else f"{f:>11}" for f in FIELDS))
    for f, text in zip(files, texts):
        counts = count_kernels(text)
        names = demangle(sorted(counts))
        rows = [(names[s], counts[s]) for s in sorted(counts, key=lambda s: names[s])]
        rows = [r for r in rows if not a.match or any(m in r[0] for m in a.match)]
        if not rows:
            continue
        print(f"# {os.path.basename(f)}")
        for name, c in rows:
            name = re.sub(r"^void ", "", name)
            name = name if len(name) <= 72 else name[:69] + "..."
            print(f"{name:<72} " + " ".join(f"{c[k]:>13}" if k == "v_mad_u64_u32" else f"{c[k]:>11}" for k in FIELDS))


if __name__ == "__main__":
    main()
