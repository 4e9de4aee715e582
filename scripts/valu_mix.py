#!/usr/bin/env python3
"""Vector-ALU instruction mix of a sweep kernel, per barrier-delimited segment and per source line (no GPU needed).

Compiles vxba_kernels.hip to gfx950 assembly with the Makefile's flags plus -gline-tables-only (the .loc lines attribute every instruction to a
source line: the innermost inlined one) and, for every kernel whose demangled name contains one of the given strings, prints
  * per segment between consecutive workgroup barriers (s_barrier), in program order, the number of vector-ALU instructions by class:
    fp64 arithmetic | MFMA | v_mov* | v_cndmask* | v_cmp* | cross-lane (DPP, readlane, permlane, swap) | other (integer, conversions, bit ops);
  * the source lines with the most NON-arithmetic vector-ALU instructions (everything but fp64 and MFMA).
The counts are STATIC: both sides of every branch, a loop body once -- a budget to judge a change against, not a measurement (the measured
figure is SQ_INSTS_VALU - SQ_INSTS_MFMA per wave, profiles/r05_k3/pmc_sq_counters.json).  Only opcodes that begin with v_ are classified.

  python scripts/valu_mix.py 'k23_fused_kernel<10, false, false, true>' 'k3_hessian_kernel<10, false, false>' 'k2_residual_kernel<10, false, false>'
  python scripts/valu_mix.py --asm kernels.s --top 30 k23_fused_kernel      # reuse an assembly file
"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxel-slam_amd", "csrc")
CLASSES = ("fp64", "mfma", "mov", "cndmask", "cmp", "xlane", "other")


def makefile_flags():
    """HIPFLAGS of csrc/Makefile with its variables expanded (warnings dropped)."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*\?=\s*(.*)$", text, re.M)}
    flags = var["HIPFLAGS"]
    for _ in range(4):
        flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), flags)
    return [f for f in flags.split() if not f.startswith("-W")]


def classify(op, operands):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "mfma"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.endswith("_dpp") or "quad_perm" in operands or "row_" in operands or "wave_" in operands or op.startswith(("v_readlane", "v_readfirstlane", "v_writelane", "v_permlane", "v_swap")):
        return "xlane"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"):
        return "mov"
    if re.search(r"_f64(_e32|_e64)?$", op) and not op.startswith("v_cvt"):
        return "fp64"
    return "other"


def kernels(asm):
    """{mangled name: list of body lines} of every .type @function symbol."""
    out, name, body = {}, None, []
    for line in asm:
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def analyse(body, files, only_segment=None):
    segs = [dict(start="kernel entry", n=collections.Counter())]
    lines = collections.defaultdict(collections.Counter)
    loc = ("?", 0)
    for line in body:
        s = line.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            loc = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
            continue
        if not s or s.startswith((".", ";")) or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        op, operands = parts[0], (parts[1] if len(parts) > 1 else "")
        if op == "s_barrier":
            segs.append(dict(start=f"barrier at {loc[0]}:{loc[1]}", n=collections.Counter()))
            continue
        if not op.startswith("v_"):
            continue
        c = classify(op, operands)
        segs[-1]["n"][c] += 1
        if only_segment is None or only_segment == len(segs) - 1:
            lines[loc][c] += 1
    return segs, lines


def report(dem, segs, lines, top):
    print(f"== {dem}")
    hdr = "  %-4s %-44s %6s | " % ("seg", "starts behind", "VALU") + " ".join("%7s" % c for c in CLASSES) + " | non-arith"
    print(hdr)
    tot = collections.Counter()
    for i, sg in enumerate(segs):
        n = sg["n"]
        tot.update(n)
        allv = sum(n.values())
        print("  %-4d %-44s %6d | " % (i, sg["start"][:44], allv) + " ".join("%7d" % n[c] for c in CLASSES) + " | %6d" % (allv - n["fp64"] - n["mfma"]))
    allv = sum(tot.values())
    print("  %-4s %-44s %6d | " % ("all", "", allv) + " ".join("%7d" % tot[c] for c in CLASSES) + " | %6d" % (allv - tot["fp64"] - tot["mfma"]))
    print(f"  top {top} source lines by non-arithmetic vector-ALU instructions (mov / cndmask / cmp / xlane / other):")
    rank = sorted(lines.items(), key=lambda kv: -(sum(kv[1].values()) - kv[1]["fp64"] - kv[1]["mfma"]))[:top]
    for (f, ln), n in rank:
        non = sum(n.values()) - n["fp64"] - n["mfma"]
        if non == 0:
            break
        print("    %5d  %-28s mov %4d cndmask %4d cmp %4d xlane %4d other %4d   (fp64 on the line: %d)" % (non, f"{f}:{ln}", n["mov"], n["cndmask"], n["cmp"], n["xlane"], n["other"], n["fp64"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("kernels", nargs="*", default=["k23_fused_kernel<10, false, false, true>", "k3_hessian_kernel<10, false, false>", "k2_residual_kernel<10, false, false>"])
    ap.add_argument("--asm", help="reuse this assembly file instead of compiling (written there if it does not exist)")
    ap.add_argument("--top", type=int, default=25)
    ap.add_argument("--segment", type=int, default=None, help="rank the source lines of this segment only")
    args = ap.parse_args()
    def compile_to(path):   # the compiler's messages go to the terminal: a compile error is read there
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run([hipcc] + makefile_flags() + ["-gline-tables-only", "--offload-device-only", "-S", os.path.join(CSRC, "vxba_kernels.hip"), "-o", path], check=True)
    if args.asm:
        if not os.path.exists(args.asm):
            compile_to(args.asm)
        asm = open(args.asm).read().splitlines()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            compile_to(os.path.join(tmp, "vxba_kernels.s"))
            asm = open(os.path.join(tmp, "vxba_kernels.s")).read().splitlines()
    files = {}
    for line in asm:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', line)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
    ks = kernels(asm)
    names = list(ks)
    dems = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    for name, dem in zip(names, dems):
        short = re.sub(r"\(.*", "", dem).replace("void vxk::", "")
        if any(short.endswith(k) or (("<" not in k) and k in short) for k in args.kernels):
            segs, lines = analyse(ks[name], files, args.segment)
            report(short, segs, lines, args.top)


if __name__ == "__main__":
    main()
