#!/usr/bin/env python3
"""The gfx950 device code inside a built libvxba.so, for comparing two builds: per code object its SHA-256, its number of kernels and a digest of
all its kernels' rows (name, registers, LDS, scratch, spills as the metadata states them), then the rows themselves of the kernels whose name
contains one of the given substrings (default: the kernels the host launchers of vxba_kernels.hip and vxba_wide.hip choose between).  Two builds
with equal output run the same device code.  (scripts/kernel_regs.py compiles one unit from source; this reads what was built.)

    python scripts/kernel_table.py [path/to/libvxba.so [substring ...]] > table.txt
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")

lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "voxel-slam_amd", "csrc", "libvxba.so")
show = sys.argv[2:] or ["k2_residual_kernel", "k3_hessian_kernel", "k23_fused_kernel", "k3_finalize_kernel", "lm_solve_kernel", "k1_build_rows_kernel", "wchol_persistent_kernel"]
objects, shown = [], []
with tempfile.TemporaryDirectory() as td:
    so = os.path.join(td, "libvxba.so")
    shutil.copy(lib, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=td)   # writes the code objects next to its input
    for fn in sorted(os.listdir(td)):
        if "gfx950" not in fn:
            continue
        with open(os.path.join(td, fn), "rb") as fh:
            sha = hashlib.sha256(fh.read()).hexdigest()
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(td, fn)], check=True, capture_output=True, text=True).stdout
        rows = []
        # a kernel's record is a list item that opens with its first key, .agpr_count; its own keys sit two columns right of the dash, its arguments' deeper
        for m in re.finditer(r"^( +)- (\.agpr_count:.*?)(?=^ +- \.agpr_count:|^\S|\Z)", notes, re.S | re.M):
            pad = " " * (len(m.group(1)) + 2)
            rec = dict(re.findall(r"^%s\.(\w+):\s+(\S+)" % pad, pad + m.group(2), re.M))
            rows.append(" ".join("%5s" % rec.get(k, "-") for k in KEYS) + " " + rec["name"])
        rows.sort()
        objects.append((sha, len(rows), hashlib.sha256("\n".join(rows).encode()).hexdigest()))
        shown += [r for r in rows if any(s in r for s in show)]
print("# %d kernels in %d gfx950 code objects" % (sum(o[1] for o in objects), len(objects)))
for sha, n, digest in sorted(objects):
    print("# code object sha256 %s: %4d kernels, sha256 of their rows %s" % (sha, n, digest))
print("# vgpr agpr sgpr lds scratch vgpr_spill sgpr_spill name, of the kernels with one of: " + " ".join(show))
names = [r.split()[-1] for r in shown]
dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines() if names else []
for r, d in sorted(zip(shown, dem), key=lambda t: t[1]):
    print(r.rsplit(" ", 1)[0], re.sub(r"\(.*", "", d).replace("void ", ""))
