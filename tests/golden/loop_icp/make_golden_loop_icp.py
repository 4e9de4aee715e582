"""Regenerates tests/golden/loop_icp/loop_icp.npz from the reference's own icp_normal (run where the reference's sources are present):

    python tests/golden/loop_icp/make_golden_loop_icp.py

icp_normal (loop_refine.hpp:47-145) is not behind the surface of oracle/ref_capi.cpp, so a small harness beside this file (ref_icp.cpp: one
translation unit that includes ref_capi.cpp unmodified and adds one extern "C" function) is compiled with the flags of oracle/Makefile's ``ref``
target into a TEMPORARY directory.  The nearest-neighbour search behind it is the shim's KdTreeFLANN -- a brute-force float32 search with
lowest-index ties, not PCL's tree.

The two plane clouds come from ``synth.loop_pair`` through the numpy checker (tests/_loopreg_ref.py: BTC.cpp cannot be compiled here, so the
extraction is the checker's).  Cases:
  a  overlapping keyframes, guess off by (1.5, -1, 2) deg and (0.25, -0.2, 0.15) m: accepted
  b  the same with icp_eigval above the measured smallest eigenvalue: converged but rejected
  c  a guess so far off that twenty iterations pass without a small step: rejected
  d  a target of four planes (rows 900-903) that only three source planes are compatible with: fewer than six matches (the reference solves a
     singular system and carries NaN from there on): the accept flag is what is compared
The fixture holds arrays and a backend string only: the two float32 clouds, per case the target's row range, the initial pose, icp_eigval, the reference's
final pose and verdict, and ``checker_vs_ref`` -- the largest pose difference [m, rad] between the checker and the reference over cases a-c.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "loop_icp.npz")
REF_SRC = os.environ.get("REF_SRC", "/root/reference/VoxelSLAM/src")
CASES = ("a", "b", "c", "d")
FAR_ROT_DEG, FAR_TR = (-6.0, 26.0, 3.0), (-1.3, 1.2, 0.9)      # case c
EIGVAL_B = 600.0                                               # case b: above the ~493 of the converged match set
TARGET_D = (900, 904)                                          # case d: rows of the target kept


def inputs():
    """Clouds and hypotheses of the four cases: dict(src, tar, and per case ((first, end) target rows, pose0, icp_eigval))."""
    from tests import _loopreg_ref as R
    from voxel_slam_amd import synth
    lp = synth.loop_pair()
    tar = R.plane_cloud(lp.cloud_tar)["rows"]; src = R.plane_cloud(lp.cloud_cur)["rows"]
    Rt, tt = synth.unpack_poses(lp.pose_true[None])
    far = synth.pack_poses((Rt[0] @ synth.rodrigues(np.deg2rad(np.asarray(FAR_ROT_DEG))))[None], (tt[0] + np.asarray(FAR_TR))[None])[0]
    full = (0, tar.shape[0])
    cases = dict(a=(full, lp.pose_guess, 14.0), b=(full, lp.pose_guess, EIGVAL_B), c=(full, far, 14.0), d=(TARGET_D, lp.pose_guess, 14.0))
    return dict(src=src, tar=tar, cases=cases, pose_true=lp.pose_true)


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def case_target(g, name):
    lo, hi = (int(v) for v in g[f"{name}_tar_range"])
    return g["tar"][lo:hi]


def compile_harness(outdir):
    so = os.path.join(outdir, "libref_icp.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O3", "-std=c++14", "-fPIC", "-pthread", "-w", "-I", os.path.join(ROOT, "oracle", "shim"), "-I", os.path.join(ROOT, "oracle"),
                           "-I", REF_SRC, "-shared", "-o", so, os.path.join(HERE, "ref_icp.cpp")])
    return so


def load_reference(so):
    L = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    L.vxr_icp_normal.argtypes = [C.c_int64, f32p, C.c_int64, f32p, f64p, C.c_double]
    L.vxo_backend.restype = C.c_char_p
    return L, L.vxo_backend().decode()


def ref_icp(L, src, tar, pose, icp_eigval):
    src = np.ascontiguousarray(src, dtype=np.float32); tar = np.ascontiguousarray(tar, dtype=np.float32)
    P = np.array(pose, dtype=np.float64).reshape(12).copy()
    ok = L.vxr_icp_normal(src.shape[0], src, tar.shape[0], tar, P, float(icp_eigval))
    return P, int(ok)


def build(L, backend):
    from tests import _loopreg_ref as R
    inp = inputs()
    out = dict(backend=backend, src=inp["src"], tar=inp["tar"], pose_true=inp["pose_true"])
    worst = np.zeros(2)
    for name in CASES:
        (lo, hi), pose0, eigval = inp["cases"][name]
        P, ok = ref_icp(L, inp["src"], inp["tar"][lo:hi], pose0, eigval)
        out[f"{name}_tar_range"] = np.array([lo, hi], dtype=np.int64); out[f"{name}_pose0"] = np.asarray(pose0); out[f"{name}_icp_eigval"] = np.float64(eigval)
        out[f"{name}_accept"] = np.int64(ok)
        if name != "d":                                  # the reference's pose of case d is NaN
            out[f"{name}_pose"] = P
            c = R.icp(inp["src"], inp["tar"][lo:hi], pose0, icp_eigval=eigval)
            worst = np.maximum(worst, R.pose_diff(c["pose"], P))
    out["checker_vs_ref"] = worst
    return out


if __name__ == "__main__":
    if not os.path.exists(os.path.join(REF_SRC, "loop_refine.hpp")):
        sys.exit(f"{REF_SRC} is not present: the golden is generated where the reference is")
    with tempfile.TemporaryDirectory() as td:
        L, backend = load_reference(compile_harness(td))
        d = build(L, backend)
    np.savez_compressed(FIXTURE, **d)
    print(os.path.getsize(FIXTURE), "bytes;", d["src"].shape[0], "source and", d["tar"].shape[0], "target planes; accept", [int(d[f"{c}_accept"]) for c in CASES],
          "; checker vs reference", d["checker_vs_ref"])
