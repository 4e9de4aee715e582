"""Regenerates tests/golden/keyframe/keyframe.npz from the reference's own down_sampling_pvec (run where the reference's sources are present):

    python tests/golden/keyframe/make_golden_keyframe.py

The keyframe merge (voxelslam.cpp:1944-1955) lives inside thd_loop_closure and is not behind the surface of oracle/ref_capi.cpp, so a small harness
beside this file (ref_keyframe.cpp: one translation unit that includes ref_capi.cpp unmodified, restates that loop on the shim's Eigen types and
calls the reference's down_sampling_pvec, voxel_map.hpp:24-65) is compiled with the flags of oracle/Makefile's ``ref`` target into a TEMPORARY directory.

One keyframe: ``synth.make_scanpose_stream(3, 700, 3)`` without the stationary stretch and the empty scan -- three scans of 700 points on the walls
of a 3 x 3 x 2 m room around the origin, so both signs of every coordinate occur and about a third of the 0.1 m voxels hold two or more points.
The fixture holds arrays and a backend string only: the three poses and v6, the scan offsets, body points and covariances, and the reference's
``full`` (N x 3 float32) and ``down`` (n_down x 6 float32) with the voxel index of every down row, sorted by that index (upstream leaves the order to
its hash map).  It decides how ``delta_R pnt + delta_p`` and the mean recurrence associate; tests/_keyframe_ref.py and the device code follow it.
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

FIXTURE = os.path.join(HERE, "keyframe.npz")
REF_SRC = os.environ.get("REF_SRC", "/root/reference/VoxelSLAM/src")
WIN, PTS, VOXEL_SIZE = 3, 700, 1.0
ARRAYS = ("poses", "v6", "scan_ptr", "pnt", "var", "voxel_size", "full", "down", "down_index")


def inputs():
    from voxel_slam_amd import synth
    st = synth.make_scanpose_stream(WIN, PTS, WIN, stationary=False, empty_scan=-1)
    scan_ptr = np.concatenate([[0], np.cumsum([p.shape[0] for p in st.points])]).astype(np.int64)
    return dict(poses=st.poses, v6=st.v6, scan_ptr=scan_ptr, pnt=np.ascontiguousarray(np.concatenate(st.points)), var=np.ascontiguousarray(np.concatenate(st.variances)),
                voxel_size=np.float64(VOXEL_SIZE))


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def scans_of(g):
    """The fixture's stream as (pose, v6, points, covariances) per scan."""
    sp = g["scan_ptr"]
    return [(g["poses"][k], g["v6"][k], g["pnt"][sp[k]:sp[k + 1]], g["var"][sp[k]:sp[k + 1]]) for k in range(g["poses"].shape[0])]


def compile_harness(outdir):
    so = os.path.join(outdir, "libref_keyframe.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O3", "-std=c++14", "-fPIC", "-pthread", "-w", "-I", os.path.join(ROOT, "oracle", "shim"), "-I", os.path.join(ROOT, "oracle"),
                           "-I", REF_SRC, "-shared", "-o", so, os.path.join(HERE, "ref_keyframe.cpp")])
    return so


def load_reference(so):
    L = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    L.vxr_keyframe.argtypes = [C.c_int, f64p, i64p, f64p, f64p, C.c_double, f32p, f32p, i64p]
    L.vxr_keyframe.restype = C.c_int64
    L.vxo_backend.restype = C.c_char_p
    return L, L.vxo_backend().decode()


def build(L, backend):
    inp = inputs()
    N = inp["pnt"].shape[0]
    full = np.zeros((N, 3), np.float32); down = np.zeros((N, 6), np.float32); index = np.zeros((N, 3), np.int64)
    n = int(L.vxr_keyframe(inp["poses"].shape[0], np.ascontiguousarray(inp["poses"]).reshape(-1), inp["scan_ptr"], inp["pnt"].reshape(-1), inp["var"].reshape(-1), float(inp["voxel_size"]),
                           full.reshape(-1), down.reshape(-1), index.reshape(-1)))
    if n < 0:
        raise RuntimeError("the harness could not match the filter's rows to voxels")
    order = np.lexsort((index[:n, 2], index[:n, 1], index[:n, 0]))
    return dict(backend=backend, full=full, down=np.ascontiguousarray(down[:n][order]), down_index=np.ascontiguousarray(index[:n][order]), **inp)


if __name__ == "__main__":
    if not os.path.exists(os.path.join(REF_SRC, "voxel_map.hpp")):
        sys.exit(f"{REF_SRC} is not present: the golden is generated where the reference is")
    with tempfile.TemporaryDirectory() as td:
        L, backend = load_reference(compile_harness(td))
        d = build(L, backend)
    np.savez_compressed(FIXTURE, **d)
    print(os.path.getsize(FIXTURE), "bytes;", d["pnt"].shape[0], "points ->", d["down"].shape[0], "voxels; backend", d["backend"])
