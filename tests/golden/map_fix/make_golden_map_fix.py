"""Regenerates tests/golden/map_fix/map_fix_cycle.npz and map_fix_loop.npz from the reference's own code (run in a container that has /root/reference):

    python tests/golden/map_fix/make_golden_map_fix.py

The reference's fix-form ``cut_voxel`` / ``allocate_fix`` (keyframe_loading) and the map part of ``loop_update`` are not behind the surface of
oracle/ref_capi.cpp, so a small harness beside this file (ref_fixmap.cpp: one translation unit that includes ref_capi.cpp unmodified and adds four
extern "C" functions) is compiled with the flags of oracle/Makefile's ``ref`` target into a TEMPORARY directory and loaded through ``tests/_ref._load``,
so that ``LocalMapOracle`` / ``Oracle`` of tests/_oracle.py work on it unchanged.

``scenario`` below is the one driver of both sides: the generator runs it on the reference, tests/test_gpu_map_fix.py on the device map, and
tests/test_map_fix_golden_cpu.py on the reference again where it is present.  The fixture holds arrays and a backend string only.

Stages (leaf tables sorted by node id):
  fix0   scans 0-3 at their true poses, every second point, as four keyframe clouds (jour = k, no variances): roots without window or slide map
  w3..w8 scans 3-8 through cut_voxel -> recut -> 3 LM iterations -> margi -> slide (window 3, max_points 60), poses perturbed as make_golden.py does
  kf5    behind the window of scan 5: scan 1's odd points as one more keyframe (jour = 7) into a map that has subdivided nodes
  loop   the loop update: five keyframe clouds (scans 0-4 under dx o true pose, diagonal variances as voxelslam.cpp:2145-2146 builds them), the two
         scans left in the window under dx o their optimised poses, recut of every root
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

FIXTURES = (os.path.join(HERE, "map_fix_cycle.npz"), os.path.join(HERE, "map_fix_loop.npz"))     # stages fix0 .. w8 | the loop update (two files: each stays a small one)
REF_SRC = os.environ.get("REF_SRC", "/root/reference/VoxelSLAM/src")
S, WIN, PTS, SEED, EXTENT, MAX_POINTS = 9, 3, 3000, 31, 6.0, 60
TRIU = np.triu_indices(9)


def load_fixture():
    g = {}
    for p in FIXTURES:
        with np.load(p) as z:
            g.update({k: z[k] for k in z.files})
    return g


def inputs():
    """Everything both sides are fed that does not depend on a BA result."""
    from tests.test_oracle_octree import PRM, point_vars
    from voxel_slam_amd import synth
    xyz, fp, poses_gt, _ = synth.make_scans(win_size=S, pts_per_scan=PTS, extent=EXTENT, seed=synth.MASTER_SEED + 900 + SEED)
    kw = dict(PRM); kw["max_points"] = MAX_POINTS
    rng = np.random.default_rng(SEED)
    poses_in = poses_gt.copy()
    for k in range(3, S):
        poses_in[k, 9:12] += rng.normal(0, 0.01, 3)
    ang = np.deg2rad(1.0)
    dR = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]]); dp = np.array([0.04, -0.03, 0.02])
    return dict(xyz=xyz, fp=fp, poses_gt=poses_gt, poses_in=poses_in, var=point_vars(xyz.shape[0], SEED), kw=kw, dR=dR, dp=dp)


def corrected(pose, dR, dp):
    """dx o pose (voxelslam.cpp:1141-1143)."""
    R = pose[:9].reshape(3, 3).T
    q = pose.copy(); q[:9] = (dR @ R).T.reshape(-1); q[9:12] = dR @ pose[9:12] + dp
    return q


def keyframe_vars(k, n):
    """Diagonal variances of a keyframe cloud (`pv.var(j, j) = ap.normal[j]`, voxelslam.cpp:2145-2146)."""
    d = np.abs(np.random.default_rng(100 + k).normal(0, 1e-4, (n, 3)))
    v = np.zeros((n, 3, 3)); v[:, 0, 0] = d[:, 0]; v[:, 1, 1] = d[:, 1]; v[:, 2, 2] = d[:, 2]
    return v


def scenario(m, f, optimise, inp, on_stage, on_factor=None, fixed=None, steps=4):
    """Drives map ``m`` (cut_voxel_fix / cut_voxel / recut / margi / slide / loop_update) and factor ``f`` through the stages.  ``fixed``: the stored
    ``kf_poses`` / ``loop_poses`` of a fixture (fed as they are); None computes them (the generator)."""
    from tests.test_oracle_octree import to_world
    xyz, fp, var, gt = inp["xyz"], inp["fp"], inp["var"], inp["poses_gt"]
    sl = lambda k: slice(fp[k], fp[k + 1])
    for k in range(4):
        m.cut_voxel_fix(np.ascontiguousarray(to_world(gt[k], xyz[sl(k)])[::2]), None, float(k))
    on_stage("fix0", None)
    xb, wc = [], 0
    for k in range(3, S):
        xb.append(inp["poses_in"][k].copy()); wc += 1
        f.clear()
        m.cut_voxel(wc - 1, xyz[sl(k)], var[sl(k)], to_world(xb[-1], xyz[sl(k)]))
        m.recut(wc, np.stack(xb), f)
        if wc < WIN:
            continue
        if on_factor:
            on_factor(k)
        lm = optimise(f, np.stack(xb))
        m.margi(wc, lm["poses"], f)
        m.slide(1)
        xb = [p for p in lm["poses"][1:]]; wc -= 1
        on_stage(f"w{k}", lm)
        if k == 5:
            if steps < 3:
                return None
            m.cut_voxel_fix(np.ascontiguousarray(to_world(gt[1], xyz[sl(1)])[1::2]), None, 7.0)
            on_stage("kf5", None)
    if steps < 4:
        return None
    if fixed is None:
        fixed = dict(kf_poses=np.stack([corrected(gt[k], inp["dR"], inp["dp"]) for k in range(5)]), loop_poses=np.stack([corrected(p, inp["dR"], inp["dp"]) for p in xb]))
    clouds = [np.ascontiguousarray(to_world(fixed["kf_poses"][k], xyz[sl(k)])[::2]) for k in range(5)]
    cvars = [keyframe_vars(k, c.shape[0]) for k, c in enumerate(clouds)]
    base = S - len(xb)
    m.loop_update(clouds, cvars, fixed["loop_poses"], [(xyz[sl(base + i)], var[sl(base + i)]) for i in range(len(xb))])
    on_stage("loop", None)
    return fixed


# ---- the reference behind the calls `scenario` makes -------------------------------------------------------------------------------------------
def compile_harness(outdir):
    so = os.path.join(outdir, "libref_fixmap.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O3", "-std=c++14", "-fPIC", "-pthread", "-w", "-I", os.path.join(ROOT, "oracle", "shim"), "-I", os.path.join(ROOT, "oracle"),
                           "-I", REF_SRC, "-shared", "-o", so, os.path.join(HERE, "ref_fixmap.cpp")])
    return so


def load_reference(so):
    from tests import _ref
    mod = _ref._load("tests._fixmap_backend", so, "ref")
    if mod is None:
        raise RuntimeError("the harness library does not load")
    L = mod.lib()
    L.vxo_backend.restype = C.c_char_p
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    raw = C.CDLL(so)
    raw.vxr_localmap_cut_voxel_fix.argtypes = [C.c_void_p, C.c_int64, f64p, C.c_void_p, C.c_double]
    raw.vxr_localmap_clear.argtypes = [C.c_void_p]
    raw.vxr_localmap_cut_voxel_single.argtypes = [C.c_void_p, C.c_int, C.c_int64, f64p, f64p, f64p]
    raw.vxr_localmap_recut_all.argtypes = [C.c_void_p, C.c_int, f64p]
    return mod, raw, L.vxo_backend().decode()


def reference_map(mod, raw, **kw):
    """LocalMapOracle of the harness library with the three calls it lacks."""
    m = mod.LocalMapOracle(win_size=WIN, **kw)
    colmajor = lambda v: np.ascontiguousarray(np.transpose(np.asarray(v, dtype=np.float64).reshape(-1, 3, 3), (0, 2, 1))).reshape(-1, 9)

    def cut_voxel_fix(pnt, v=None, jour=0.0):
        pnt = np.ascontiguousarray(pnt, dtype=np.float64).reshape(-1, 3)
        vv = colmajor(v) if v is not None else None
        raw.vxr_localmap_cut_voxel_fix(m._h, pnt.shape[0], pnt, vv.ctypes.data_as(C.c_void_p) if vv is not None else None, float(jour))

    def loop_update(clouds, cvars, poses, scans):
        raw.vxr_localmap_clear(m._h)
        for c, v in zip(clouds, cvars):
            cut_voxel_fix(c, v, 0.0)
        for i, (pnt, v) in enumerate(scans):
            pnt = np.ascontiguousarray(pnt, dtype=np.float64).reshape(-1, 3)
            raw.vxr_localmap_cut_voxel_single(m._h, i, pnt.shape[0], pnt, colmajor(v), np.ascontiguousarray(poses[i], dtype=np.float64))
        raw.vxr_localmap_recut_all(m._h, len(scans), np.ascontiguousarray(poses, dtype=np.float64))

    m.cut_voxel_fix, m.loop_update = cut_voxel_fix, loop_update
    return m


def table(lv, stage):
    """What the fixture keeps of a leaf table.  The loop stage adds the window clusters and cov_add (upper triangle: the matrix is symmetric) of the leaves
    that have a window; kf5 differs from w5 in the loaded points only, so it keeps the fix side."""
    o = np.argsort(lv["node_id"], kind="stable")
    out = {"node_id": lv["node_id"][o], "pcr_fix": lv["pcr_fix"][o], "pcr_add": lv["pcr_add"][o]}
    for key in ("layer", "isexist", "is_plane", "has_sw", "in_slide"):
        out[key] = lv[key][o].astype(np.uint8)
    for key in ("last_num", "n_point_fix"):
        out[key] = lv[key][o].astype(np.int32)
    out["n_points"] = lv["n_points"][o].astype(np.int32)
    if stage != "kf5":
        out["eig_val"] = lv["eig_val"][o]
    if stage == "loop":
        out["pcrs_local"] = lv["pcrs_local"][o]
        out["cov_add_triu"] = lv["cov_add"][o][lv["has_sw"][o]][:, TRIU[0], TRIU[1]]
    return out


def build(mod, raw, backend, steps=4):
    inp = inputs()
    m = reference_map(mod, raw, **inp["kw"])
    f = mod.Oracle(WIN)
    out = dict(backend=backend, poses_in=inp["poses_in"], dR=inp["dR"], dp=inp["dp"])

    def on_stage(tag, lm):
        for key, v in table(m.leaves(), tag).items():
            out[f"{tag}_{key}"] = v
        if lm is not None:
            out[f"{tag}_poses"] = lm["poses"]; out[f"{tag}_trace"] = lm["trace"]

    def on_factor(k):
        lv = m.leaves()
        out[f"w{k}_factor_ids"] = np.sort(lv["node_id"][lv["opt_state"] >= 0])

    fixed = scenario(m, f, lambda ff, xs: ff.damping_iter(xs, max_iter=3, thd_num=2), inp, on_stage, on_factor, steps=steps)
    if fixed is not None:
        out.update(fixed)
    return out


if __name__ == "__main__":
    if not os.path.exists(os.path.join(REF_SRC, "voxel_map.hpp")):
        sys.exit(f"{REF_SRC} is not present: the golden is generated where the reference is")
    with tempfile.TemporaryDirectory() as td:
        mod, raw, backend = load_reference(compile_harness(td))
        d = build(mod, raw, backend)
    loop_keys = [k for k in d if k.startswith("loop_") or k == "kf_poses"]
    np.savez_compressed(FIXTURES[1], backend=d["backend"], **{k: d[k] for k in loop_keys})
    np.savez_compressed(FIXTURES[0], **{k: v for k, v in d.items() if k not in loop_keys})
    lp = d["loop_layer"]
    print([os.path.getsize(p) for p in FIXTURES], "bytes;", d["fix0_node_id"].size, "roots after step 1,", d["w5_node_id"].size, "->", d["kf5_node_id"].size, "leaves at step 3,",
          d["loop_node_id"].size, "leaves /", int(d["loop_is_plane"].sum()), "planes after the loop update,", int(((lp > 0) & (d["loop_pcr_fix"][:, 9] > 0)).sum()), "children with loaded points")
