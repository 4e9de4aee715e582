"""Keyframes end to end and timed (vxba_keyframe_*, hba.keyframe_stream), next to the numpy checker.

    python scripts/run_keyframes.py [--profile] [--out profiles/keyframes/keyframes.json] [--reps 9] [--scans 30] [--pts 4000]

1. A ScanPose stream (synth.make_scanpose_stream: a stationary stretch, an empty scan) scan by scan through the keyframe builder into the loop
   registration handle and a hierarchical-BA session, device to device; the same stream through the checker (tests/_keyframe_ref.py): ids, jour and
   cloud sizes side by side, the last keyframe compared bit for bit.
2. --profile: ONE keyframe of 10 x 100 000 points.  The scans are resident on the device (the device-pointer route); per repetition nine buffering
   pushes, then the emitting one is timed: wall clock around the call (its single host wait included) and, from events recorded on the handle's
   stream between the stages, assembly / sort + group / filter.  Warm-up first, then the median of --reps.  Next to it the host-pointer route
   (the emitting push's 4.8 MB upload included) and the same keyframe through the checker on the CPU.  A first measurement, not a bar.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (its HIP runtime must enter the process before libvxba.so, as in tests/conftest.py)
except Exception:
    torch = None

import numpy as np  # noqa: E402

from tests import _keyframe_ref as R  # noqa: E402
from voxel_slam_amd import hba, synth, vxba  # noqa: E402


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def stream_demo(n_scans, pts, win):
    st = synth.make_scanpose_stream(n_scans, pts, win)
    ref = R.KeyframeRef(win, 1.0)
    t0 = time.perf_counter()
    kfs = [ref.keyframe for s in st if ref.push_scan(*s)]
    t_chk = time.perf_counter() - t0
    b = vxba.KeyframeBuilder(win, 1.0)
    ses = vxba.HbaSession()
    with vxba.LoopRegistration() as reg:
        t0 = time.perf_counter()
        got = hba.keyframe_stream(b, reg, ses, st)
        t_gpu = time.perf_counter() - t0
        planes = [reg.cloud_size(k) for k in range(reg.num_clouds())]
    full, down = b.read()
    same = bool(np.array_equal(bits(full), bits(kfs[-1]["full"])) and np.array_equal(bits(down), bits(kfs[-1]["down"])))
    ids_ok = [g[0] for g in got] == [k["id"] for k in kfs] and all(g[2] == k["jour"] for g, k in zip(got, kfs))
    print(f"stream: {n_scans} scans of {pts} points, win_size {win}: {len(got)} keyframes, ids {[g[0] for g in got]}, jour {got[-1][2]:.3f} m; "
          f"full {full.shape[0]} -> down {down.shape[0]} points; plane clouds {planes}")
    print(f"stream: ids and jour equal the checker's: {ids_ok}; last keyframe bit-identical: {same}; {1e3 * t_gpu:.1f} ms on the GPU (first calls included), checker {1e3 * t_chk:.0f} ms")
    ses.close(); b.close()
    if not (same and ids_ok):
        raise SystemExit("the device and the checker disagree")
    return dict(scans=n_scans, pts_per_scan=pts, win_size=win, keyframes=len(got), plane_cloud_sizes=planes, matches_checker=True, gpu_ms=1e3 * t_gpu, checker_ms=1e3 * t_chk)


def profile(reps, win=10, pts=100_000):
    st = synth.make_scanpose_stream(win, pts, win, room=(40.0, 30.0, 6.0), stationary=False, empty_scan=-1)
    N = win * pts
    dev = [(torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()) for p, v in zip(st.points, st.variances)]
    b = vxba.KeyframeBuilder(win, 1.0)
    b.set_profiling(True)

    def one(route):
        b.clear()
        for k in range(win - 1):
            if route == "device":
                b.push_scan_device(st.poses[k], st.v6[k], pts, dev[k][0].data_ptr(), dev[k][1].data_ptr())
            else:
                b.push_scan(st.poses[k], st.v6[k], st.points[k], st.variances[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "device":
            em = b.push_scan_device(st.poses[-1], st.v6[-1], pts, dev[-1][0].data_ptr(), dev[-1][1].data_ptr())
        else:
            em = b.push_scan(st.poses[-1], st.v6[-1], st.points[-1], st.variances[-1])
        dt = 1e3 * (time.perf_counter() - t0)
        assert em
        return dt, b.stage_times(), b.stats()

    out = {}
    for route in ("device", "host"):
        for _ in range(3):
            one(route)
        runs = [one(route) for _ in range(reps)]
        med = lambda f: float(np.median([f(r) for r in runs]))
        out[route] = dict(emitting_push_ms=med(lambda r: r[0]), assembly_ms=med(lambda r: r[1]["assembly"]), sort_group_ms=med(lambda r: r[1]["sort_group"]),
                          filter_ms=med(lambda r: r[1]["filter"]), push_ms_min=float(min(r[0] for r in runs)), push_ms_max=float(max(r[0] for r in runs)), stats=runs[-1][2])
    info = b.info()
    full, down = b.read()
    t0 = time.perf_counter()
    q, v, rfull = R.assemble(list(st.poses), st.points, st.variances)
    t_asm = time.perf_counter() - t0
    t0 = time.perf_counter()
    rdown, _, counts = R.down_sampling_pvec(q, v, 0.1)
    t_flt = time.perf_counter() - t0
    same = bool(np.array_equal(bits(full), bits(rfull)) and np.array_equal(bits(down), bits(rdown)))
    nd = info["n_down"]
    # algorithmic bytes per stage: assembly reads 48 B per point (body point + variance diagonal) and writes 12 (full) + 48 (row) + 8 (key) + 4 (index);
    # the filter reads 4 + 48 B per point and 4 per voxel, writes 24 + 12 per voxel; the sort moves 12 B per point per pass (rocPRIM decides the passes)
    out.update(points=N, voxels=nd, max_points_per_voxel=int(counts.max()), bit_identical_to_checker=same, checker_assembly_ms=1e3 * t_asm, checker_filter_ms=1e3 * t_flt,
               bytes=dict(assembly=N * (48 + 72), filter=N * 52 + nd * 40, sort_pair_bytes_per_pass=N * 24), reps=reps)
    b.close()
    d = out["device"]
    print(f"keyframe of {win} x {pts} points -> {nd} voxels (largest {counts.max()} points), bit-identical to the checker: {same}")
    print(f"device route: emitting push {d['emitting_push_ms']:.3f} ms (min {d['push_ms_min']:.3f}, max {d['push_ms_max']:.3f}); assembly {d['assembly_ms']:.3f}, sort + group {d['sort_group_ms']:.3f}, "
          f"filter {d['filter_ms']:.3f} ms; {d['stats']['launches']} launches, {d['stats']['host_waits']} host wait")
    print(f"host route: emitting push {out['host']['emitting_push_ms']:.3f} ms; checker on the CPU: assembly {1e3 * t_asm:.0f} ms, filter {1e3 * t_flt:.0f} ms")
    if not same:
        raise SystemExit("the device and the checker disagree")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scans", type=int, default=30)
    ap.add_argument("--pts", type=int, default=4000)
    ap.add_argument("--win", type=int, default=10)
    a = ap.parse_args()
    res = dict(stream=stream_demo(a.scans, a.pts, a.win))
    if a.profile:
        if torch is None or not torch.cuda.is_available():
            raise SystemExit("--profile needs the GPU: a timing taken anywhere else says nothing")
        res["keyframe_10x100k"] = profile(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
