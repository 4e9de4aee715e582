"""Corners end to end and timed (vxba_corner_*, vxba.CornerExtractor, hba.keyframe_stream(corners=...)), next to the numpy checker.

    python scripts/run_corners.py [--profile] [--out profiles/corners/corners.json] [--reps 9]

1. A ScanPose stream (synth.make_corner_revisit_stream: one scene seen twice) through hba.keyframe_stream with a corner extractor into
   hba.loop_closure: no corner is supplied by hand.  The corner sets next to the checker's (tests/_corner_ref.py), the revisit found, the edge.
2. --profile: ONE keyframe of 10 x 100 000 points, resident on the device (the keyframe builder's `full` cloud), through extract_device: wall clock
   around the call and, from events recorded on the handle's stream around the stages, the device time per stage; warm-up first, then the median of
   --reps.  P, merged planes, candidates and corners, the launch and wait counts, and the same cloud through the checker on the CPU.  A first
   measurement, not a bar.
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

from tests import _corner_ref as R  # noqa: E402
from voxel_slam_amd import hba, synth, vxba  # noqa: E402


def chain_demo():
    scans = synth.make_corner_revisit_stream(2, 3, seed=55)
    b = vxba.KeyframeBuilder(3, 1.0)
    ses = vxba.HbaSession()
    prm = vxba.LoopSearchParams(skip_near_num=-1)
    with vxba.LoopRegistration() as reg, vxba.CornerExtractor() as ce, vxba.LoopSearch(reg) as ls:
        t0 = time.perf_counter()
        got = hba.keyframe_stream(b, reg, ses, scans, corners=ce)
        t_stream = time.perf_counter() - t0
        poses = np.stack([g[1] for g in got])
        v6 = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
        results = []
        for k, g in enumerate(got):
            results.append(hba.loop_closure(g[3], k, k, poses[:k + 1], v6, ls, reg, params=prm))
        full = b.read()[0]
    ref = R.extract(full.astype(np.float64))
    loc, occ = got[-1][3]
    same = bool(np.array_equal(occ, ref["occupancy"]) and np.abs(loc - ref["locations"]).max(initial=0) < 1e-9)
    last = results[-1]
    print(f"chain: {len(scans)} scans -> {len(got)} keyframes, corners {[g[3][0].shape[0] for g in got]}; the last set equals the checker's: {same}; "
          f"{1e3 * t_stream:.1f} ms for the stream (first calls included)")
    print(f"chain: keyframe {len(got) - 1} found frame {last['search']['frame']} (score {last['search']['score']:.3f}); edges {[(e['i'], e['j']) for e in last['edges']]}")
    ses.close(); b.close()
    if not same or last["search"]["frame"] != 0 or not last["edges"]:
        raise SystemExit("the chain did not close the loop, or the device and the checker disagree")
    return dict(keyframes=len(got), corners=[int(g[3][0].shape[0]) for g in got], found_frame=int(last["search"]["frame"]), score=float(last["search"]["score"]),
                edges=len(last["edges"]), matches_checker=True, stream_ms=1e3 * t_stream)


def profile(reps):
    world = synth.make_corner_scene(seed=77, extent=50.0, n_walls=3, n_poles=120, n_boxes=30, density=300.0)[0]
    n = 100_000
    assert world.shape[0] >= 10 * n
    world = world[:10 * n]
    ident = synth.pack_poses(np.eye(3)[None], np.zeros((1, 3)))[0]
    b = vxba.KeyframeBuilder(10, 1.0)
    for k in range(10):
        pose = ident.copy(); pose[9] = 0.02 * k
        em = b.push_scan(pose, 1e-4 * np.ones(6), world[k * n:(k + 1) * n] - np.array([0.02 * k, 0.0, 0.0]))
    assert em
    info, ptrs = b.info(), b.device_ptrs()
    times, walls = [], []
    with vxba.CornerExtractor() as ce:
        ce.set_profiling(True)
        for r in range(reps + 2):
            t0 = time.perf_counter()
            nc = ce.extract_device(info["n_full"], ptrs["full"])
            w = time.perf_counter() - t0
            if r >= 2:
                walls.append(1e3 * w); times.append(ce.stage_times())
        st = ce.stats()
        cd, pl, pp = ce.candidates(), ce.planes(), ce.projection_planes()
    full = b.read()[0].astype(np.float64)
    b.close()
    t0 = time.perf_counter()
    ref = R.extract(full)
    t_chk = time.perf_counter() - t0
    same = bool(nc == ref["locations"].shape[0] and np.array_equal(cd["kept"], ref["kept"]) and st["cells"] == sum(im["cells"] for im in ref["images"] if im["valid"]))
    med = {k: float(np.median([t[k] for t in times])) for k in times[0]}
    out = dict(points=int(info["n_full"]), plane_voxels=int(pl["labels"].shape[0]), projection_planes=int(pp["used"].shape[0]), used_planes=int((pp["used"] >= 0).sum()),
               cells=st["cells"], candidates=int(cd["kept"].shape[0]), corners=int(nc), stage_ms=med, device_ms=float(sum(med.values())), wall_ms=float(np.median(walls)), launches=st["launches"],
               host_waits=st["host_waits"], bytes_d2h=st["bytes_d2h"], bytes_h2d=st["bytes_h2d"], checker_cpu_ms=1e3 * t_chk, matches_checker=same, reps=reps)
    print("profile: " + json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corners", "corners.json"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    res = dict(chain=chain_demo())
    if a.profile:
        res["profile"] = profile(a.reps)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
