"""The loop hand-back, timed: the corridor revisit of scripts/run_loop_search.py carried through the keyframe archive to a rebuilt local map on the device
route (vxba_kfarchive_map_loop -> vxba_map_loop_update_device), next to the host route that script uses today (numpy multiplies every keyframe cloud by
its pose, LocalMap.loop_update uploads float64 points and variances).

    python scripts/run_handback.py [--profile] [--out profiles/handback] [--keyframes 41] [--radius 25]

Two shapes of the same rebuild, both routes each, on the same optimised poses:
  all_keyframes   every keyframe as one cloud, no variances -- what run_loop_search.py feeds the map
  upstream        the last five keyframes, cumulative, with their variance columns -- map_loop as the reference writes it (voxelslam.cpp:2131-2150)
Per route: wall milliseconds (host synchronisation included) of the transform and of the map rebuild, launches and host waits of the transform, bytes sent
up; the two maps' leaf tables are compared byte for byte.  --profile: medians of 9 (otherwise of 3) written to <out>/handback.json.
A first measurement, no threshold: records, not bars."""
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
    pass

import numpy as np  # noqa: E402

from tests import _loopsearch_cases as K  # noqa: E402
from voxel_slam_amd import hba, vxba  # noqa: E402


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def optimised_poses(a):
    """The session of run_loop_search.py up to the pose graph: (keyframe clouds (n, 3) float64 in their own frames, poses after the loop closed, chain record)."""
    ses = K.session(5, True, n_keyframes=a.keyframes, radius=a.radius, n_landmarks=int(190 * (a.keyframes + 1) / 26 * 1.25), skip_near_num=a.skip)
    prm = vxba.LoopSearchParams(skip_near_num=a.skip)
    kfs = ses["keyframes"]
    cur = len(kfs) - 1
    with vxba.LoopRegistration() as reg, vxba.LoopSearch(reg) as ls:
        clouds = []
        for k, (loc, occ, rows) in enumerate(kfs):
            clouds.append(reg.add_cloud(rows))
            ls.describe(loc, occ, prm)
            if k < cur:
                ls.search(clouds[k], prm)
                ls.add(clouds[k])
        poses = K.pose_records(ses["R"], ses["p"])
        poses[:, 10] += 0.01 * np.arange(len(kfs))                                         # odometry drift
        v6 = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
        loc, occ, _ = kfs[cur]
        out = hba.loop_closure((loc, occ), clouds[cur], cur, poses, v6, ls, reg, params=prm, add=True)
    chain = dict(found_frame=out["search"]["frame"], edges=len(out["edges"]))
    after = out["poses"] if out["edges"] else poses
    return [np.ascontiguousarray(rows[:, :3], dtype=np.float64) for _, _, rows in kfs], poses, after, chain


def same_leaves(a, b):
    return all(np.array_equal(v, b[k]) for k, v in a.items() if isinstance(v, np.ndarray))


def host_clouds(xyzv, poses, first, cumulative, with_var):
    """What the caller of LocalMap.loop_update does today: every cloud times its pose in numpy (and the variance diagonals widened)."""
    world, var, tem_w, tem_v = [], [], [], []
    for k in range(first, len(xyzv)):
        P, x = poses[k], xyzv[k][:, :3].astype(np.float64)
        w = np.stack([((P[i] * x[:, 0] + P[3 + i] * x[:, 1]) + P[6 + i] * x[:, 2]) + P[9 + i] for i in range(3)], axis=1)     # the sums written out: no fused `@`, so the two maps can be compared byte for byte
        v = None
        if with_var:
            v = np.zeros((w.shape[0], 3, 3))
            for j in range(3):
                v[:, j, j] = xyzv[k][:, 3 + j]
        if cumulative:
            tem_w.append(w); tem_v.append(v)
            world.append(np.concatenate(tem_w)); var.append(np.concatenate(tem_v) if with_var else None)
        else:
            world.append(w); var.append(v)
    return world, (var if with_var else None)


def run(a):
    reps = 9 if a.profile else 3
    xyz, before, after, chain = optimised_poses(a)
    rng = np.random.default_rng(5)
    xyzv = [np.concatenate([c, np.abs(rng.normal(0, 1e-4, c.shape))], axis=1).astype(np.float32) for c in xyz]
    Kn = len(xyzv)
    res = dict(keyframes=Kn, points=int(sum(c.shape[0] for c in xyzv)), chain=chain, repetitions=reps, shapes={})
    with vxba.KeyframeArchive() as ar:
        for k, c in enumerate(xyzv):
            ar.add(k, before[k], 0.1 * k, c)
        ar.set_poses(after)
        for name, init, cumulative, with_var in (("all_keyframes", Kn, False, False), ("upstream", 5, True, True)):
            if init > 64:
                continue
            first = max(0, Kn - init)
            md, mh = vxba.LocalMap(win_size=10), vxba.LocalMap(win_size=10)
            dev, host = [], []
            for rep in range(reps + 1):                                                     # the first repetition (allocations, module load) is left out
                ml, t_tr = ms(lambda: ar.map_loop(init, cumulative))
                st = ar.stats()
                _, t_map = ms(lambda: md.loop_update_device(ml["cloud_ptr"], ml["pnt_world"], ml["var"] if with_var else 0))
                (world, var), t_np = ms(lambda: host_clouds(xyzv, after, first, cumulative, with_var))
                _, t_up = ms(lambda: mh.loop_update(world, var))
                if rep:
                    dev.append((t_tr, t_map)); host.append((t_np, t_up))
            n_out = int(ml["cloud_ptr"][-1])
            med = lambda rows, j: float(np.median([r[j] for r in rows]))
            res["shapes"][name] = dict(
                init_num=init, cumulative=cumulative, variances=with_var, clouds=len(ml["cloud_ptr"]) - 1, output_points=n_out,
                device_route=dict(transform_ms=med(dev, 0), map_rebuild_ms=med(dev, 1), total_ms=float(np.median([r[0] + r[1] for r in dev])), launches=st["launches"],
                                  host_waits=st["host_waits"], bytes_h2d=st["bytes_h2d"]),
                host_route=dict(transform_ms=med(host, 0), map_rebuild_ms=med(host, 1), total_ms=float(np.median([r[0] + r[1] for r in host])), launches=0, host_waits=0,
                                bytes_h2d=n_out * (24 + (72 if with_var else 0))),
                leaves=int(md.leaves()["node_id"].size), leaf_tables_identical=bool(same_leaves(md.leaves(), mh.leaves())), map=md.counts())
            md.close(); mh.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for handback.json (default with --profile: profiles/handback)")
    ap.add_argument("--keyframes", type=int, default=41)
    ap.add_argument("--radius", type=float, default=25.0)
    ap.add_argument("--skip", type=int, default=30)
    ap.add_argument("--profile", action="store_true", help="medians of 9 and the JSON file")
    a = ap.parse_args()
    res = run(a)
    out = a.out or (os.path.join(ROOT, "profiles", "handback") if a.profile else None)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "handback.json"), "w") as fh:
            json.dump(res, fh, indent=1, default=float)
    print(json.dumps(res, default=float))


if __name__ == "__main__":
    main()
