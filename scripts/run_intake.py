"""Driver messages in, end to end and timed (vxba_intake_*, vxba.ScanIntake, front.ScanIntake, OdometryFront.step_message), next to the numpy checker.

    python scripts/run_intake.py [--profile] [--out profiles/intake/intake.json] [--reps 9]

Three messages built from synth.make_raw_odometry_step on an 800-root plane map and packed by synth.make_driver_message: a Livox-like one of 24 000 x 19
bytes, an Ouster-like one of 131 072 x 48 bytes and a 100 000-point one at step 22 (time f32 at 18).  Each goes through front.ScanIntake.push and
OdometryFront.step_message; the same bytes through the checker (tests/_intake_ref.py) on the CPU and OdometryFront.step on its arrays next to it, and
the two must agree byte for byte.
--profile: warm-up first, then the median of --reps of: the device time of upload + decode / filter, of the sort and of the whole push (events on the
handle's stream), the wall clock of push, of step_message behind it and of step on the decoded arrays; next to them the CPU time of the checker's
loop-faithful decode and of a vectorised numpy decode of the same message (what a host front end would pay before step).  No threshold: a first
measurement.  Every repetition restarts from the same filter history, so each processes the same scan.
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

from tests import _imuekf_ref as E  # noqa: E402
from tests import _intake_ref as R  # noqa: E402
from voxel_slam_amd import front, synth, vxba  # noqa: E402

MESSAGES = {
    "livox_24000x19": (front.LIVOX, front.layout_livox(), 24_000),
    "ouster_131072x48": (front.OUSTER, front.layout_from_fields([("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 16, 7), ("t", 20, 6), ("reflectivity", 24, 4), ("ring", 26, 2),
                                                                 ("ambient", 28, 4), ("range", 32, 6)], 48, front.OUSTER), 131_072),
    "step22_100000": (front.VELODYNE, front.layout_from_fields([("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 12, 7), ("ring", 16, 4), ("time", 18, 7)], 22, front.VELODYNE),
                      100_000),
}
BLIND, PFN = 0.01, 1


def numpy_decode(data, lay, lidar):
    """A vectorised host decode of the same message (no per-point loop): what a numpy front end would do before OdometryFront.step."""
    x, y, z, t = R.unpack(data, lay)
    cur = t.astype(np.float32) / np.float32(1e9) if lidar in (front.LIVOX, front.OUSTER) else t.astype(np.float32)
    s = (x * x + y * y) + z * z
    keep = (s.astype(np.float64) > BLIND) & np.isfinite(s) & np.isfinite(cur) & (cur.astype(np.float64) <= 0.11)
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(cur[idx], kind="stable")]
    return np.stack([x[idx], y[idx], z[idx]], axis=1), cur[idx]


def run_one(name, pm, reps, profile):
    lidar, lay, points = MESSAGES[name]
    ext = E.ext_default()
    opt = E.filter_options(dict())
    ref = E.ImuEkfRef(**opt)
    st, _ = E.initialise(ref, t_end=100.0, lag=E.LAG)
    step = synth.make_raw_odometry_step(pm, ref.last_imu, 100.0, st[21:24], scale_gravity=ref.scale_gravity, n_points=points, K=20, ext=ext)
    data = synth.make_driver_message(step.scan[0], synth.raw_times(step.scan[1], lay), lay)
    t0 = time.perf_counter()
    want = R.process(data, lay, lidar, PFN, BLIND, step.beg_time)
    t_chk = time.perf_counter() - t0
    t0 = time.perf_counter()
    vx, vt = numpy_decode(data, lay, lidar)
    t_np = time.perf_counter() - t0
    assert vx.tobytes() == want["xyz"].tobytes() and vt.tobytes() == want["toff"].tobytes()
    end = step.beg_time + float(want["toff"][-1])                # sync_packages: pcl_end_time = beg + the last curvature
    rows = []
    with vxba.ImuEkf(vxba.ImuEkfParams.make(**opt)) as ea, vxba.ImuEkf(vxba.ImuEkfParams.make(**opt)) as eb:
        la = vxba.LioEstimator(pm.voxel_size, pm.max_layer); la.map_update(*pm.args())
        lb = vxba.LioEstimator(pm.voxel_size, pm.max_layer); lb.map_update(*pm.args())
        fa, fb = front.OdometryFront(ea, la, ext, down_size=0.1), front.OdometryFront(eb, lb, ext, down_size=0.1)
        fi = front.ScanIntake(lidar, lay, point_filter_num=PFN, blind=BLIND)
        fi.dev.set_profiling(profile)
        for r in range((reps + 2) if profile else 1):
            for e in (ea, eb):
                e.clear(); E.initialise(e, t_end=100.0, lag=E.LAG)
            w = {}
            t = time.perf_counter()
            beg = fi.push(data, step.beg_time)
            w["push"] = time.perf_counter() - t; t = time.perf_counter()
            rb = fb.step_message(step.state_prev, step.cov, fi, step.imus, beg, end)
            w["step_message"] = time.perf_counter() - t; t = time.perf_counter()
            ra = fa.step(step.state_prev, step.cov, (want["xyz"], want["toff"]), step.imus, beg, end)
            w["step"] = time.perf_counter() - t
            if profile and r >= 2:
                rows.append(({k: 1e3 * v for k, v in w.items()}, fi.dev.stage_times()))
        stats = fi.dev.stats()
        xyz, toff = fi.read()
        same = bool(fi.record["record"].tobytes() == want["record"].tobytes() and xyz.tobytes() == want["xyz"].tobytes() and toff.tobytes() == want["toff"].tobytes() and
                    all(ra[k].tobytes() == rb[k].tobytes() for k in ("state", "cov", "state_prop", "cov_prop", "pwld")))
        fi.close(); la.close(); lb.close()
    print(f"intake {name}: {points} points x {lay.point_step} B -> {fi.record['n_out']} out; cloud and step_message equal to the checker and to step, byte for byte: {same}; "
          f"ok {rb['ok']}, {rb['n_filtered']} filtered")
    if not same or not rb["ok"]:
        raise SystemExit("the device and the checker disagree")
    out = dict(points=points, point_step=int(lay.point_step), message_bytes=len(data), n_out=int(fi.record["n_out"]), matches_checker=same, launches=stats["launches"],
               host_waits=stats["waits"], checker_decode_cpu_ms=1e3 * t_chk, numpy_decode_cpu_ms=1e3 * t_np)
    if profile:
        med = lambda i, k: float(np.median([x[i][k] for x in rows]))
        out.update(reps=reps, device_ms=dict(upload_decode_filter=med(1, "decode"), sort=med(1, "sort"), push=med(1, "push")),
                   wall_ms=dict(push=med(0, "push"), step_message=med(0, "step_message"), push_plus_step_message=float(np.median([x[0]["push"] + x[0]["step_message"] for x in rows])),
                                step_on_decoded_arrays=med(0, "step")))
    else:
        out.update(device_ms="not measured", wall_ms="not measured")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intake", "intake.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, help="one of " + ", ".join(MESSAGES))
    a = ap.parse_args()
    pm = synth.make_plane_map(n_roots=800, extent=6, seed=17)
    res = {name: run_one(name, pm, a.reps, a.profile) for name in MESSAGES if a.only in (None, name)}
    print("intake: " + json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
