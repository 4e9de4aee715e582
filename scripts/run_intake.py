"""Driver messages in, end to end and timed (vxba_intake_*, vxba.ScanIntake, front.ScanIntake, OdometryFront.step_message), next to the numpy checker.

    python scripts/run_intake.py [--profile] [--out profiles/intake/intake.json] [--reps 9]
    python scripts/run_intake.py --profile --only velodyne_yaw_30000x22 --out profiles/intake/intake_yaw.json

Three messages built from synth.make_raw_odometry_step on an 800-root plane map and packed by synth.make_driver_message: a Livox-like one of 24 000 x 19
bytes, an Ouster-like one of 131 072 x 48 bytes and a 100 000-point one at step 22 (time f32 at 18).  Each goes through front.ScanIntake.push and
OdometryFront.step_message; the same bytes through the checker (tests/_intake_ref.py) on the CPU and OdometryFront.step on its arrays next to it, and
the two must agree byte for byte.
A fourth message, velodyne_yaw_30000x22, is a clockwise 16-ring scan of 30 000 points at step 22 pushed twice: with its time field filled (the AS_IS
route) and with the field zero under front.ScanIntake(yaw_times=True) (vxba_intake_push_yaw, checked against tests/_intake_yaw_ref.py): the stage
times of the two routes on the same points, side by side.
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
from tests import _intake_yaw_cases as YC  # noqa: E402
from tests import _intake_yaw_ref as YR  # noqa: E402
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


YAW_NAME, YAW_POINTS, YAW_PFN, YAW_BLIND, YAW_OMEGA = "velodyne_yaw_30000x22", 30_000, 1, 1.0, 3610.0


def run_yaw(reps, profile):
    """The yaw-timed route next to the AS_IS route on the same points: push only (what differs), the stage times of each."""
    lidar, lay, _ = MESSAGES["step22_100000"]
    x, y, z = YC.ring_scan(YAW_POINTS, 30.0, 0.3, 77)
    xyz = np.stack([x, y, z], axis=1)
    with_times = synth.make_driver_message(xyz, np.linspace(0.0, 0.0997, YAW_POINTS).astype(np.float32), lay)
    zero_times = synth.make_driver_message(xyz, np.zeros(YAW_POINTS, dtype=np.float32), lay)
    t0 = time.perf_counter()
    want_yaw = YR.replay(x, y, z, YAW_PFN, YAW_BLIND, YAW_OMEGA)
    t_chk = time.perf_counter() - t0
    want_as_is = R.process(with_times, lay, lidar, YAW_PFN, YAW_BLIND, 100.0)
    out = dict(points=YAW_POINTS, point_step=int(lay.point_step), message_bytes=len(zero_times), omega_l=YAW_OMEGA, replay_cpu_ms=1e3 * t_chk)
    fi = front.ScanIntake(lidar, lay, point_filter_num=YAW_PFN, blind=YAW_BLIND, yaw_times=True, omega_l=YAW_OMEGA)
    fi.dev.set_profiling(profile)
    for route, data, want in (("as_is", with_times, want_as_is), ("yaw", zero_times, want_yaw)):
        rows = []
        for r in range((reps + 2) if profile else 1):
            t = time.perf_counter()
            fi.push(data, 100.0)
            wall = 1e3 * (time.perf_counter() - t)
            if profile and r >= 2:
                rows.append((wall, fi.dev.stage_times()))
        xyz_g, toff_g = fi.read()
        same = bool(fi.route == ("yaw" if route == "yaw" else "push") and fi.record["record"].tobytes() == want["record"].tobytes() and xyz_g.tobytes() == want["xyz"].tobytes() and
                    toff_g.tobytes() == want["toff"].tobytes())
        stats = fi.dev.stats()
        res = dict(n_out=int(fi.record["n_out"]), matches_checker=same, launches=stats["launches"], host_waits=stats["waits"])
        if route == "yaw":
            res["yaw_info"] = fi.dev.yaw_info()
        if profile:
            med = lambda k: float(np.median([x[1][k] for x in rows]))
            res.update(reps=reps, device_ms=dict(upload_decode_filter=med("decode"), sort=med("sort"), push=med("push")), wall_ms=dict(push=float(np.median([x[0] for x in rows]))))
        else:
            res.update(device_ms="not measured", wall_ms="not measured")
        print(f"intake {YAW_NAME} / {route}: {YAW_POINTS} points -> {res['n_out']} out; equal to the checker byte for byte: {same}")
        if not same:
            raise SystemExit("the device and the checker disagree")
        out[route] = res
    fi.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intake", "intake.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None, help="one of " + ", ".join([*MESSAGES, YAW_NAME]))
    a = ap.parse_args()
    pm = synth.make_plane_map(n_roots=800, extent=6, seed=17)
    res = {name: run_one(name, pm, a.reps, a.profile) for name in MESSAGES if a.only in (None, name)}
    if a.only in (None, YAW_NAME):
        res[YAW_NAME] = run_yaw(a.reps, a.profile)
    print("intake: " + json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
