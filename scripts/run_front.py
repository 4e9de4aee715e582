"""The front of the chain end to end and timed (vxba_imuekf_*, vxba.ImuEkf, front.OdometryFront), next to the numpy checker.

    python scripts/run_front.py [--profile] [--out profiles/front/front.json] [--reps 9] [--points 100000]

One raw scan of --points points with 20 IMU messages (synth.make_raw_odometry_step on an 800-root plane map) through OdometryFront.step: raw scan + raw
IMU in, estimated state out, the scan crossing the bus once.  The same scan through the checker (tests/_imuekf_ref.py) on the CPU: state, covariance
and de-skewed floats next to it.
--profile: warm-up first, then the median of --reps of the wall clock per stage (process, filter, var_init, lio_state_estimation, pvec_update) and,
from events on the handle's stream, the device time of the de-skew (upload + kernel) and of the filter; var_init runs on the odometry handle's stream
and is timed by the host clock around a call that waits for it.  No threshold: a first measurement.  Every repetition restarts from the same filter
history (clear + the same stationary messages), so each processes the same scan.
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
from voxel_slam_amd import synth, vxba  # noqa: E402
from voxel_slam_amd.front import OdometryFront  # noqa: E402


def run(points, reps, profile):
    pm = synth.make_plane_map(n_roots=800, extent=6, seed=17)
    ext = E.ext_default()
    opt = E.filter_options(dict())
    ref = E.ImuEkfRef(**opt)
    st, _ = E.initialise(ref, t_end=100.0, lag=E.LAG)
    step = synth.make_raw_odometry_step(pm, ref.last_imu, 100.0, st[21:24], scale_gravity=ref.scale_gravity, n_points=points, K=20, ext=ext)
    t0 = time.perf_counter()
    want = ref.process(step.state_prev, step.cov, step.scan, step.imus, step.beg_time, step.end_time)
    t_chk = time.perf_counter() - t0
    walls, devs = [], []
    with vxba.ImuEkf(vxba.ImuEkfParams.make(**opt)) as ekf:
        est = vxba.LioEstimator(pm.voxel_size, pm.max_layer); est.map_update(*pm.args())
        front = OdometryFront(ekf, est, ext, down_size=0.1)
        ekf.set_profiling(profile)
        for r in range((reps + 2) if profile else 1):
            ekf.clear()
            E.initialise(ekf, t_end=100.0, lag=E.LAG)
            w = {}
            t = time.perf_counter()
            p = ekf.process(step.state_prev, step.cov, step.scan, step.imus, step.beg_time, step.end_time)
            w["process"] = time.perf_counter() - t; t = time.perf_counter()
            n_f, half = ekf.filter(front.down_size, front.min_points)
            w["filter"] = time.perf_counter() - t; t = time.perf_counter()
            d_xyz, n_d = ekf.filtered_device()
            est.var_init_device(d_xyz, n_d, ext, front.dept_err, front.beam_err)
            w["var_init"] = time.perf_counter() - t; t = time.perf_counter()
            e = est.lio_state_estimation(p["state"], p["cov"])
            w["lio_state_estimation"] = time.perf_counter() - t; t = time.perf_counter()
            est.pvec_update(e["state"], e["cov"], resident=True)
            w["pvec_update"] = time.perf_counter() - t
            if profile and r >= 2:
                walls.append({k: 1e3 * v for k, v in w.items()}); devs.append(ekf.stage_times())
        stats = ekf.stats()
        scan = ekf.read_scan()
        # once more through the class the tests pin, for the printed result
        ekf.clear(); E.initialise(ekf, t_end=100.0, lag=E.LAG)
        got = front.step(step.state_prev, step.cov, step.scan, step.imus, step.beg_time, step.end_time)
        est.close()
    ulp = E.ulp_diff32(scan, want["scan"])
    K = 20
    same = bool((np.abs(p["state"] - want["state"]) <= E.tol(K + 1, want["state"])).all() and (np.abs(p["cov"] - want["cov"]) <= E.tol(K + 1, want["cov"])).all() and ulp.max() <= 1)
    from tests._init_ref import so3_log

    def err(a, b):
        return float(np.linalg.norm(a[9:12] - b[9:12])), float(np.linalg.norm(so3_log(a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T)))
    ep, pp = err(got["state"], step.truth_end), err(got["state_prop"], step.truth_end)
    print(f"front: {points} points, {p['heads']} heads, {p['compensated']} compensated -> {n_f} filtered (half size: {half}); {int((ulp > 0).sum())} of {ulp.size} "
          f"de-skewed coordinates differ from the checker (max {int(ulp.max())} ulp); state and covariance within tolerance: {same}")
    print(f"front: ok {got['ok']}, {got['estimation']['match_num']} matches, {got['estimation']['iterations']} iterations; off the truth {ep[0]:.4f} m {ep[1]:.5f} rad "
          f"(propagated {pp[0]:.4f} m {pp[1]:.5f} rad)")
    if not same or not got["ok"] or not (ep[0] < pp[0] and ep[1] < pp[1]):
        raise SystemExit("the device and the checker disagree, or the odometry did not improve on the propagated state")
    out = dict(points=points, imu_messages=K, heads=p["heads"], filtered=n_f, half_size=bool(half), coordinates_differing=int((ulp > 0).sum()), matches_checker=same,
               launches=stats["launches"], host_waits=stats["waits"], deskew_bytes=28 * points, checker_cpu_ms=1e3 * t_chk)
    if profile:
        med = lambda rows, k: float(np.median([x[k] for x in rows]))
        out.update(reps=reps, wall_ms={k: med(walls, k) for k in walls[0]}, wall_total_ms=float(np.median([sum(x.values()) for x in walls])),
                   device_ms=dict(deskew=med(devs, "deskew"), filter=med(devs, "filter")), var_init="host clock around a call that waits for its stream (wall_ms.var_init)")
    else:
        out.update(wall_ms="not measured", device_ms="not measured")
    print("front: " + json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "front", "front.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--points", type=int, default=100_000)
    a = ap.parse_args()
    res = run(a.points, a.reps, a.profile)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
