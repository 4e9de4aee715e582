"""Times the initialisation on one GPU next to the numpy checker (tests/_init_ref.py) on the CPU.  A whole session (synth.make_init_session: raw scans
taken during the motion, raw IMU, propagated states) goes through voxel_slam_amd.init.Initializer and through the checker's driver; per push_scan the
wall time of the voxel filter, var_init, the odometry, pvec_update and the raw copy (down_sampling_close + time sort), and of motion_init its split into
de-skew, map build, LM and re-preintegration as the library measures it.  Also the scan-to-cloud odometry alone (vxba.InitOdometry): the one-step
session of the tests (6 000 scan points against a 20 000-point cloud) and a window of five scans from an empty handle.  Wall clock around calls that end in a device synchronisation; the GPU figure is the median of --repeats runs after one
warm-up, the checker runs once.  Agreement with the checker is printed beside the times (the tests assert it).
--profile: the device work once more in a child process under `rocprofv3 --kernel-trace --stats`; its per-kernel table -- the odometry's split into
search sweeps (init_sweep_kernel), EKF (lio_ekf_kernel), append and filter, and the kernels of motion_init (init_deskew_kernel, init_pointvar_kernel, the
map's and the sweeps') -- is copied next to the JSON.  First measurements: records, not bars."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (its HIP runtime must enter the process before libvxba.so, as in tests/conftest.py)
except Exception:
    pass

import numpy as np  # noqa: E402

from tests import _init_ref as R  # noqa: E402
from voxel_slam_amd import vxba  # noqa: E402

IDENT = R.pack_state(np.eye(3), np.zeros(3))


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def gpu_step_session(case, repeats):
    times, got, stats = [], None, None
    for k in range(repeats + 1):
        with vxba.InitOdometry() as g:
            g.step(case["seed_pts"].astype(np.float32).astype(np.float64), IDENT, case["cov"])
            got, t = ms(lambda: g.step(case["scan_body"], case["state_init"], case["cov"]))
            stats = g.stats()
        if k:
            times.append(t)
    return got, float(np.median(times)), stats


def gpu_window_session(steps, repeats):
    per_step, got = [], None
    for k in range(repeats + 1):
        with vxba.InitOdometry() as g:
            row, got = [], []
            for st in steps:
                r, t = ms(lambda: g.step(st["scan_body"], st["state_init"], st["cov"]))
                row.append(t); got.append((r, g.cloud_size()))
        if k:
            per_step.append(row)
    return got, [float(x) for x in np.median(np.array(per_step), axis=0)]


def gpu_initializer_session(sess, repeats):
    from voxel_slam_amd.init import Initializer
    runs = []
    ini = Initializer(sess.win_size, sess.ext, sess.noise_meas, sess.noise_walk, imupre_scale_gravity=sess.imupre_scale_gravity, **R.MOTION_MAP)
    for k in range(repeats + 1):
        ini.reset()
        rets, t_push = [], []
        for i in range(sess.win_size):
            r, t = ms(lambda: ini.push_scan(sess.scans[i], sess.imus[i], sess.states_init[i], sess.covs[i], sess.beg_times[i]))
            rets.append(r); t_push.append(t)
        if k:
            runs.append(dict(push_ms=t_push, stage_ms=[dict(d) for d in ini.stage_ms], motion=dict(ini.report["stage_ms"])))
    med = lambda rows: [float(x) for x in np.median(np.array(rows), axis=0)]
    stages = {name: med([[d.get(name, 0.0) for d in r["stage_ms"]] for r in runs]) for name in ("filter", "var_init", "odometry", "pvec_update", "raw_copy", "motion_init")}
    motion = {name: float(np.median([r["motion"][name] for r in runs])) for name in runs[0]["motion"]}
    push = med([r["push_ms"] for r in runs])
    return ini, rets, dict(win_size=sess.win_size, points_per_scan=int(sess.scans[0][0].shape[0]), returns=rets, gpu_ms_per_push=push, gpu_ms=float(sum(push)),
                           gpu_stage_ms_per_push=stages, motion_init_gpu_ms=stages["motion_init"][-1], motion_init_stage_ms=motion,
                           rounds=len(ini.report["rounds"]), factor_voxels=[r["n_vox"] for r in ini.report["rounds"]])


def run(a, with_checker=True):
    sess = R.motion_session("room")
    ini, rets, init_res = gpu_initializer_session(sess, a.repeats)
    case = R.make_step_case()
    steps = R.make_window_case()
    got, step_ms, stats = gpu_step_session(case, a.repeats)
    wgot, window_ms = gpu_window_session(steps, a.repeats)
    res = dict(one_step=dict(scan_points=int(case["scan_body"].shape[0]), cloud_points=int(case["seed_pts"].shape[0]), gpu_ms=step_ms, iterations=got["iterations"],
                             refind=got["refind"], valid=got["valid"], launches=stats["launches"], host_syncs=stats["syncs"], cloud_after=stats["cloud_size"]),
               window=dict(steps=len(steps), scan_points=int(steps[0]["scan_body"].shape[0]), gpu_ms_per_step=window_ms, gpu_ms=float(sum(window_ms)),
                           cloud_sizes=[c for _, c in wgot]),
               initializer=init_res, first_measurement=True)
    if not with_checker:
        return res
    want, t = ms(lambda: R.initializer(sess, R.MOTION_MAP))
    got_x, ref_x = np.stack(ini.states), want["motion"]["states"]
    res["initializer"].update(checker_cpu_ms=t, same_returns=rets == want["returns"], same_rounds=[r["n_vox"] for r in want["motion"]["rounds"]] == init_res["factor_voxels"],
                              pose_diff_m=float(np.abs(got_x[:, 9:12] - ref_x[:, 9:12]).max()))
    ref = R.InitOdometryRef()
    ref.step(case["seed_pts"], IDENT, case["cov"])
    want, t = ms(lambda: ref.step(case["scan_body"], case["state_init"], case["cov"]))
    res["one_step"].update(checker_cpu_ms=t, pose_diff_m=float(np.linalg.norm(got["state"][9:12] - want["state"][9:12])), same_schedule=got["refind"] == want["refind"] and got["valid"] == want["valid"])
    ref = R.InitOdometryRef()
    cms = []
    for st in steps:
        _, t = ms(lambda: ref.step(st["scan_body"], st["state_init"], st["cov"]))
        cms.append(t)
    res["window"].update(checker_cpu_ms_per_step=cms, checker_cpu_ms=float(sum(cms)), same_cloud_sizes=[c for _, c in wgot][-1] == ref.cloud_size())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for init.json (and kernel_stats.csv with --profile)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:                                             # under the profiler: the device work only
        run(a, with_checker=False)
        return
    res = run(a)
    if a.profile:
        with tempfile.TemporaryDirectory() as td:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--child", "--repeats", "1"]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            found = sorted(glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True))
            res["profile"] = dict(returncode=p.returncode, kernel_stats=bool(found))
            if found and a.out:
                os.makedirs(a.out, exist_ok=True)
                shutil.copy(found[0], os.path.join(a.out, "kernel_stats.csv"))
            elif not found:
                res["profile"]["stderr_tail"] = p.stderr[-600:]
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "init.json"), "w") as fh:
            json.dump(res, fh, indent=1, default=float)
    print(json.dumps(res, default=float))


if __name__ == "__main__":
    main()
