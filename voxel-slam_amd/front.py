"""The front of the chain: raw scan + raw IMU messages in, through ``IMUEKF::process`` on the GPU (:class:`vxba.ImuEkf`), into the odometry or the
initialisation.

``OdometryFront.step`` is the steady-state branch of ``thd_odometry_localmapping`` (voxelslam.cpp:1571-1594) on the device route: the scan crosses the
bus once, is de-skewed, filtered and handed to ``var_init`` without coming back.  ``feed_initializer`` is the head of ``initialization()`` (:1236-1238).
"""
import numpy as np

from . import vxba


class OdometryFront:
    """process -> voxel filter with the < 500 fallback -> var_init -> lio_state_estimation -> pvec_update, for one scan per :meth:`step`.

    ``ekf``: a :class:`vxba.ImuEkf` (made with the same extrinsic); ``est``: a :class:`vxba.LioEstimator` that holds the plane map; both on one device."""

    def __init__(self, ekf, est, ext, down_size, dept_err=0.02, beam_err=0.05, min_points=500):
        self.ekf, self.est = ekf, est
        self.ext = np.asarray(ext, dtype=np.float64).reshape(12)
        self.down_size, self.dept_err, self.beam_err, self.min_points = float(down_size), float(dept_err), float(beam_err), int(min_points)
        self.degrade_cnt = 0

    def step(self, state, cov, scan, imus, beg_time, end_time):
        """scan: (xyz n x 3 float32 in the LiDAR frame, toff n seconds after ``beg_time``, non-decreasing); imus: (stamps, gyr, acc) of the interval;
        state (24) / cov (15 x 15): ``x_curr`` as the last scan left it.  Returns dict(ready, state, cov, ok, degrade_cnt, pwld, imus, n_filtered,
        half_size, state_prop, cov_prop); while the filter is not ready (``continue`` upstream) only ready, state (with the new gravity) and cov are
        meaningful."""
        r = self.ekf.process(state, cov, scan, imus, beg_time, end_time)
        if not r["ready"]:
            return {"ready": False, "state": r["state"], "cov": r["cov"], "ok": False, "degrade_cnt": self.degrade_cnt, "pwld": None, "imus": None,
                    "n_filtered": 0, "half_size": False, "state_prop": r["state"], "cov_prop": r["cov"]}
        n_f, half = self.ekf.filter(self.down_size, self.min_points)
        d_xyz, n_d = self.ekf.filtered_device()
        self.est.var_init_device(d_xyz, n_d, self.ext, self.dept_err, self.beam_err)
        e = self.est.lio_state_estimation(r["state"], r["cov"])
        if e["ok"]:
            if self.degrade_cnt > 0:
                self.degrade_cnt -= 1
        else:
            self.degrade_cnt += 1
        pwld = self.est.pvec_update(e["state"], e["cov"], with_var=False)
        return {"ready": True, "state": e["state"], "cov": e["cov"], "ok": e["ok"], "degrade_cnt": self.degrade_cnt, "pwld": pwld, "imus": r["imus"],
                "n_filtered": n_f, "half_size": half, "state_prop": r["state"], "cov_prop": r["cov"], "estimation": e}


def feed_initializer(init, ekf, state, cov, scan, imus, beg_time, end_time):
    """``initialization()`` up to its odometry (voxelslam.cpp:1236-1238): the raw scan through ``ekf`` (a :class:`vxba.ImuEkf`), then
    ``init.push_scan`` (an :class:`init.Initializer`) with the handle's propagated state and covariance, its de-skewed scan, the edited message list
    and ``beg_time``.  Returns (push_scan's code -- 0 while the handle is not ready --, the process result)."""
    r = ekf.process(state, cov, scan, imus, beg_time, end_time)
    if not r["ready"]:
        return 0, r
    return init.push_scan(scan, r["imus"], r["state"], r["cov"], beg_time, scan_odom=ekf.read_scan()), r
