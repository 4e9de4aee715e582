"""The initialisation stage on the GPU: ``initialization()`` of the reference (voxelslam.cpp:1230-1288) after ``odom_ekf.process``.

Raw scans, the raw IMU messages of their intervals and the propagated state of every scan go in; after ``win_size`` scans an initialised window comes
out: states, gravity, IMU factors, the resident local map, the factor and the Hessian -- what ``LI_BA_Optimizer.damping_iter`` and the map's scan
cycle take over from.  ``IMUEKF::process`` (the IMU propagation and per-scan de-skew in front of the odometry) is :class:`vxba.ImuEkf`: its results are
the ``state_prop`` / ``cov_prop`` / ``scan_odom`` arguments of ``push_scan``, and ``front.feed_initializer`` passes them on.
"""
import time

import numpy as np

from . import vxba


class Initializer:
    """``push_scan`` once per scan; returns 0 while the window fills, then 1 (initialised) or -1 (``motion_init`` failed: the caller resets, as upstream).

    After a 1: ``states`` (W x 24, ``x_curr`` is the last), ``covs``, ``imus_factor`` (W - 1 ``IMU_PRE``), ``local_map``, ``factor``, ``hess``, ``report``."""

    def __init__(self, win_size, ext, noise_meas, noise_walk, voxel_size=1.0, max_layer=2, min_point=(20, 20, 15, 10), min_eigen_value=0.0025,
                 plane_eigen_value_thre=(0.25, 0.25, 0.25, 0.25), max_points=100, down_size=0.1, dept_err=0.02, beam_err=0.05, imupre_scale_gravity=1.0,
                 imu_coef=1e-4, point_notime=False, device=0):
        self.win_size = int(win_size)
        self.ext = np.asarray(ext, dtype=np.float64).reshape(12)
        self.noise_meas, self.noise_walk = np.asarray(noise_meas, dtype=np.float64), np.asarray(noise_walk, dtype=np.float64)
        self.min_eigen_value, self.plane_eigen_value_thre = float(min_eigen_value), tuple(plane_eigen_value_thre)
        self.down_size, self.dept_err, self.beam_err = float(down_size), float(dept_err), float(beam_err)
        self.imupre_scale_gravity, self.imu_coef, self.point_notime, self.device = float(imupre_scale_gravity), float(imu_coef), bool(point_notime), int(device)
        self.odom = vxba.InitOdometry(device=device)
        self.est = vxba.LioEstimator(voxel_size=voxel_size, max_layer=max_layer, device=device)       # var_init / pvec_update of the scan
        # thread_num = 1: motion_init walks every root itself, the early returns of the multi-thread variants never fire
        self.local_map = vxba.LocalMap(voxel_size=voxel_size, max_layer=max_layer, min_point=min_point, min_eigen_value=min_eigen_value,
                                       plane_eigen_value_thre=plane_eigen_value_thre, max_points=max_points, win_size=win_size, thread_num=1, device=device)
        self.factor = vxba.LidarFactor(win_size, device=device)
        self.reset()

    def reset(self):
        """``system_reset`` as far as this stage goes: the world cloud, the map, the factor and the buffers."""
        self.odom.clear(); self.local_map.clear(); self.factor.clear()
        self.states, self.covs, self.imus_factor, self.scans, self.beg_times, self.imus = [], [], [], [], [], []
        self.hess, self.report, self.pwld = None, None, None
        self.stage_ms = []      # per push_scan: wall milliseconds of filter, var_init, odometry, pvec_update, raw_copy (and motion_init on the last)

    @property
    def win_count(self):
        return len(self.states)

    def push_scan(self, scan, imus, state_prop, cov_prop, beg_time, scan_odom=None):
        """scan: (xyz n x 3 float32 in the LiDAR frame, toff n seconds after ``beg_time``) as received; imus: (stamps, gyr, acc) of its interval;
        state_prop (24) / cov_prop (15 x 15): the IMU-propagated state at the scan's end; scan_odom: the scan as ``IMUEKF::process`` de-skewed it for
        the odometry (None: the raw points)."""
        if self.win_count >= self.win_size:
            raise vxba.VxbaError("Initializer.push_scan: the window is full (reset first)")
        xyz = np.ascontiguousarray(scan[0], dtype=np.float32).reshape(-1, 3)
        toff = np.ascontiguousarray(scan[1], dtype=np.float32).reshape(-1)
        cur = xyz if scan_odom is None else np.ascontiguousarray(scan_odom, dtype=np.float32).reshape(-1, 3)
        tm, t0 = {}, time.perf_counter()

        def lap(name):
            nonlocal t0
            t1 = time.perf_counter()
            tm[name] = 1e3 * (t1 - t0); t0 = t1
        self.stage_ms.append(tm)
        cur = vxba.down_sampling_voxel(cur, max(self.down_size, 0.5), device=self.device)
        lap("filter")
        self.est.var_init(cur, self.ext[:9].reshape(3, 3).T, self.ext[9:12], self.dept_err, self.beam_err)
        pnt, _ = self.est.read_points()
        lap("var_init")
        r = self.odom.step(pnt, state_prop, cov_prop)                             # lio_state_estimation_kdtree
        lap("odometry")
        x_curr, cov = r["state"], r["cov"]
        self.pwld = self.est.pvec_update(x_curr, cov, with_var=False)
        lap("pvec_update")
        if self.win_count >= 1:                                                   # IMU_PRE(x_buf[win_count - 2].bg, .ba) -> push_imu(imus)
            prev = self.states[-1]
            fac = vxba.IMU_PRE(prev[15:18], prev[18:21])
            fac.push_imu(imus[0], imus[1], imus[2], self.imupre_scale_gravity, self.noise_meas, self.noise_walk)
            self.imus_factor.append(fac)
        self.states.append(np.asarray(x_curr, dtype=np.float64).copy()); self.covs.append(np.asarray(cov, dtype=np.float64).copy())
        # the raw copy for motion_init: down_sampling_close, the < 1000 fallback at half the size, sorted by time
        pts, sel = vxba.down_sampling_close(xyz, self.down_size, device=self.device)
        if pts.shape[0] < 1000:
            pts, sel = vxba.down_sampling_close(xyz, self.down_size / 2, device=self.device)
        o = np.argsort(toff[sel], kind="stable")
        self.scans.append((pts[o], toff[sel][o])); self.beg_times.append(float(beg_time))
        self.imus.append(tuple(np.asarray(a, dtype=np.float64) for a in imus))
        lap("raw_copy")
        if self.win_count < self.win_size:
            return 0
        got = vxba.motion_init(self.local_map, self.factor, self.scans, np.array(self.beg_times), self.imus, np.stack(self.states), np.stack(self.covs), self.ext,
                               self.imus_factor, self.noise_meas, self.noise_walk, self.min_eigen_value, self.plane_eigen_value_thre,
                               imupre_scale_gravity=self.imupre_scale_gravity, dept_err=self.dept_err, beam_err=self.beam_err, point_notime=self.point_notime,
                               imu_coef=self.imu_coef)
        lap("motion_init")
        self.states = list(got["states"]); self.hess = got["hess"]; self.report = got
        return 1 if got["flag"] else -1
