"""The front of the chain: raw scan + raw IMU messages in, through ``IMUEKF::process`` on the GPU (:class:`vxba.ImuEkf`), into the odometry or the
initialisation.

``OdometryFront.step`` is the steady-state branch of ``thd_odometry_localmapping`` (voxelslam.cpp:1571-1594) on the device route: the scan crosses the
bus once, is de-skewed, filtered and handed to ``var_init`` without coming back.  ``feed_initializer`` is the head of ``initialization()`` (:1236-1238).

In front of both: the driver's messages.  ``ScanIntake`` is ``Features::process`` + ``pcl_handler`` (feature_point.hpp:96-368, voxelslam.hpp:76-103) on
the GPU (:class:`vxba.ScanIntake`), ``PackageSync`` is ``sync_packages`` (voxelslam.hpp:105-161), state and all, and ``OdometryFront.step_message`` is
``step`` with the scan taken from the intake's resident cloud: it crosses the bus once, as message bytes.
"""
import collections
import struct

import numpy as np

from . import vxba

LIVOX, VELODYNE, OUSTER, HESAI, ROBOSENSE, TARTANAIR = range(6)        # feature_point.hpp:12
_FLOAT32, _UINT32, _FLOAT64 = 7, 6, 8                                   # sensor_msgs/PointField datatypes
# the time field each handler's point type registers (feature_point.hpp:23-94): name, datatype, vxba_scan_layout time_type and time_rule
_TIME_FIELD = {VELODYNE: ("time", _FLOAT32, vxba.ScanLayout.TIME_F32, vxba.ScanLayout.RULE_AS_IS),
               OUSTER: ("t", _UINT32, vxba.ScanLayout.TIME_U32, vxba.ScanLayout.RULE_NANOSECONDS),
               HESAI: ("timestamp", _FLOAT64, vxba.ScanLayout.TIME_F64, vxba.ScanLayout.RULE_MINUS_HEAD),
               ROBOSENSE: ("timestamp", _FLOAT64, vxba.ScanLayout.TIME_F64, vxba.ScanLayout.RULE_MINUS_HEAD)}


def layout_livox():
    """``livox_ros_driver/CustomPoint`` as it is serialised: 19 bytes, offset_time u32 at 0, x y z f32 at 4 8 12 (reflectivity, tag, line behind)."""
    return vxba.ScanLayout(19, 4, 8, 12, 0, vxba.ScanLayout.TIME_U32, vxba.ScanLayout.RULE_NANOSECONDS, 1)


def _xyz_offsets(who, fields):
    """The byte offsets of the FLOAT32 fields x, y, z of a PointCloud2 field list, and the list as a dict name -> (offset, datatype)."""
    by_name = {}
    for name, offset, datatype in fields:
        if name in by_name:
            raise ValueError(f"{who}: field {name!r} is listed twice")
        by_name[name] = (int(offset), int(datatype))
    off = []
    for name in ("x", "y", "z"):
        if name not in by_name:
            raise ValueError(f"{who}: no field {name!r}")
        o, dt = by_name[name]
        if dt != _FLOAT32:
            raise ValueError(f"{who}: field {name!r} is not FLOAT32")
        off.append(o)
    return off, by_name


def _check_spans(who, spans, point_step):
    if not 12 <= int(point_step) <= vxba.ScanLayout.MAX_STEP:
        raise ValueError(f"{who}: point_step {point_step} outside 12..{vxba.ScanLayout.MAX_STEP}")
    spans = sorted(spans)
    for k, (o, ln) in enumerate(spans):
        if o < 0 or o + ln > int(point_step) or (k and spans[k - 1][0] + spans[k - 1][1] > o):
            raise ValueError(f"{who}: a field leaves the point or overlaps another")


def layout_from_fields(fields, point_step, lidar_type, is_bigendian=False):
    """A layout from a PointCloud2 field list of (name, offset, datatype) -- count 1 assumed -- for the handler ``lidar_type`` selects.  Little-endian
    only; x, y, z must be FLOAT32 and the time field must carry the name and datatype the handler's point type registers (``time`` FLOAT32, ``t``
    UINT32, ``timestamp`` FLOAT64): pcl::fromROSMsg maps nothing else.  ValueError on anything else."""
    who = "layout_from_fields"
    if is_bigendian:
        raise ValueError("layout_from_fields: big-endian messages are not supported")
    if lidar_type == LIVOX:
        raise ValueError("layout_from_fields: Livox sends a CustomMsg, not a PointCloud2 (layout_livox)")
    if lidar_type not in (VELODYNE, OUSTER, HESAI, ROBOSENSE, TARTANAIR):
        raise ValueError(f"layout_from_fields: unknown lidar_type {lidar_type}")
    off, by_name = _xyz_offsets(who, fields)
    if lidar_type == TARTANAIR:
        lay = vxba.ScanLayout(int(point_step), off[0], off[1], off[2], 0, vxba.ScanLayout.TIME_NONE, vxba.ScanLayout.RULE_NONE, 0)
        spans = [(o, 4) for o in off]
    else:
        name, want, ttype, rule = _TIME_FIELD[lidar_type]
        if name not in by_name:
            raise ValueError(f"layout_from_fields: no time field {name!r}")
        o, dt = by_name[name]
        if dt != want:
            raise ValueError(f"layout_from_fields: time field {name!r} has datatype {dt}, the handler reads {want}")
        lay = vxba.ScanLayout(int(point_step), off[0], off[1], off[2], o, ttype, rule, 1)
        spans = [(p, 4) for p in off] + [(o, 8 if want == _FLOAT64 else 4)]
    _check_spans(who, spans, point_step)
    return lay


def layout_velodyne_yaw(fields, point_step, is_bigendian=False):
    """A ``RULE_YAW`` layout from a PointCloud2 field list: a Velodyne message whose point times are derived from the yaw angle
    (feature_point.hpp:200-252).  No ``time`` field is needed and one that is listed is not read.  The checks on x, y, z, point_step and the
    spans are :func:`layout_from_fields`'."""
    who = "layout_velodyne_yaw"
    if is_bigendian:
        raise ValueError("layout_velodyne_yaw: big-endian messages are not supported")
    off, _ = _xyz_offsets(who, fields)
    _check_spans(who, [(o, 4) for o in off], point_step)
    return vxba.ScanLayout(int(point_step), off[0], off[1], off[2], 0, vxba.ScanLayout.TIME_NONE, vxba.ScanLayout.RULE_YAW, 1)


class ScanIntake:
    """``Features::process`` + ``pcl_handler`` for one sensor: :meth:`push` takes a message's point bytes and its header stamp and returns ``beg_time``.

    ``lidar_type``: LIVOX .. TARTANAIR; ``layout``: :func:`layout_livox` / :func:`layout_from_fields` / :func:`layout_velodyne_yaw`;
    ``point_filter_num`` / ``blind``: the reference's.  ``yaw_times`` (Velodyne only): a message whose layout is ``RULE_YAW``, or whose last ``time``
    fails upstream's test (:176), gets its point times from the yaw angles at ``omega_l`` degrees per second (:200-252); without it such a message
    is refused (``VXBA_ERR_UNSUPPORTED``)."""

    def __init__(self, lidar_type, layout, point_filter_num=1, blind=1.0, device=0, yaw_times=False, omega_l=3610.0):
        self.lidar_type, self.layout, self.point_filter_num, self.blind = int(lidar_type), layout, int(point_filter_num), float(blind)
        self.yaw_times, self.omega_l = bool(yaw_times), float(omega_l)
        self.route = None                      # "yaw" or "push": where the last message went
        self.dev = vxba.ScanIntake(device)
        self.record = None

    def _point0_time(self, data):
        o = int(self.layout.off_time)
        return struct.unpack_from("<d", data, o)[0]

    def _yaw_layout(self, data):
        """The layout a Velodyne message goes to ``push_yaw`` with under ``yaw_times``, or None: its own when that is ``RULE_YAW``; its own with the
        rule replaced when the last point's ``time`` is not in (0.01, 0.12) -- feature_point.hpp:176, read on the host as vxba_intake_push does."""
        lay = self.layout
        if int(lay.time_rule) == vxba.ScanLayout.RULE_YAW:
            return lay
        step = int(lay.point_step)
        if int(lay.time_rule) != vxba.ScanLayout.RULE_AS_IS or len(data) < step or len(data) % step:
            return None
        t = np.float32(struct.unpack_from("<f", data, len(data) - step + int(lay.off_time))[0])
        if float(t) > 0.01 and float(t) < 0.12:
            return None
        return vxba.ScanLayout(step, lay.off_x, lay.off_y, lay.off_z, lay.off_time, lay.time_type, vxba.ScanLayout.RULE_YAW, 1)

    def push(self, data, stamp):
        """data: n x point_step bytes.  Returns beg_time: the header stamp, or for Robosense the first point's timestamp (feature_point.hpp:326, 347).
        Hesai and Robosense take ``time_head`` from point 0."""
        data = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
        head, beg = 0.0, float(stamp)
        if self.yaw_times and self.lidar_type == VELODYNE:
            lay = self._yaw_layout(data)
            if lay is not None:
                self.record = self.dev.push_yaw(lay, data, self.point_filter_num, self.blind, self.omega_l)
                self.route = "yaw"
                return beg
        self.route = "push"
        if self.lidar_type in (HESAI, ROBOSENSE):
            if len(data) < int(self.layout.point_step):
                raise vxba.VxbaError("ScanIntake.push: an empty Hesai / Robosense message (upstream reads points[0])")
            head = self._point0_time(data)
            if self.lidar_type == ROBOSENSE:
                beg = head
        self.record = self.dev.push(self.layout, data, self.point_filter_num, self.blind, head)
        return beg

    def read(self):
        return self.dev.read()

    def close(self):
        self.dev.close()


class PackageSync:
    """``sync_packages`` (voxelslam.hpp:105-161) with the buffers ``pcl_handler`` / ``imu_handler`` fill (:42-103), state and all.

    ``add_scan(scan, beg_time, toff_last)``: what pcl_handler pushes -- ``scan`` is any token for the cloud (an array pair, a message's bytes to push
    later), ``toff_last`` its last ``curvature``.  ``add_imu(stamp, gyr, acc)``: imu_handler.  :meth:`sync` returns (ok, scan, imus, beg, end): ``scan``
    persists while the IMU has not passed the scan's end (``pl_ready``); ``imus`` is the caller's list, appended to as upstream's deque is."""

    def __init__(self, point_notime=False):
        self.point_notime = bool(point_notime)
        self.imu_buf, self.pcl_buf, self.time_buf = collections.deque(), collections.deque(), collections.deque()
        self.imu_last_time, self.last_pcl_time = -1.0, -1.0
        self.pl_ready = False
        self.scan, self.beg_time, self.end_time = None, 0.0, 0.0

    def add_imu(self, stamp, gyr, acc):
        self.imu_last_time = float(stamp)
        self.imu_buf.append((float(stamp), np.asarray(gyr, dtype=np.float64), np.asarray(acc, dtype=np.float64)))

    def add_scan(self, scan, beg_time, toff_last):
        self.time_buf.append(float(beg_time))
        self.pcl_buf.append((scan, float(toff_last)))

    def sync(self, imus):
        if not self.pl_ready:
            if not self.pcl_buf:
                return False, self.scan, imus, self.beg_time, self.end_time
            self.scan, toff_last = self.pcl_buf.popleft()
            self.beg_time = self.time_buf.popleft()
            self.end_time = self.beg_time + toff_last
            if self.point_notime:
                if self.last_pcl_time < 0:
                    self.last_pcl_time = self.beg_time
                    return False, self.scan, imus, self.beg_time, self.end_time
                self.end_time = self.beg_time
                self.beg_time = self.last_pcl_time
                self.last_pcl_time = self.end_time
            self.pl_ready = True
        if not self.pl_ready or self.imu_last_time <= self.end_time:
            return False, self.scan, imus, self.beg_time, self.end_time
        if not self.imu_buf:
            raise RuntimeError("PackageSync.sync: imu buf empty")        # upstream reads front() of the empty deque, then exits
        imu_time = self.imu_buf[0][0]
        while self.imu_buf and imu_time < self.end_time:
            imu_time = self.imu_buf[0][0]
            if imu_time > self.end_time:
                break
            imus.append(self.imu_buf.popleft())
        if not self.imu_buf:
            raise RuntimeError("PackageSync.sync: imu buf empty")        # printf + exit(0) upstream
        self.pl_ready = False
        return len(imus) > 4, self.scan, imus, self.beg_time, self.end_time

    @staticmethod
    def pack(imus):
        """The drained list as the (stamps, gyr, acc) arrays :meth:`OdometryFront.step` takes."""
        return (np.array([m[0] for m in imus], dtype=np.float64), np.array([m[1] for m in imus], dtype=np.float64).reshape(-1, 3),
                np.array([m[2] for m in imus], dtype=np.float64).reshape(-1, 3))


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
        return self._after_process(self.ekf.process(state, cov, scan, imus, beg_time, end_time))

    def step_message(self, state, cov, intake, imus, beg_time, end_time):
        """:meth:`step` with the scan taken from ``intake`` (a :class:`ScanIntake` or a :class:`vxba.ScanIntake` after its push), device to device."""
        return self._after_process(self.ekf.process_device(state, cov, getattr(intake, "dev", intake), imus, beg_time, end_time))

    def _after_process(self, r):
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
    if hasattr(scan, "read"):                  # a scan intake after its push: the initialisation keeps its clouds on the host
        scan = scan.read()
    r = ekf.process(state, cov, scan, imus, beg_time, end_time)
    if not r["ready"]:
        return 0, r
    return init.push_scan(scan, r["imus"], r["state"], r["cov"], beg_time, scan_odom=ekf.read_scan()), r
