"""numpy replay of the driver-message intake, written against the reference's text: one loop-faithful function per handler of ``Features::process``
(VoxelSLAM/src/feature_point.hpp:142-366), ``pcl_handler`` (voxelslam.hpp:76-103) and ``sync_packages`` (:105-161).

The reference's own file needs pcl_conversions and the Livox message headers, so it cannot be compiled as a checker; this replay is the pin for
vxba_intake_* (bit for bit) and for front.PackageSync.  Every float operation is written with np.float32 scalars in the order of the C++ expression:
``ap.x*ap.x + ap.y*ap.y + ap.z*ap.z`` is ((x*x) + (y*y)) + (z*z) in float, compared with the double ``blind``; ``offset_time / float(1000000000)`` is
the uint32 converted to float (round to nearest) and one float division; ``(timestamp - time_head)`` is a double difference assigned to a float.

The choices the product fixes where upstream leaves the result open are applied where a point is pushed (``_push``) and in ``pcl_handler``:
  * a point whose time or any coordinate is not finite is not pushed (upstream's sort is undefined on a NaN; nothing downstream takes an infinity),
  * a time of -0.0 is pushed as +0.0,
  * the sort is stable: by time, ties in input order (upstream's std::sort leaves tie order open),
  * a cloud whose every point lies behind 0.11 raises AllTrimmed (upstream pops an empty vector),
  * the Velodyne branch without a usable time field (:200-252) raises Unsupported.
"""
import collections

import numpy as np

F = np.float32
LIVOX, VELODYNE, OUSTER, HESAI, ROBOSENSE, TARTANAIR = range(6)          # feature_point.hpp:12
_TIME_DTYPES = {0: None, 1: "<f4", 2: "<u4", 3: "<f8"}


class Refused(Exception):
    """upstream dereferences what is not there (points[0] of an empty message)"""


class Unsupported(Exception):
    """the yaw-derived Velodyne times"""


class AllTrimmed(Exception):
    """pcl_handler pops an empty vector; ``record`` is what the run had established by then"""

    def __init__(self, record):
        super().__init__("every point lies behind 0.11")
        self.record = record


def unpack(data, layout):
    """pcl::fromROSMsg / the CustomMsg's point array: (x, y, z float32 arrays, the time field's raw values or None) of a message's point bytes."""
    step = int(layout.point_step)
    names, formats, offsets = ["x", "y", "z"], ["<f4"] * 3, [int(layout.off_x), int(layout.off_y), int(layout.off_z)]
    dt = _TIME_DTYPES[int(layout.time_type)]
    if dt is not None:
        names.append("t"); formats.append(dt); offsets.append(int(layout.off_time))
    rec = np.frombuffer(data, dtype=np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": step}))
    return rec["x"].copy(), rec["y"].copy(), rec["z"].copy(), (rec["t"].copy() if dt is not None else None)


def _push(pl, x, y, z, curvature):
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z) and np.isfinite(curvature)):
        return                                                         # stated deviation
    pl.append((x, y, z, F(0.0) if curvature == 0 else curvature))      # -0.0 -> +0.0


def _beyond_blind(x, y, z, blind):
    with np.errstate(over="ignore", invalid="ignore"):
        s = F(F(F(x * x) + F(y * y)) + F(z * z))
    return float(s) > blind


def livox_handler(x, y, z, offset_time, point_filter_num, blind):      # :142-167
    pl = []
    for i in range(len(x)):
        curvature = F(F(offset_time[i]) / F(1000000000))
        if i % point_filter_num == 0:
            if _beyond_blind(x[i], y[i], z[i], blind):
                _push(pl, x[i], y[i], z[i], curvature)
    return pl


def velodyne_handler(x, y, z, time, point_filter_num, blind):          # :169-254
    pl = []
    plsize = len(x)
    if plsize == 0:
        return pl
    if float(time[-1]) > 0.01 and float(time[-1]) < 0.12:
        for i in range(plsize):
            curvature = F(time[i])
            if i % point_filter_num == 0:
                if _beyond_blind(x[i], y[i], z[i], blind):
                    _push(pl, x[i], y[i], z[i], curvature)
        return pl
    raise Unsupported("velodyne_handler: no usable time field (:200-252)")


def ouster_handler(x, y, z, t, point_filter_num, blind):               # :256-283
    pl = []
    for i in range(len(x)):
        curvature = F(F(t[i]) / F(1e9))
        if i % point_filter_num == 0:
            if _beyond_blind(x[i], y[i], z[i], blind):
                _push(pl, x[i], y[i], z[i], curvature)
    return pl


def hesai_handler(x, y, z, timestamp, point_filter_num, blind):        # :285-317
    pl = []
    if len(x) == 0:
        raise Refused("hesai_handler reads points[0]")
    time_head = np.float64(timestamp[0])
    for i in range(len(x)):
        with np.errstate(over="ignore", invalid="ignore"):
            curvature = F(np.float64(timestamp[i]) - time_head)
        if i % point_filter_num == 0:
            if _beyond_blind(x[i], y[i], z[i], blind):
                _push(pl, x[i], y[i], z[i], curvature)
    return pl


def robosense_handler(x, y, z, timestamp, point_filter_num, blind):    # :319-348
    pl = []
    if len(x) == 0:
        raise Refused("robosense_handler reads pl_orig[0]")
    t0 = np.float64(timestamp[0])
    for i in range(len(x)):
        with np.errstate(over="ignore", invalid="ignore"):
            curvature = F(np.float64(timestamp[i]) - t0)
        if i % point_filter_num == 0:
            if _beyond_blind(x[i], y[i], z[i], blind):
                _push(pl, x[i], y[i], z[i], curvature)
    return pl, float(t0)


def tartanair_handler(x, y, z):                                         # :350-366
    pl = []
    for i in range(len(x)):
        _push(pl, x[i], y[i], z[i], F(0))
    return pl


def pcl_handler(pl, n_decoded):
    """voxelslam.hpp:82-97 on the handler's cloud.  Returns (xyz n x 3 float32, toff n float32, record of six doubles)."""
    n_filtered = len(pl)
    fallback = 0
    if not pl:
        pl = [(F(0), F(0), F(0), F(0)), (F(0), F(0), F(0), F(0.09))]
        fallback = 1
    pl = sorted(pl, key=lambda p: float(p[3]))                          # stable
    while pl and float(pl[-1][3]) > 0.11:
        pl.pop()
    if not pl:
        raise AllTrimmed(np.array([0.0, 0.0, 0.0, 0.0, float(n_decoded), float(n_filtered)]))
    xyz = np.array([p[:3] for p in pl], dtype=np.float32).reshape(-1, 3)
    toff = np.array([p[3] for p in pl], dtype=np.float32)
    rec = np.array([len(pl), float(toff[0]), float(toff[-1]), float(fallback), float(n_decoded), float(n_filtered)])
    return xyz, toff, rec


def process(data, layout, lidar_type, point_filter_num, blind, stamp):
    """``pcl_handler`` on one message: dict(xyz, toff, record, beg_time, time_head)."""
    x, y, z, t = unpack(data, layout)
    beg, head = float(stamp), 0.0
    if lidar_type == LIVOX:
        pl = livox_handler(x, y, z, t, point_filter_num, blind)
    elif lidar_type == VELODYNE:
        pl = velodyne_handler(x, y, z, t, point_filter_num, blind)
    elif lidar_type == OUSTER:
        pl = ouster_handler(x, y, z, t, point_filter_num, blind)
    elif lidar_type == HESAI:
        pl = hesai_handler(x, y, z, t, point_filter_num, blind)
        head = float(t[0])
    elif lidar_type == ROBOSENSE:
        pl, beg = robosense_handler(x, y, z, t, point_filter_num, blind)
        head = beg
    elif lidar_type == TARTANAIR:
        pl = tartanair_handler(x, y, z)
    else:
        raise ValueError("Lidar Type Error")
    xyz, toff, rec = pcl_handler(pl, len(x))
    return {"xyz": xyz, "toff": toff, "record": rec, "beg_time": beg, "time_head": head}


class SyncRef:
    """``sync_packages`` restated loop by loop, with the globals of voxelslam.hpp:42-50 and its static ``pl_ready`` as attributes.  ``exit(0)`` is
    SystemExit; reading ``front()`` of the empty IMU deque (:140, undefined upstream) is SystemExit too."""

    def __init__(self, point_notime=0):
        self.imu_buf, self.pcl_buf, self.time_buf = collections.deque(), collections.deque(), collections.deque()
        self.imu_last_time, self.point_notime, self.last_pcl_time = -1.0, point_notime, -1.0
        self.pl_ready = False
        self.pl_ptr, self.pcl_beg_time, self.pcl_end_time = None, 0.0, 0.0

    def imu_handler(self, stamp):
        self.imu_last_time = stamp
        self.imu_buf.append(stamp)

    def pcl_handler(self, cloud, t0, back_curvature):
        self.time_buf.append(t0)
        self.pcl_buf.append((cloud, back_curvature))

    def sync_packages(self, imus):
        if not self.pl_ready:
            if len(self.pcl_buf) == 0:
                return False
            self.pl_ptr, back = self.pcl_buf[0]
            self.pcl_beg_time = self.time_buf[0]
            self.pcl_buf.popleft(); self.time_buf.popleft()
            self.pcl_end_time = self.pcl_beg_time + back
            if self.point_notime:
                if self.last_pcl_time < 0:
                    self.last_pcl_time = self.pcl_beg_time
                    return False
                self.pcl_end_time = self.pcl_beg_time
                self.pcl_beg_time = self.last_pcl_time
                self.last_pcl_time = self.pcl_end_time
            self.pl_ready = True
        if (not self.pl_ready) or self.imu_last_time <= self.pcl_end_time:
            return False
        if len(self.imu_buf) == 0:
            raise SystemExit("front() of an empty deque")
        imu_time = self.imu_buf[0]
        while len(self.imu_buf) != 0 and imu_time < self.pcl_end_time:
            imu_time = self.imu_buf[0]
            if imu_time > self.pcl_end_time:
                break
            imus.append(self.imu_buf[0])
            self.imu_buf.popleft()
        if len(self.imu_buf) == 0:
            raise SystemExit("imu buf empty")
        self.pl_ready = False
        if len(imus) > 4:
            return True
        return False
