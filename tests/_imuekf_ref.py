"""Numpy replay of ``IMUEKF`` (VoxelSLAM/src/ekf_imu.hpp:41-214; include/vxba.h: vxba_imuekf_*): the CHECKER of tests/test_gpu_imuekf.py and of
tests/test_imuekf_cpu.py, never the thing run.

``IMU_init``, ``process`` and ``motion_blur`` are written against the reference's text, loop for loop: the message list with ``last_imu`` pushed in
front, the skipped pairs, the clamped ``cur_time``, ``imu_poses`` stored before each step, ``F_x`` / ``cov_w`` block by block, the tail with ``note``,
the re-stamped front and back, and the backward walk over the scan with its ``break`` at ``begin()`` that leaves only the inner loop.  Points are
stored in float32, as ``PointType`` stores them: every compensated point is rounded to float32 before anything else reads it.

The reference's own class cannot be compiled as a pin against the committed API stand-ins (``sensor_msgs::Imu::Ptr``, ``asDiagonal``), so this model is
pinned to mathematics in turn (tests/test_imuekf_cpu.py): closed-form motions, central differences of its own mean propagation, the closed form of the
``IMU_init`` recurrence.

Where upstream has undefined behaviour or exits, ``process`` raises :class:`Refused`; so does the product.
"""
import numpy as np

from tests import _oracle as O
from tests._init_ref import exp_rate

G_M_S2 = 9.8
MAX_HEADS = 64


class Refused(ValueError):
    pass


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=np.float64)


def unpack(state):
    s = np.asarray(state, dtype=np.float64)
    return dict(R=s[:9].reshape(3, 3).T.copy(), p=s[9:12].copy(), v=s[12:15].copy(), bg=s[15:18].copy(), ba=s[18:21].copy(), g=s[21:24].copy())


def pack(x):
    return np.concatenate([x["R"].T.reshape(9), x["p"], x["v"], x["bg"], x["ba"], x["g"]])


def step_matrices(R, rate, acc, dt, cov_acc, cov_gyr, cov_bias_gyr, cov_bias_acc):
    """F_x and cov_w of one step (:89-103)."""
    F = np.eye(15); W = np.zeros((15, 15))
    F[0:3, 0:3] = exp_rate(rate, -dt)
    F[0:3, 9:12] = -np.eye(3) * dt
    F[3:6, 6:9] = np.eye(3) * dt
    F[6:9, 0:3] = -R @ hat(acc) * dt
    F[6:9, 12:15] = -R * dt
    W[0:3, 0:3] = np.diag(cov_gyr * dt * dt)
    W[6:9, 6:9] = R @ np.diag(cov_acc) @ R.T * dt * dt
    W[9:12, 9:12] = np.diag(cov_bias_gyr * dt * dt)
    W[12:15, 12:15] = np.diag(cov_bias_acc * dt * dt)
    return F, W


class ImuEkfRef:
    def __init__(self, cov_acc=0.1, cov_gyr=0.1, cov_bias_gyr=1e-4, cov_bias_acc=1e-4, ext=None, acc_in_g=True, point_notime=False):
        b = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (3,)).copy()
        self.cov_acc, self.cov_gyr, self.cov_bias_gyr, self.cov_bias_acc = b(cov_acc), b(cov_gyr), b(cov_bias_gyr), b(cov_bias_acc)
        e = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]) if ext is None else np.asarray(ext, dtype=np.float64).reshape(12)
        self.L, self.l = e[:9].reshape(3, 3).T.copy(), e[9:12].copy()       # Lid_rot_to_IMU, Lid_offset_to_IMU
        self.acc_in_g, self.point_notime = bool(acc_in_g), bool(point_notime)
        self.min_init_num = 30
        self.clear()

    def clear(self):
        self.init_flag, self.init_num = False, 0
        self.mean_acc, self.mean_gyr = np.zeros(3), np.zeros(3)
        self.scale_gravity, self.last_pcl_end_time = 1.0, 0.0
        self.last_imu = None                                                # (stamp, gyr, acc)
        self.imu_poses = []

    # ---- IMU_init (:167-195) ----
    def imu_init(self, imus):
        for stamp, cur_gyr, cur_acc in imus:
            if self.init_num != 0:
                self.mean_acc = self.mean_acc + (cur_acc - self.mean_acc) / self.init_num
                self.mean_gyr = self.mean_gyr + (cur_gyr - self.mean_gyr) / self.init_num
            else:
                self.mean_acc = cur_acc.copy()
                self.mean_gyr = cur_gyr.copy()
                self.init_num = 1
            self.init_num += 1
        self.last_imu = imus[-1]

    def reinit(self, imus, scale):
        """system_reset's share (voxelslam.cpp:1302-1305)."""
        self.mean_acc = np.zeros(3); self.init_num = 0
        self.imu_init(_messages(imus))
        return -self.mean_acc * scale

    # ---- process (:197-214) ----
    def process(self, state, cov, scan, imus, beg_time, end_time):
        """Returns dict(ready, state, cov, imus, scan (float32, de-skewed in place), heads, compensated, point0_applications)."""
        msgs = _messages(imus)
        x = unpack(state); cov = np.array(cov, dtype=np.float64).reshape(15, 15)
        if len(msgs) < 1 or not all(np.isfinite(m[0]) and np.isfinite(m[1]).all() and np.isfinite(m[2]).all() for m in msgs):
            raise Refused("messages")
        if not (np.isfinite(pack(x)).all() and np.isfinite(cov).all() and np.isfinite(beg_time) and np.isfinite(end_time)):
            raise Refused("state")
        if not self.init_flag:
            self.imu_init(msgs)
            if np.linalg.norm(self.mean_acc) < 2 and self.acc_in_g:
                self.scale_gravity = G_M_S2
            x["g"] = -self.mean_acc * self.scale_gravity
            if self.init_num > self.min_init_num:
                self.init_flag = True
            self.last_pcl_end_time = end_time
            return dict(ready=False, state=pack(x), cov=cov, imus=None, scan=None, heads=0, compensated=0, point0_applications=0)
        xyz = np.array(scan[0], dtype=np.float32).reshape(-1, 3)
        toff = None if scan[1] is None else np.asarray(scan[1], dtype=np.float32).reshape(-1)
        self._refusals(xyz, toff, msgs, beg_time)
        return self.motion_blur(x, cov, xyz, toff, msgs, beg_time, end_time)

    def _refusals(self, xyz, toff, msgs, beg_time):
        if xyz.shape[0] == 0:
            raise Refused("empty scan: upstream dereferences end() - 1")
        if not np.isfinite(xyz).all() or (toff is not None and not np.isfinite(toff).all()):
            raise Refused("scan not finite")
        if self.last_pcl_end_time - beg_time > 0.01:
            raise Refused("LiDAR time regress: upstream exits")
        if toff is not None and not self.point_notime and (np.diff(toff) < 0).any():
            raise Refused("toff not sorted: upstream sorts in pcl_handler")
        stamps = np.array([self.last_imu[0]] + [m[0] for m in msgs])
        if (np.diff(stamps) < 0).any():
            raise Refused("IMU stamps go back")
        n_pairs = int((stamps[1:] >= self.last_pcl_end_time).sum())
        if n_pairs == 0:
            raise Refused("no surviving pair: upstream reads uninitialised vectors")
        if n_pairs > MAX_HEADS:
            raise Refused("unsupported: more than 64 heads")

    # ---- motion_blur (:41-165) ----
    def motion_blur(self, xc, cov, pcl_in, toff, imus, pcl_beg_time, pcl_end_time):
        imus = [self.last_imu] + list(imus)                                 # imus.push_front(last_imu)
        self.imu_poses = []
        vel_imu, pos_imu, R_imu = xc["v"].copy(), xc["p"].copy(), xc["R"].copy()
        acc_imu = angvel_avr = None
        for head, tail in zip(imus[:-1], imus[1:]):
            if tail[0] < self.last_pcl_end_time:
                continue
            angvel_avr = 0.5 * (head[1] + tail[1])
            acc_avr = 0.5 * (head[2] + tail[2])
            angvel_avr = angvel_avr - xc["bg"]
            acc_avr = acc_avr * self.scale_gravity - xc["ba"]
            acc_imu = R_imu @ acc_avr + xc["g"]
            cur_time = head[0]
            if cur_time < self.last_pcl_end_time:
                cur_time = self.last_pcl_end_time
            dt = tail[0] - cur_time
            offt = cur_time - pcl_beg_time
            self.imu_poses.append(dict(t=offt, R=R_imu.copy(), p=pos_imu.copy(), v=vel_imu.copy(), bg=angvel_avr.copy(), ba=acc_imu.copy()))
            Exp_f = exp_rate(angvel_avr, dt)
            F_x, cov_w = step_matrices(R_imu, angvel_avr, acc_avr, dt, self.cov_acc, self.cov_gyr, self.cov_bias_gyr, self.cov_bias_acc)
            cov = F_x @ cov @ F_x.T + cov_w
            pos_imu = pos_imu + vel_imu * dt + 0.5 * acc_imu * dt * dt
            vel_imu = vel_imu + acc_imu * dt
            R_imu = R_imu @ Exp_f
        imu_end_time = imus[-1][0]
        note = 1.0 if pcl_end_time > imu_end_time else -1.0
        dt = note * (pcl_end_time - imu_end_time)
        xc = dict(xc)
        xc["v"] = vel_imu + note * acc_imu * dt
        xc["R"] = R_imu @ exp_rate(note * angvel_avr, dt)
        xc["p"] = pos_imu + note * vel_imu * dt + note * 0.5 * acc_imu * dt * dt
        imu1 = (self.last_pcl_end_time, imus[0][1], imus[0][2])
        imu2 = (pcl_end_time, imus[-1][1], imus[-1][2])
        self.last_imu = imus[-1]
        self.last_pcl_end_time = pcl_end_time
        imus[0] = imu1; imus[-1] = imu2
        edited = (np.array([m[0] for m in imus]), np.array([m[1] for m in imus]), np.array([m[2] for m in imus]))
        out = dict(ready=True, state=pack(xc), cov=cov, imus=edited, scan=pcl_in, heads=len(self.imu_poses), compensated=0, point0_applications=0)
        if self.point_notime:
            return out
        touched = np.zeros(pcl_in.shape[0], dtype=bool)
        L, l = self.L, self.l
        it_pcl = pcl_in.shape[0] - 1                                        # pcl_in.end() - 1
        for head in reversed(self.imu_poses):
            while float(toff[it_pcl]) > head["t"]:
                dt = float(toff[it_pcl]) - head["t"]
                R_i = head["R"] @ exp_rate(head["bg"], dt)
                T_ei = head["p"] + head["v"] * dt + 0.5 * head["ba"] * dt * dt - xc["p"]
                P_i = pcl_in[it_pcl].astype(np.float64)
                P_compensate = L.T @ (xc["R"].T @ (R_i @ (L @ P_i + l) + T_ei) - l)
                pcl_in[it_pcl] = P_compensate.astype(np.float32)
                touched[it_pcl] = True
                if it_pcl == 0:
                    out["point0_applications"] += 1
                    break
                it_pcl -= 1
        out["compensated"] = int(touched.sum())
        return out

    def pose_table(self):
        return np.array([np.concatenate([[e["t"]], e["R"].T.reshape(9), e["p"], e["v"], e["bg"], e["ba"]]) for e in self.imu_poses]).reshape(-1, 22)


def _messages(imus):
    st, gy, ac = np.asarray(imus[0], dtype=np.float64).reshape(-1), np.asarray(imus[1], dtype=np.float64).reshape(-1, 3), np.asarray(imus[2], dtype=np.float64).reshape(-1, 3)
    return [(float(st[k]), gy[k].copy(), ac[k].copy()) for k in range(st.shape[0])]


def filter_scan(xyz32, down_size, min_points=500):
    """voxelslam.cpp:1574-1581: (filtered cloud, whether the half size was used)."""
    out = O.down_sampling_voxel(np.ascontiguousarray(xyz32, dtype=np.float32), down_size)
    if out.shape[0] < min_points:
        return O.down_sampling_voxel(np.ascontiguousarray(xyz32, dtype=np.float32), down_size / 2), True
    return out, False


def push_imu_dt_sum(edited):
    """The sum of the dt that IMU_PRE::push_imu (preintegration.hpp:50-73) forms from the edited list."""
    return float(np.diff(edited[0]).sum())


def tol(K, x):
    """K steps of 15-term sums in f64, x 64 for the order of summation."""
    return 64.0 * K * 2.0 ** -52 * np.maximum(1.0, np.abs(x))


def ulp_diff32(a, b):
    """Distance in float32 units in the last place between two float32 arrays (same sign assumed where they differ by few ulps)."""
    ia = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ---- cases shared by the CPU and the GPU tests -------------------------------------------------------------------------------------------
def ext_default():
    from tests._init_ref import so3_exp
    eR = so3_exp(np.array([0.02, -0.03, 0.5])); ep = np.array([0.1, 0.05, -0.02])
    return np.concatenate([eR.T.reshape(9), ep])


def stationary_imus(beg, K, dt, last, acc=(0.01, -0.02, 0.98), gyr=(0.001, -0.002, 0.0005), seed=0):
    """K messages of a sensor at rest (accelerometer in g by default), stamps rising by dt to `last` exactly."""
    rng = np.random.default_rng(seed)
    st = last - dt * np.arange(K - 1, -1, -1)
    st[-1] = last
    return st, np.asarray(gyr) + 1e-4 * rng.normal(size=(K, 3)), np.asarray(acc) + 1e-3 * rng.normal(size=(K, 3))


def initialise(f, t_end=100.0, lag=0.0, scans=3, K=10, dt=0.01, acc=(0.01, -0.02, 0.98), state=None):
    """Feed `scans` stationary intervals through process() of a checker or of a vxba.ImuEkf: 3 x 10 messages make init_num 31 > 30.  The last scan ends
    at t_end exactly and its last message is stamped t_end - lag.  Returns (state with the estimated g, results)."""
    st = np.concatenate([np.eye(3).reshape(9), np.zeros(15)]) if state is None else np.asarray(state, dtype=np.float64).copy()
    cov = np.eye(15) * 1e-4
    res = []
    xyz = np.ones((1, 3), dtype=np.float32); toff = np.zeros(1, dtype=np.float32)
    for s in range(scans):
        end = t_end - (scans - 1 - s) * K * dt if s < scans - 1 else t_end
        r = f.process(st, cov, (xyz, toff), stationary_imus(end - K * dt, K, dt, end - lag, acc=acc, seed=100 + s), end - K * dt, end)
        st = r["state"]; res.append(r)
    return st, res


def make_case(n, K, seed=0, t_end=100.0, lag=0.0, span=0.1, prefix=0, late_first=0, ties=False, on_head=False, one_head=False, rate=(0.4, -0.3, 0.5), grid=False,
              end_after=True):
    """One scan interval behind :func:`initialise` (t_end, lag).  K messages at t_end + span k / K, k = 1..K (`grid`: at t_end + k / 128, so that every
    head offset is exact in float32); n points with times inside the interval.
      prefix      that many leading points with toff <= t_0 = 0
      late_first  point 0 is later than exactly that many heads
      ties        runs of equal times
      on_head     some toff equal a head's time exactly (needs `grid`)
      one_head    every message but the last lies between the last message and the last scan end (needs lag > 0): all pairs but one are skipped, and
                  the surviving head's time is clamped
      end_after   the scan ends after the last message (note = +1) or before it (note = -1)."""
    rng = np.random.default_rng(seed)
    step = 1.0 / 128.0 if grid else span / K
    span = K * step
    stamps = t_end + step * np.arange(1, K + 1)
    if one_head:
        assert lag > 0
        stamps = np.concatenate([t_end - lag + lag * np.arange(1, K) / (K + 1), [t_end + span]])
    gyr = np.asarray(rate) + 0.05 * rng.normal(size=(K, 3))
    acc = np.array([0.02, -0.01, 1.0]) + 0.05 * rng.normal(size=(K, 3))
    lo = step * (late_first - 1) + 0.25 * step if late_first else 1e-4
    t = np.sort(rng.uniform(lo, span, n))
    t[0] = lo
    if ties and n >= 8:
        t[n // 4: n // 4 + 3] = t[n // 4]; t[n // 2: n // 2 + 4] = t[n // 2]
    if on_head and n >= 6:
        heads = step * np.arange(1, min(K, 4))
        t[np.linspace(2, n - 2, heads.shape[0]).astype(int)] = heads
    t = np.sort(t)
    if prefix:
        t[:prefix] = np.linspace(-0.002, 0.0, prefix)
    toff = np.maximum.accumulate(t.astype(np.float32))
    xyz = (rng.uniform(-10, 10, size=(n, 3))).astype(np.float32)
    return dict(scan=(xyz, toff), imus=(stamps, gyr, acc), beg=t_end, end=t_end + span + (0.3 if end_after else -0.3) * step)


def moving_state(g):
    from tests._init_ref import so3_exp
    R = so3_exp(np.array([0.1, 0.2, -0.1]))
    return np.concatenate([R.T.reshape(9), [0.5, -0.2, 0.1], [1.0, -0.5, 0.3], [0.01, -0.02, 0.005], [0.05, 0.02, -0.03], g])


def moving_cov(seed=5):
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(15, 15)) * 1e-2
    return np.eye(15) * 1e-4 + M @ M.T




# every shape and quirk tests/test_gpu_imuekf.py runs, by name: keyword arguments of make_case plus the filter's options
LAG = 0.003


def gpu_cases():
    cases = {}
    for n in (1, 2, 63, 64, 65, 257, 3000):
        for K in (5, 21):
            cases[f"n{n}_K{K}"] = dict(n=n, K=K, seed=7 * n + K, lag=LAG, ties=True, prefix=3 if n >= 63 else 0, end_after=K == 5)
    cases["one_head"] = dict(n=257, K=5, seed=11, lag=LAG, one_head=True)                     # M = 1: all pairs but one skipped, the head's time clamped
    cases["late_first"] = dict(n=257, K=21, seed=12, lag=LAG, late_first=3)                   # the first point is later than 3 heads
    cases["on_head"] = dict(n=257, K=5, seed=13, lag=0.0, grid=True, on_head=True, prefix=2)  # toff == t_i exactly
    cases["notime"] = dict(n=65, K=5, seed=14, lag=LAG, point_notime=True)
    cases["acc_ms2"] = dict(n=65, K=5, seed=15, lag=LAG, acc_in_g=False)
    cases["acc_large"] = dict(n=65, K=5, seed=16, lag=LAG, rest_acc=(0.1, -0.2, 9.6))         # acc_in_g set, but |mean_acc| >= 2: the scale stays 1
    return cases


def filter_options(kw):
    return dict(ext=ext_default(), cov_acc=0.1, cov_gyr=0.2, cov_bias_gyr=1e-4, cov_bias_acc=2e-4, acc_in_g=kw.get("acc_in_g", True), point_notime=kw.get("point_notime", False))


def run_case(f, kw, t_end=100.0):
    """Initialise `f` (a checker or a vxba.ImuEkf made with filter_options(kw)) and process the case: (case, state handed in, cov handed in, result)."""
    kw = dict(kw)
    rest_acc = kw.pop("rest_acc", (0.01, -0.02, 0.98))
    kw.pop("acc_in_g", None); kw.pop("point_notime", None)
    st, _ = initialise(f, t_end=t_end, lag=kw.get("lag", 0.0), acc=rest_acc)
    c = make_case(t_end=t_end, **kw)
    state = moving_state(st[21:24]); cov = moving_cov()
    return c, state, cov, f.process(state, cov, c["scan"], c["imus"], c["beg"], c["end"])


# the scan of the filter test (800 points that a 3 m grid brings below 500) and its (size, min_points, half size used) rows; the refusal test's scans
FILTER_CASE = dict(n=800, K=5, seed=21, lag=LAG, ties=True, prefix=3)
FILTER_PASSES = ((3.0, 500, True), (3.0, 100, False), (0.1, 500, False), (1e-4, 0, False))
REFUSAL_CASE = dict(n=257, K=5, seed=31, lag=LAG, ties=True, prefix=3)
REFUSAL_NEXT = dict(n=257, K=5, seed=32)


def bad_calls(c, last_end, lag):
    """name -> arguments (scan, imus, beg, end) of a call that must be turned away, built from a good case."""
    xyz, toff = c["scan"]; st, gy, ac = c["imus"]; K = st.shape[0]
    nan_g = gy.copy(); nan_g[1, 2] = np.nan
    inf_a = ac.copy(); inf_a[0, 0] = np.inf
    nan_x = xyz.copy(); nan_x[5, 1] = np.nan
    inf_t = toff.copy(); inf_t[-1] = np.inf
    unsorted = toff.copy(); unsorted[[10, 20]] = unsorted[[20, 10]]
    back = st.copy(); back[[1, 3]] = back[[3, 1]]
    early = last_end - lag + lag * np.arange(1, K + 1) / (K + 2)                          # every message before the last scan end
    many = (last_end + 0.1 * np.arange(1, 71) / 70, np.tile(gy[0], (70, 1)), np.tile(ac[0], (70, 1)))
    return {
        "n = 0": ((xyz[:0], toff[:0]), c["imus"], c["beg"], c["end"]),
        "K = 0": (c["scan"], (st[:0], gy[:0], ac[:0]), c["beg"], c["end"]),
        "NaN rate": (c["scan"], (st, nan_g, ac), c["beg"], c["end"]),
        "inf acc": (c["scan"], (st, gy, inf_a), c["beg"], c["end"]),
        "NaN stamp": (c["scan"], (np.where(np.arange(K) == 2, np.nan, st), gy, ac), c["beg"], c["end"]),
        "NaN point": ((nan_x, toff), c["imus"], c["beg"], c["end"]),
        "inf toff": ((xyz, inf_t), c["imus"], c["beg"], c["end"]),
        "NaN end": (c["scan"], c["imus"], c["beg"], np.nan),
        "time regress": (c["scan"], c["imus"], last_end - 0.0101, c["end"]),
        "no surviving pair": (c["scan"], (early, gy, ac), c["beg"], c["end"]),
        "toff unsorted": ((xyz, unsorted), c["imus"], c["beg"], c["end"]),
        "stamps go back": (c["scan"], (back, gy, ac), c["beg"], c["end"]),
        "more than 64 heads": (c["scan"], many, c["beg"], c["end"]),
    }
