"""Numpy model of the initialisation's scan-to-cloud odometry (include/vxba.h: vxba_initodom_*): the CHECKER of tests/test_gpu_init.py and
of tests/test_init_cpu.py, never the thing run.

``lio_state_estimation_kdtree`` (voxelslam.cpp:960-1098) written against the reference's text: per scan point the world point, the five
nearest points of the world cloud, the plane ``direct . x = -1`` through them by least squares, the 0.1 gate, one Jacobian row; the
15-dimensional iterated EKF with ``K_1 = (H_T_H + cov^-1 / 1000)^-1``; the refind / rematch schedule; the append and the 0.5 m voxel filter.

Every quantity a decision rests on is formed by the same sequence of roundings as csrc/vxba_init_math.hpp forms it: the world point as
``((R0 x + R1 y) + R2 z) + t`` in float64, the query and the cloud in float32, the squared distance ``(dx dx + dy dy) + dz dz`` by numpy
float32 operations, candidates ordered by (distance, index).  The fit is ``numpy.linalg.lstsq`` and the inversions ``numpy.linalg.inv``:
those agree with the product to rounding, not bit for bit, and tests/test_init_cpu.py asserts that no decision of a session the GPU
tests use hangs on that difference.

The reference's own function cannot be compiled as a pin: the kd-tree stand-in under oracle/shim answers K = 1 only.
"""
import numpy as np

from tests import _oracle as O

NMATCH = 5
GATE = 0.1
SEED_MIN = 100
NUM_MAX_ITER = 4
FILTER = 0.5


# ---- search ----------------------------------------------------------------------------------------------------------------------
def sqdist(cloud, q):
    """float32 ((dx dx + dy dy) + dz dz) of every cloud point to one float32 query."""
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float32)
    dx, dy, dz = c[:, 0] - q[0], c[:, 1] - q[1], c[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def knn(cloud, queries, k=NMATCH, with_next=False):
    """Exact k nearest by (float32 distance, index) ascending: idx (n, k) with -1 beyond the cloud's size, sqd (n, k) with +inf there.
    with_next: also the distance of neighbour k + 1 (inf if none)."""
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)
    qs = np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    n, M = qs.shape[0], c.shape[0]
    idx = np.full((n, k), -1, dtype=np.int32); sqd = np.full((n, k), np.inf, dtype=np.float32); nxt = np.full(n, np.inf, dtype=np.float32)
    kk = min(k + 1, M)
    if kk == 0:
        return (idx, sqd, nxt) if with_next else (idx, sqd)
    cx, cy, cz = c[:, 0][None, :], c[:, 1][None, :], c[:, 2][None, :]
    B = max(1, min(n, (1 << 22) // max(M, 1)))
    for i0 in range(0, n, B):
        q = qs[i0:i0 + B]
        dx, dy, dz = cx - q[:, 0:1], cy - q[:, 1:2], cz - q[:, 2:3]
        D = (dx * dx + dy * dy) + dz * dz                                 # float32 throughout
        part = np.argpartition(D, kk - 1, axis=1)[:, :kk] if kk < M else np.broadcast_to(np.arange(M), (q.shape[0], M))
        cut = np.take_along_axis(D, part, axis=1).max(axis=1)
        for r in range(q.shape[0]):
            cand = part[r]
            if np.count_nonzero(D[r] <= cut[r]) != kk:                    # ties of the cut: all of them compete, the index order decides
                cand = np.nonzero(D[r] <= cut[r])[0]
            dc = D[r, cand]
            order = cand[np.lexsort((cand, dc))]
            m = min(k, order.size)
            idx[i0 + r, :m] = order[:m]; sqd[i0 + r, :m] = D[r, order[:m]]
            if order.size > k:
                nxt[i0 + r] = D[r, order[k]]
    return (idx, sqd, nxt) if with_next else (idx, sqd)


# ---- per-point arithmetic ---------------------------------------------------------------------------------------------------------
def world_points(state, pnt):
    s = np.asarray(state, dtype=np.float64)
    p = np.asarray(pnt, dtype=np.float64).reshape(-1, 3)
    return np.stack([((s[r] * p[:, 0] + s[3 + r] * p[:, 1]) + s[6 + r] * p[:, 2]) + s[9 + r] for r in range(3)], axis=1)


def fit_plane(A):
    """direct of A direct = -1 (least squares), the worst gate residual, and the singular-value ratio of A."""
    A = np.asarray(A, dtype=np.float64).reshape(NMATCH, 3)
    direct, _, _, sv = np.linalg.lstsq(A, -np.ones(NMATCH), rcond=None)
    worst = np.max(np.abs(A @ direct + 1.0))
    return direct, worst, sv[-1] / sv[0]


def jac_row(state, p, n, d, w):
    R = np.asarray(state[:9]).reshape(3, 3).T
    u = R.T @ n
    return np.concatenate([np.cross(p, u), n]), -(n @ w + d)


# ---- state algebra (IMUST, tools.hpp:135-199) -------------------------------------------------------------------------------------
def so3_exp(w):
    a = np.linalg.norm(w)
    if not a >= 1e-11:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * K @ K


def so3_log(R):
    tr = np.trace(R)
    theta = 0.0 if tr > 3.0 - 1e-6 else np.arccos(0.5 * (tr - 1))
    K = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 0.5 * K if abs(theta) < 0.001 else 0.5 * theta / np.sin(theta) * K


def state_minus(a, b):
    """a - b: [Log(b.R^T a.R), a.p - b.p, v, bg, ba]"""
    Ra, Rb = a[:9].reshape(3, 3).T, b[:9].reshape(3, 3).T
    return np.concatenate([so3_log(Rb.T @ Ra), a[9:21] - b[9:21]])


def state_plus(s, dx):
    out = s.copy()
    out[:9] = (s[:9].reshape(3, 3).T @ so3_exp(dx[:3])).T.reshape(9)
    out[9:21] = s[9:21] + dx[3:15]
    return out


# ---- the odometry -----------------------------------------------------------------------------------------------------------------
class InitOdometryRef:
    """Same call shapes as vxba.InitOdometry.  ``trace`` of the last step: per refind the margins the CPU suite asserts."""

    def __init__(self):
        self.cloud_ = np.zeros((0, 3), dtype=np.float32)
        self.records = {}

    def clear(self):
        self.cloud_ = np.zeros((0, 3), dtype=np.float32)

    def cloud_size(self):
        return self.cloud_.shape[0]

    def cloud(self):
        return self.cloud_.copy()

    def search(self, queries):
        return knn(self.cloud_, queries)

    def step(self, pnt_body, state, cov):
        pnt = np.asarray(pnt_body, dtype=np.float64).reshape(-1, 3)
        x = np.asarray(state, dtype=np.float64).copy()
        cov = np.asarray(cov, dtype=np.float64).reshape(15, 15).copy()
        self.records = {}
        if self.cloud_.shape[0] < SEED_MIN:
            self.cloud_ = np.concatenate([self.cloud_, world_points(x, pnt).astype(np.float32)])
            return {"seeded": True, "state": x, "cov": cov, "iterations": 0, "valid": [], "rematch_num": 0, "refind": [], "sweeps": []}
        n = pnt.shape[0]
        x_prop = x.copy()
        cov_inv = np.linalg.inv(cov)
        G = np.zeros((15, 15)); H_T_H = np.zeros((15, 15))
        ok = np.zeros(n, dtype=bool); nrm = np.zeros((n, 3)); ds = np.zeros(n)
        refind, converged_once, rematch_num = True, False, 0
        valid_tr, refind_tr, sweeps = [], [], []
        for it in range(NUM_MAX_ITER):
            wld = world_points(x, pnt)
            if refind:
                idx, sqd, nxt = knn(self.cloud_, wld.astype(np.float32), with_next=True)
                worst = np.zeros(n); svr = np.zeros(n)
                for i in range(n):
                    A = self.cloud_[idx[i]].astype(np.float64)
                    direct, worst[i], svr[i] = fit_plane(A)
                    ok[i] = worst[i] <= GATE
                    d = 1.0 / np.linalg.norm(direct)
                    nrm[i] = direct * d; ds[i] = d
                self.records[it] = {"nn": idx.copy(), "ok": ok.copy(), "n": nrm.copy(), "d": ds.copy(), "worst": worst, "sv_ratio": svr, "sqd5": sqd[:, NMATCH - 1].copy(),
                                    "sqd6": nxt}
            refind_tr.append(refind)
            HTH = np.zeros((6, 6)); HTz = np.zeros(6)
            for i in np.nonzero(ok)[0]:
                j, r = jac_row(x, pnt[i], nrm[i], ds[i], wld[i])
                HTH += np.outer(j, j); HTz += j * r
            valid = int(ok.sum())
            valid_tr.append(valid); sweeps.append({"HTH": HTH, "HTz": HTz, "match_num": valid})
            H_T_H[:6, :6] = HTH
            K_1 = np.linalg.inv(H_T_H + cov_inv / 1000)
            G[:, :6] = K_1[:, :6] @ HTH
            vec = state_minus(x_prop, x)
            sol = K_1[:, :6] @ HTz + vec - G[:, :6] @ vec[:6]
            x = state_plus(x, sol)
            refind = False
            if np.linalg.norm(sol[:3]) * 57.3 < 0.01 and np.linalg.norm(sol[3:6]) * 100 < 0.015:
                refind = True; converged_once = True; rematch_num += 1
            if it == NUM_MAX_ITER - 2 and not converged_once:
                refind = True
            if rematch_num >= 2 or it == NUM_MAX_ITER - 1:
                cov = (np.eye(15) - G) @ cov
                break
        self.cloud_ = O.down_sampling_voxel(np.concatenate([self.cloud_, world_points(x, pnt).astype(np.float32)]), FILTER)
        return {"seeded": False, "state": x, "cov": cov, "iterations": it + 1, "valid": valid_tr, "rematch_num": rematch_num, "refind": refind_tr, "sweeps": sweeps}

    def inspect(self, iteration):
        return self.records[iteration]


# ---- honesty of a session: no decision may hang on the checker-vs-product rounding ---------------------------------------------------
def near_tie_share(rec, ulps=4):
    """Share of points whose 5th and 6th neighbour distances lie within `ulps` float32 ulps of each other."""
    d5, d6 = rec["sqd5"], rec["sqd6"]
    fin = np.isfinite(d6)
    gap = np.abs(d6[fin] - d5[fin])
    return float(np.mean(gap <= ulps * np.spacing(np.maximum(d5[fin], d6[fin])))) if fin.any() else 0.0


def near_tie_mask(rec, ulps=4):
    d5, d6 = rec["sqd5"], rec["sqd6"]
    return np.isfinite(d6) & (np.abs(d6 - d5) <= ulps * np.spacing(np.maximum(d5, d6)))


# ---- sessions the tests share ------------------------------------------------------------------------------------------------------
def make_room(n_points, seed, extent=8.0, noise=0.005, clutter=0.05):
    """World points on the six faces of a box of half-size `extent` (a planes-plus-clutter scene), float64."""
    rng = np.random.default_rng(seed)
    face = rng.integers(0, 6, n_points)
    uv = rng.uniform(-extent, extent, (n_points, 2))
    pts = np.zeros((n_points, 3))
    for f in range(6):
        m = face == f
        ax, sgn = f // 2, 1.0 if f % 2 else -1.0
        o = [a for a in range(3) if a != ax]
        pts[m, ax] = sgn * extent + rng.normal(0, noise, m.sum())
        pts[m, o[0]] = uv[m, 0]; pts[m, o[1]] = uv[m, 1]
    c = rng.random(n_points) < clutter
    pts[c] = rng.uniform(-extent, extent, (int(c.sum()), 3))
    return pts


def pack_state(R, p):
    s = np.zeros(24)
    s[:9] = np.asarray(R).T.reshape(9); s[9:12] = p; s[21:24] = [0, 0, -9.8]
    return s


def make_step_case(n_cloud=20000, n_scan=6000, seed=3, rot=0.01, tra=0.05, extent=8.0):
    """A seed scan (identity pose) that becomes the cloud, and a scan of the same room taken from a known pose, with a propagated state off the
    truth by (rot rad, tra m): dict(seed_pts, scan_body, state_true, state_init, cov)."""
    rng = np.random.default_rng(seed + 1000)
    seed_pts = make_room(n_cloud, seed, extent)
    a = rng.normal(size=3); a *= 0.2 / np.linalg.norm(a)
    R_true = so3_exp(a); p_true = rng.uniform(-0.5, 0.5, 3)
    wld = make_room(n_scan, seed + 1, extent)
    body = (wld - p_true) @ R_true                       # R^T (w - p)
    e = rng.normal(size=3); e *= rot / np.linalg.norm(e)
    t = rng.normal(size=3); t *= tra / np.linalg.norm(t)
    cov = np.diag(np.concatenate([np.full(3, 1e-4), np.full(3, 1e-2), np.full(3, 1e-2), np.full(3, 1e-6), np.full(3, 1e-4)]))
    return dict(seed_pts=seed_pts, scan_body=body, state_true=pack_state(R_true, p_true), state_init=pack_state(R_true @ so3_exp(e), p_true + t), cov=cov)


def make_window_case(n_steps=5, n_scan=1500, seed=11, extent=6.0):
    """n_steps scans of one room from a slowly moving pose, each with a propagated state slightly off: list of dict(scan_body, state_init, cov)."""
    rng = np.random.default_rng(seed + 2000)
    out = []
    for k in range(n_steps):
        a = np.array([0.01, -0.02, 0.03]) * k
        R = so3_exp(a); p = np.array([0.08, 0.05, -0.02]) * k
        wld = make_room(n_scan, seed + 10 * k, extent)
        e = rng.normal(size=3) * 0.002; t = rng.normal(size=3) * 0.01
        if k == 0:
            e[:] = 0; t[:] = 0
        cov = np.diag(np.concatenate([np.full(3, 1e-4), np.full(3, 1e-2), np.full(3, 1e-2), np.full(3, 1e-6), np.full(3, 1e-4)]))
        out.append(dict(scan_body=(wld - p) @ R, state_init=pack_state(R @ so3_exp(e), p + t), state_true=pack_state(R, p), cov=cov))
    return out


_CACHE = {}


def reference_step():
    """The one-step session of the GPU tests through the checker, computed once per process: dict(case, seed, result, records, cloud_before, cloud_after)."""
    if "step" not in _CACHE:
        case = make_step_case()
        ref = InitOdometryRef()
        seed = ref.step(case["seed_pts"], pack_state(np.eye(3), np.zeros(3)), case["cov"])
        before = ref.cloud()
        res = ref.step(case["scan_body"], case["state_init"], case["cov"])
        _CACHE["step"] = dict(case=case, seed=seed, result=res, records=ref.records, cloud_before=before, cloud_after=ref.cloud())
    return _CACHE["step"]


def reference_window():
    """The five-step session of the GPU tests through the checker, computed once per process: per step dict(inp, result, records, cloud)."""
    if "window" not in _CACHE:
        ref = InitOdometryRef()
        out = []
        for inp in make_window_case():
            res = ref.step(inp["scan_body"], inp["state_init"], inp["cov"])
            out.append(dict(inp=inp, result=res, records=ref.records, cloud=ref.cloud()))
        _CACHE["window"] = out
    return _CACHE["window"]


# ---- motion_init's pieces (voxelslam.cpp:461-561, preintegration.hpp:50-73) ----------------------------------------------------------------
def exp_rate(w, dt):
    """Exp(ang_vel, dt) of tools.hpp:68-84."""
    a = np.linalg.norm(w)
    if not a > 1e-7:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a * dt) * K + (1.0 - np.cos(a * dt)) * K @ K


def pose_table(stamps, gyr, acc, beg_time, xc, bias_from, scale=1.0):
    """imu_poses of motion_blur (:495-521): list of dict(t, R, p, v, w, a), heads K-2 .. 0, integrated backward from xc with bias_from's biases."""
    R = xc[:9].reshape(3, 3).T.copy(); p = xc[9:12].copy(); v = xc[12:15].copy(); g = xc[21:24]
    bg, ba = bias_from[15:18], bias_from[18:21]
    out = []
    for t in range(len(stamps) - 1, 0, -1):
        w = 0.5 * (gyr[t - 1] + gyr[t]) - bg
        a = 0.5 * (acc[t - 1] + acc[t]) * scale - ba
        dt = stamps[t - 1] - stamps[t]
        E = exp_rate(w, dt)
        acc_imu = R @ a + g
        p = p + v * dt + 0.5 * acc_imu * dt * dt
        v = v + acc_imu * dt
        R = R @ E
        out.append(dict(t=stamps[t - 1] - beg_time, R=R.copy(), p=p.copy(), v=v.copy(), w=w.copy(), a=acc_imu.copy()))
    return out


def pose_table_rows(tab):
    return np.array([np.concatenate([[e["t"]], e["R"].T.reshape(9), e["p"], e["v"], e["w"], e["a"]]) for e in tab]).reshape(-1, 22)


def motion_blur(xyz, toff, stamps, gyr, acc, beg_time, xc, bias_from, ext, scale=1.0, point_notime=False):
    """A literal replay of motion_blur's loops (:523-560): (points m x 3, src m)."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    eR, ep = ext[:9].reshape(3, 3).T, ext[9:12]
    if point_notime:
        return world_points(ext, xyz), np.arange(xyz.shape[0], dtype=np.int32)
    toff = np.asarray(toff, dtype=np.float32)
    tab = pose_table(stamps, gyr, acc, beg_time, xc, bias_from, scale)
    xR, xp = xc[:9].reshape(3, 3).T, xc[9:12]
    out, src = [], []
    it = xyz.shape[0] - 1
    if it < 0:
        return np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
    for head in tab:
        while float(toff[it]) > head["t"]:
            dt = float(toff[it]) - head["t"]
            R_i = head["R"] @ exp_rate(head["w"], dt)
            T_ei = head["p"] + head["v"] * dt + 0.5 * head["a"] * dt * dt - xp
            out.append(xR.T @ (R_i @ (eR @ xyz[it] + ep) + T_ei)); src.append(it)
            if it == 0:
                break
            it -= 1
    return np.array(out).reshape(-1, 3), np.array(src, dtype=np.int32)


def push_imu_samples(stamps, gyr, acc, bg, ba, scale=1.0):
    """What push_imu (preintegration.hpp:50-73) feeds add_imu: (gyr K-1 x 3, acc K-1 x 3, dt K-1)."""
    g = 0.5 * (gyr[:-1] + gyr[1:]) - bg
    a = 0.5 * (acc[:-1] + acc[1:]) * scale - ba
    return g, a, np.diff(stamps)


def align_gravity(states):
    """align_gravity (:461-486) on W x 24 states: g of state 0 turned onto +-z, everything rotated about p of state 0."""
    xs = np.asarray(states, dtype=np.float64).copy()
    g0 = xs[0, 21:24].copy()
    n0 = g0 / np.linalg.norm(g0)
    n1 = np.array([0.0, 0.0, -1.0 if n0[2] < 0 else 1.0])
    rv = np.cross(n0, n1); rn = np.linalg.norm(rv); rv = rv / rn
    ang = np.arcsin(rn)
    K = np.array([[0, -rv[2], rv[1]], [rv[2], 0, -rv[0]], [-rv[1], rv[0], 0]])
    rot = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K          # Eigen::AngleAxisd(asin(rnorm), rotvec).matrix()
    g0 = rot @ g0
    p0 = xs[0, 9:12].copy()
    for s in xs:
        s[9:12] = rot @ (s[9:12] - p0) + p0
        s[:9] = (rot @ s[:9].reshape(3, 3).T).T.reshape(9)
        s[12:15] = rot @ s[12:15]
        s[21:24] = g0
    return xs


def make_motion_scan(n, K=7, seed=0, span=0.1, rate=(0.4, -0.3, 0.5), v0=(1.0, -0.5, 0.3), t_lo=None):
    """A scan taken DURING a motion that mid-point integration reproduces to rounding: constant body rate, ballistic translation (world acceleration = g,
    so the accelerometer reads its bias), K IMU messages over `span` seconds, points on the plane z = 2 seen through a non-trivial extrinsic at their own
    time.  dict(xyz float32 LiDAR frame, toff float32 ascending, stamps, gyr, acc, beg_time, xc (the state at the LAST message), bias_from, ext, wld: the planted
    plane points, meas: the world points the float32-rounded measurements name)."""
    rng = np.random.default_rng(seed)
    w = np.array(rate); g = np.array([0.0, 0.0, -9.8]); bg = np.array([0.01, -0.02, 0.005]); ba = np.array([0.05, 0.02, -0.03])
    beg = 100.0
    stamps = beg + np.linspace(0.0, span, K)
    R0 = so3_exp(np.array([0.1, 0.2, -0.1])); p0 = np.array([0.5, -0.2, 0.1]); v0 = np.array(v0)

    def pose(t):                                                               # t seconds after beg
        return R0 @ exp_rate(w, t), p0 + v0 * t + 0.5 * g * t * t, v0 + g * t
    gyr = np.tile(w + bg, (K, 1)); acc = np.tile(ba, (K, 1))
    Re, pe, ve = pose(span)
    xc = np.concatenate([Re.T.reshape(9), pe, ve, bg, ba, g])
    eR = so3_exp(np.array([0.02, -0.03, 0.5])); ep = np.array([0.1, 0.05, -0.02])
    ext = np.concatenate([eR.T.reshape(9), ep])
    lo = -0.2 * span if t_lo is None else t_lo
    toff = np.sort(rng.uniform(lo, span, n)).astype(np.float32)
    wld = np.column_stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), np.full(n, 2.0)])
    xyz = np.zeros((n, 3))
    for i in range(n):
        Ri, pi, _ = pose(float(toff[i]))
        xyz[i] = eR.T @ (Ri.T @ (wld[i] - pi) - ep)
    xyz = xyz.astype(np.float32)                                               # the measurement is float32: `meas` is the world point it really names
    meas = np.array([pose(float(toff[i]))[0] @ (eR @ xyz[i].astype(np.float64) + ep) + pose(float(toff[i]))[1] for i in range(n)]).reshape(-1, 3)
    return dict(xyz=xyz, toff=toff, stamps=stamps, gyr=gyr, acc=acc, beg_time=beg, xc=xc, bias_from=xc.copy(), ext=ext, wld=wld, meas=meas)


# ---- motion_init itself (voxelslam.cpp:563-713) ----------------------------------------------------------------------------------------------
def calc_body_var(pb, dept_err, beam_err):
    """calcBodyVar (voxelslam.hpp:164-185): (the point with a zero z rewritten, its 3 x 3 variance).  range, range_inc and degree_inc are float upstream."""
    pb = np.array(pb, dtype=np.float64)
    if pb[2] == 0:
        pb[2] = 0.0001
    rng_ = float(np.float32(np.linalg.norm(pb)))
    range_var = float(np.float32(dept_err) * np.float32(dept_err))
    dir_var = np.sin(float(np.float32(beam_err)) * 0.017453293) ** 2
    d = pb / np.linalg.norm(pb)
    hat = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])
    b1 = np.array([1.0, 1.0, -(d[0] + d[1]) / d[2]]); b1 /= np.linalg.norm(b1)
    b2 = np.cross(b1, d); b2 /= np.linalg.norm(b2)
    A = rng_ * hat @ np.column_stack([b1, b2])
    return pb, np.outer(d, d) * range_var + A @ (dir_var * np.eye(2)) @ A.T


def pvec_update(pnt, var, state, cov):
    """pvec_update (voxelslam.hpp:203-215): (world variances n x 3 x 3, world points n x 3)."""
    R, p = state[:9].reshape(3, 3).T, state[9:12]
    rot_var, tsl_var = cov[0:3, 0:3], cov[3:6, 3:6]
    out = np.zeros((len(pnt), 3, 3))
    for k, (q, V) in enumerate(zip(pnt, var)):
        H = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
        out[k] = R @ V @ R.T + H @ rot_var @ H.T + tsl_var
    return out, world_points(state, pnt)


def normal_scatter(eig_vec):
    """sum of n n^T over eig_vectors[k].col(0) of a factor cache (n x 9 column-major)."""
    n = np.asarray(eig_vec).reshape(-1, 9)[:, :3]
    return n.T @ n


def motion_init(sess, map_kw, imu_coef=1e-4, dept_err=0.02, beam_err=0.05, point_notime=False, states=None, blobs=None):
    """A replay of motion_init on the oracles.  map_kw: voxel_size, max_layer, min_point, min_eigen_value, plane_eigen_value_thre (the caller's), max_points.
    Returns dict(flag, states, blobs, rounds: list of dict(n_vox, resis, g, ratio, phase, trace, fired), eig, leaves (None when the flag is 0), hess)."""
    from tests import _oracle as O
    W = sess.win_size
    x = np.array(sess.states_init if states is None else states, dtype=np.float64).copy()
    scale = sess.imupre_scale_gravity

    def preint(i):                                                              # factor i - 1: x[i - 1]'s biases, scan i's messages
        st, gy, ac = sess.imus[i]
        g, a, dt = push_imu_samples(st, gy, ac, x[i - 1, 15:18], x[i - 1, 18:21], scale)
        return O.imu_preintegrate([(g, a, dt)], sess.noise_meas, sess.noise_walk, x[i - 1, 15:18], x[i - 1, 18:21])[0]
    bl = np.stack([preint(i) for i in range(1, W)]) if blobs is None else np.array(blobs, dtype=np.float64).copy()
    flag, thre, degrade, eig, rounds, mo, fo, hess = 0, 0.05, True, np.zeros(3), [], None, None, None
    for it in range(10):
        kw = dict(map_kw)
        if not flag:
            kw.update(min_eigen_value=0.02, plane_eigen_value_thre=(0.25,) * 4)
        mo = O.LocalMapOracle(win_size=W, thread_num=1, **kw)
        for i in range(W):
            xyz, toff = sess.scans[i]
            st, gy, ac = sess.imus[i]
            body, _ = motion_blur(xyz, toff, st, gy, ac, sess.beg_times[i], x[i], x[max(i - 1, 0)], sess.ext, scale, point_notime)
            if flag:
                pv = [calc_body_var(q, dept_err, beam_err) for q in body]
                body = np.array([a for a, _ in pv]).reshape(-1, 3)
                var, pw = pvec_update(body, [b for _, b in pv], x[i], sess.covs[i])
            else:
                var, pw = np.tile(np.eye(3), (len(body), 1, 1)), world_points(x[i], body)
            mo.cut_voxel(i, body, var, pw)
        fo = O.Oracle(W)
        mo.recut(W, x[:, :12].copy(), fo)
        rec = dict(n_vox=fo.size(), phase=flag, thre=thre, fired=False, resis=None, g=None, ratio=None, trace=None)
        rounds.append(rec)
        if fo.size() < 10:
            break
        r = O.li_damping_iter_gravity(fo, x, bl, max_iter=3, thd_num=1, imu_coef=imu_coef)
        x, hess = r["states"], r["hess"]
        ratio = abs(r["resis"][0] - r["resis"][1]) / r["resis"][0]
        rec.update(resis=r["resis"].copy(), g=x[0, 21:24].copy(), ratio=ratio, trace=r["trace"])
        bl = np.stack([preint(i) for i in range(1, W)])
        if ratio < thre and it >= 2:
            eig = np.linalg.eigvalsh(normal_scatter(fo.read_cache()[1]))
            degrade = eig[0] < 15
            thre = 0.01
            rec["fired"] = True
            if not flag:
                x = align_gravity(x)
                flag = 1
                continue
            break
    gn = np.linalg.norm(x[W - 1, 21:24])
    if degrade or gn < 9.6 or gn > 10.0:
        flag = 0
    leaves = mo.leaves() if flag else None
    return dict(flag=flag, states=x, blobs=bl, rounds=rounds, eig=eig, gnorm=gn, leaves=leaves, hess=hess, map=mo if flag else None, factor=fo if flag else None)


MOTION_MAP = dict(voxel_size=1.0, max_layer=2, min_point=(20, 20, 15, 10), min_eigen_value=0.0025, plane_eigen_value_thre=(1 / 4, 1 / 4, 1 / 4, 1 / 4), max_points=100)
# the sessions of the GPU tests: the smallest converging one, and the three exits
MOTION_SESSIONS = {
    "room": dict(win_size=6, pts_per_scan=1500),
    "parallel": dict(win_size=6, pts_per_scan=1500, scene="parallel"),
    "sparse": dict(win_size=6, pts_per_scan=300, scene="sparse"),
    "gravity": dict(win_size=6, pts_per_scan=1500, gravity_norm=10.3),
}


def motion_session(kind):
    from voxel_slam_amd import synth
    key = ("msess", kind)
    if key not in _CACHE:
        _CACHE[key] = synth.make_init_session(**MOTION_SESSIONS[kind])
    return _CACHE[key]


def reference_motion(kind):
    key = ("mref", kind)
    if key not in _CACHE:
        _CACHE[key] = motion_init(motion_session(kind), MOTION_MAP)
    return _CACHE[key]


# ---- initialization() after odom_ekf.process (voxelslam.cpp:1230-1288) -------------------------------------------------------------------------
def voxel_keys(xyz32, voxel_size):
    """Upstream's float-typed voxel index (tools.hpp:209-216): n x 3 int64."""
    loc = (xyz32.astype(np.float64) / voxel_size).astype(np.float32)
    loc = np.where(loc < 0, (loc.astype(np.float64) - 1.0).astype(np.float32), loc)
    return loc.astype(np.int64)


def down_sampling_close(xyz, voxel_size):
    """down_sampling_close (tools.hpp:240-302): per voxel the point nearest the voxel's mean; (points, their indices) in ascending voxel index."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    if voxel_size < 0.001:
        return xyz.copy(), np.arange(xyz.shape[0], dtype=np.int32)
    cells = {}
    for i, k in enumerate(map(tuple, voxel_keys(xyz, voxel_size))):
        cells.setdefault(k, []).append(i)
    sel = []
    for k in sorted(cells):
        ids = cells[k]
        pb = xyz[ids[0]].copy()
        for i in ids[1:]:
            pb += xyz[i]                                                        # float sums in cloud order
        pb /= np.float32(len(ids))
        ndis, best = 100.0, ids[0]
        for i in ids:
            d = (pb - xyz[i]).astype(np.float64)
            dis = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if dis < ndis:
                best, ndis = i, dis
        sel.append(best)
    sel = np.array(sel, dtype=np.int32)
    return xyz[sel], sel


def var_init_points(xyz32, ext):
    """The points of var_init (voxelslam.hpp:187-201): calcBodyVar's rewrite of a zero z, then the extrinsic."""
    p = np.asarray(xyz32, dtype=np.float32).astype(np.float64).reshape(-1, 3).copy()
    p[p[:, 2] == 0, 2] = 0.0001
    return world_points(ext, p)


def initializer(sess, map_kw, down_size=0.1, **kw):
    """The checker's driver: dict(returns: per scan, odom: the per-scan step results and records, states_in: what motion_init received, motion: its result)."""
    import types
    odo = InitOdometryRef()
    states, covs, scans, odom = [], [], [], []
    for i in range(sess.win_size):
        xyz, toff = sess.scans[i]
        cur = O.down_sampling_voxel(xyz, max(down_size, 0.5))
        r = odo.step(var_init_points(cur, sess.ext), sess.states_init[i], sess.covs[i])
        odom.append(dict(result=r, records=odo.records, cloud=odo.cloud()))
        states.append(r["state"]); covs.append(r["cov"])
        pts, sel = down_sampling_close(xyz, down_size)
        if pts.shape[0] < 1000:
            pts, sel = down_sampling_close(xyz, down_size / 2)
        o = np.argsort(toff[sel], kind="stable")
        scans.append((pts[o], toff[sel][o]))
    s2 = types.SimpleNamespace(**{**sess.__dict__, "scans": scans, "states_init": np.stack(states), "covs": np.stack(covs)})
    mot = motion_init(s2, map_kw, **kw)
    return dict(returns=[0] * (sess.win_size - 1) + [1 if mot["flag"] else -1], odom=odom, states_in=np.stack(states), covs_in=np.stack(covs), scans=scans, motion=mot)


def reference_initializer():
    key = "initializer"
    if key not in _CACHE:
        _CACHE[key] = initializer(motion_session("room"), MOTION_MAP)
    return _CACHE[key]
