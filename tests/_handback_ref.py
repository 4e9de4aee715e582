"""numpy / pure-Python CHECKER of the loop hand-back (include/vxba.h ``vxba_kfarchive_*``, voxel_slam_amd/handback.py): a loop-by-loop replay of the
four functions of the reference it restates --

  loop_update        voxelslam.cpp:1101-1186   dx on every window state, x_curr, the path, the buffered scans; the g_update rule
  keyframe_loading   :1189-1228                the radius search over the float32 snapshot, the skip-not-stop walk, one keyframe per call
  the loop thread    :2100-2168                x0 by id, dx from the newest scan pose before and after, the cumulative pvec_tem, arming the history
  ScanPose::update   loop_refine.hpp:29-34

Every sum is written out on float64 scalars -- ``((R00 v0 + R01 v1) + R02 v2) + p0`` -- and never goes through ``@``, which may fuse: the GPU does the
same IEEE operations in the same order without contraction, so the comparison is for EQUALITY.  The float32 distances are float32 scalar operations.
``degrade`` switches one of the deliberate mistakes on (tests/test_handback_cpu.py shows the criteria reject each of them).
"""
import numpy as np

F32 = np.float32


def world_point(pose, v):
    """x0.R double(v) + x0.p for a pose record [R column-major 9 | p 3]: three scalar sums, written out."""
    v0, v1, v2 = float(v[0]), float(v[1]), float(v[2])
    p = [float(x) for x in pose]
    return [((p[0] * v0 + p[3] * v1) + p[6] * v2) + p[9],
            ((p[1] * v0 + p[4] * v1) + p[7] * v2) + p[10],
            ((p[2] * v0 + p[5] * v1) + p[8] * v2) + p[11]]


def world_cloud(pose, xyz):
    """The loop over a cloud (float32 keyframe points widen exactly)."""
    out = np.zeros((len(xyz), 3))
    for j in range(len(xyz)):
        out[j] = world_point(pose, xyz[j])
    return out


def world_cloud_vec(pose, xyz):
    """The vectorised restatement: the same three sums on float64 columns."""
    v = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(pose, dtype=np.float64)
    return np.stack([((p[i] * v[:, 0] + p[3 + i] * v[:, 1]) + p[6 + i] * v[:, 2]) + p[9 + i] for i in range(3)], axis=1)


def rotate_var(pose, var):
    """R var R^T -- what the reference does NOT do; only the degraded checker uses it."""
    R = np.asarray(pose[:9]).reshape(3, 3).T
    return np.einsum("ij,njk,lk->nil", R, var, R)


class Archive:
    """The reference's ``keyframes`` vector with what the loop thread and keyframe_loading do to it."""

    def __init__(self, degrade=None):
        self.kf = []                 # dict(id, x0, jour, cloud (n, 6) float32, exist)
        self.snap = np.zeros((0, 3), dtype=F32)
        self.history_kfsize = 0
        self.degrade = degrade

    def add(self, kf_id, pose, jour, down_xyzv):
        self.kf.append(dict(id=int(kf_id), x0=np.array(pose, dtype=np.float64), jour=float(jour), cloud=np.array(down_xyzv, dtype=F32).reshape(-1, 6), exist=0))

    def set_poses(self, x0):
        for k, kf in enumerate(self.kf):
            kf["x0"] = np.array(x0[k], dtype=np.float64)

    def exist(self):
        return np.array([kf["exist"] for kf in self.kf], dtype=np.int32)

    def arm_history(self, init_num=5):
        K = len(self.kf)
        self.history_kfsize = 0
        for i in range(K - init_num, K):
            if i < 0:
                continue
            self.kf[i]["exist"] = 0
        if K > init_num:
            snap = []
            for i in range(K - init_num):
                self.kf[i]["exist"] = 1
                snap.append([F32(self.kf[i]["x0"][9]), F32(self.kf[i]["x0"][10]), F32(self.kf[i]["x0"][11])])
            self.snap = np.array(snap, dtype=F32).reshape(-1, 3)
            self.history_kfsize = len(snap)

    def distances(self, p_curr):
        """float32 squared distances from float(p_curr) to every snapshot position: (dx dx + dy dy) + dz dz."""
        if self.degrade == "f64_distances":
            d = self.snap.astype(np.float64) - np.asarray(p_curr, dtype=np.float64)
            return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        pc = [F32(p_curr[0]), F32(p_curr[1]), F32(p_curr[2])]
        out = np.zeros(len(self.snap), dtype=F32)
        for k in range(len(self.snap)):
            dx, dy, dz = F32(self.snap[k, 0] - pc[0]), F32(self.snap[k, 1] - pc[1]), F32(self.snap[k, 2] - pc[2])
            out[k] = F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))
        return out

    def load_near(self, p_curr, radius=10.0):
        """keyframe_loading: (k, world points) of the keyframe loaded, or (-1, None)."""
        if self.history_kfsize <= 0:
            return -1, None
        d2 = self.distances(p_curr)
        r2 = F32(radius * radius) if self.degrade != "f64_distances" else radius * radius
        cand = [k for k in range(len(d2)) if d2[k] < r2]
        cand.sort(key=lambda k: (d2[k], k))              # ascending d2, ties by the lowest index
        for k in cand:
            kf = self.kf[k]
            if kf["exist"]:
                kf["exist"] = 0
                self.history_kfsize -= 1
                return k, world_cloud(kf["x0"], kf["cloud"][:, :3])
            if self.degrade == "stop_at_first":
                break
        return -1, None

    def map_loop(self, init_num=5, cumulative=True, pending=()):
        """:2131-2150 followed by the buffered scans of :1161-1168 (``pending``: (pose, body points (n, 3) f64, var (n, 3, 3) or None)).  Returns
        (cloud_ptr, points, variances (N, 3, 3)) with the clouds concatenated in the order the map receives them."""
        if self.degrade == "not_cumulative":
            cumulative = False
        K = len(self.kf)
        pts, var, cptr = [], [], [0]
        tem_p, tem_v = [], []                            # pvec_tem, which upstream never clears
        for i in range(K - init_num, K):
            if i < 0:
                continue
            kf = self.kf[i]
            if not cumulative:
                tem_p, tem_v = [], []
            w = world_cloud(kf["x0"], kf["cloud"][:, :3])
            v = np.zeros((len(w), 3, 3))
            for j in range(3):
                v[:, j, j] = kf["cloud"][:, 3 + j].astype(np.float64)
            if self.degrade == "rotated_var":
                v = rotate_var(kf["x0"], v)
            tem_p.append(w); tem_v.append(v)
            pts.extend(tem_p); var.extend(tem_v)
            cptr.append(cptr[-1] + sum(len(x) for x in tem_p))
        for pose, body, pv in pending:
            body = np.asarray(body, dtype=np.float64).reshape(-1, 3)
            pts.append(world_cloud(pose, body))
            var.append(np.zeros((len(body), 3, 3)) if pv is None else np.asarray(pv, dtype=np.float64).reshape(-1, 3, 3))
            cptr.append(cptr[-1] + len(body))
        P = np.concatenate(pts) if pts else np.zeros((0, 3))
        V = np.concatenate(var) if var else np.zeros((0, 3, 3))
        return np.array(cptr, dtype=np.int64), P, V

    def clouds(self, cptr, P, V):
        """The lists ``LocalMap.loop_update`` takes."""
        return [P[cptr[c]:cptr[c + 1]] for c in range(len(cptr) - 1)], [V[cptr[c]:cptr[c + 1]] for c in range(len(cptr) - 1)]


# ---- dx and what loop_update does with it ----
def _R(rec):
    return [[float(rec[3 * j + i]) for j in range(3)] for i in range(3)]


def _mv(A, b):
    return [(A[i][0] * b[0] + A[i][1] * b[1]) + A[i][2] * b[2] for i in range(3)]


def _mm(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _T(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def loop_delta(x1, x3):
    """:2126-2128: (dx.R, dx.p) as nested lists / a list."""
    dR = _mm(_R(x3), _T(_R(x1)))
    t = _mv(dR, [float(x1[9]), float(x1[10]), float(x1[11])])
    return dR, [float(x3[9]) - t[0], float(x3[10]) - t[1], float(x3[11]) - t[2]]


def turn(dx, rec, with_g=False):
    """The x_buf loop of loop_update / ScanPose::update on one record."""
    dR, dp = dx
    out = np.array(rec, dtype=np.float64)
    R = _mm(dR, _R(rec))
    for i in range(3):
        for j in range(3):
            out[3 * j + i] = R[i][j]
    t = _mv(dR, [float(rec[9]), float(rec[10]), float(rec[11])])
    for i in range(3):
        out[9 + i] = t[i] + dp[i]
    if len(rec) >= 15:
        out[12:15] = _mv(dR, [float(x) for x in rec[12:15]])
    if with_g:
        out[21:24] = _mv(dR, [float(x) for x in rec[21:24]])
    return out


def loop_update(dx, scan_poses, states, x_curr, g_update, pending_poses=()):
    """The host half of loop_update: dict(states, x_curr, g_update, path, pending_poses)."""
    path = [[float(p[9]), float(p[10]), float(p[11])] for p in scan_poses]
    pend = []
    for bl in pending_poses:
        q = turn(dx, bl)
        pend.append(q)
        path.append(list(q[9:12]))
    st = []
    for x in states:
        q = turn(dx, x, with_g=(g_update == 1))
        st.append(q)
        path.append(list(q[9:12]))
    st = np.array(st).reshape(len(st), -1)
    xc = np.array(x_curr, dtype=np.float64)
    xc[:12] = st[-1, :12]
    xc[12:15] = _mv(dx[0], [float(x) for x in x_curr[12:15]])
    xc[21:24] = st[-1, 21:24]
    return dict(states=st, x_curr=xc, g_update=2 if g_update == 1 else g_update, path=np.array(path, dtype=np.float64).reshape(-1, 3).astype(F32), pending_poses=pend)


# ---- shared inputs of the CPU and GPU suites ----
def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose_rec(R, p):
    return np.concatenate([np.asarray(R, dtype=np.float64).T.reshape(9), np.asarray(p, dtype=np.float64)])


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 5)        # points per keyframe, cycled: every block boundary of the kernel, and an empty keyframe in range


MAP_LOOP_SEED = {0: 0, 1: 1, 4: 5, 5: 8, 6: 0, 9: 0}    # per K of the map_loop cases: the last five keyframes of the six cases together hold every size above


def make_keyframes(K, seed=0, sizes=SIZES, far=40.0):
    """K keyframes: (id, pose, jour, down (n, 6) float32).  Coordinates of both signs, poses tens of metres out, ids spaced like a window of 3 scans."""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for k in range(K):
        n = sizes[(k + seed) % len(sizes)]
        R = rodrigues(rng.normal(size=3) * 0.7)
        p = np.array([far * np.cos(0.9 * k), -far * np.sin(0.7 * k) + 3.0 * k, 2.0 * rng.normal()])
        xyz = rng.uniform(-6, 6, size=(n, 3))
        var = rng.uniform(1e-5, 1e-3, size=(n, 3))
        out.append((3 * k + 2, pose_rec(R, p), 0.5 * k, np.concatenate([xyz, var], axis=1).astype(F32)))
    return out


def fill(archive, kfs):
    for kid, pose, jour, down in kfs:
        archive.add(kid, pose, jour, down)
    return archive


def make_history(n_hist=8, init_num=5):
    """Keyframes whose positions script keyframe_loading: history keyframes on a line 4 m apart along x, except that keyframes 2 and 3 are MIRRORED
    about the plane x = 10 of the query used for the tie (x = 8 and x = 12: float32-exact, so the two d2 are equal bit for bit), followed by
    ``init_num`` recent keyframes far away.  Returns (kfs, steps): steps = list of (p_curr, what the step exercises)."""
    rng = np.random.default_rng(77)
    pos = [np.array([4.0 * k, 0.5 * (k % 3), 0.25 * k]) for k in range(n_hist)]
    pos[2] = np.array([8.0, 1.0, 0.5]); pos[3] = np.array([12.0, 1.0, 0.5])
    pos += [np.array([500.0 + 10 * j, 300.0, 0.0]) for j in range(init_num)]
    kfs = []
    for k, p in enumerate(pos):
        n = (7, 65, 0, 33, 12)[k % 5] if k != 2 else 9
        xyz = rng.uniform(-3, 3, size=(n, 3)); var = rng.uniform(1e-5, 1e-3, size=(n, 3))
        kfs.append((2 * k + 1, pose_rec(rodrigues(rng.normal(size=3) * 0.4), p), 0.1 * k, np.concatenate([xyz, var], axis=1).astype(F32)))
    steps = [
        (np.array([10.0 + 1e-7, 1.0, 0.5]), "tie between keyframes 2 and 3 once p_curr is float32 (in float64 keyframe 3 is nearer): the lower index loads"),
        (np.array([10.0, 1.0, 0.5]), "the nearest candidate (2) is already loaded: 3 loads"),
        (np.array([10.0, 1.0, 0.5]), "2 and 3 are both loaded: skipped, the walk goes on to the next nearest"),
        (np.array([-200.0, 0.0, 0.0]), "nothing in range"),
        (np.array([27.5, 0.3, 1.6]), "the far end of the line"),
        (np.array([0.4, 0.1, 0.1]), "the near end"),
    ]
    return kfs, steps
