"""Plain numpy / Python checker of the keyframe builder (include/vxba.h: vxba_keyframe_*), written against the reference's text: the front half of
thd_loop_closure (voxelslam.cpp:1898-1977) and down_sampling_pvec (voxel_map.hpp:24-65).

Everything is float64 written out term by term -- every 3-term inner product (a0 b0 + a1 b1) + a2 b2, the translation added last, the running mean
(m c + v) / (c + 1) with a true division -- the association tests/golden/keyframe/keyframe.npz pins; upstream's float-typed voxel index is emulated with
np.float32.  The filter is sequential per voxel (points in input order); ``down_sampling_pvec`` runs the voxels side by side, one numpy step per
rank of a point inside its voxel, ``down_sampling_pvec_map`` is the literal hash-map loop the former is checked against.

A pose record is [R column-major 9 | t 3]; a covariance is 9 values column-major (or 3 x 3: it is symmetric where it matters -- only the diagonal is read).
"""
import math

import numpy as np

KEY_OFF = 1 << 20
KEY_BITS = 21


def mat_tmul(A, B):
    """A^T B of two column-major 3 x 3 (9 values each), column-major."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    out = np.zeros(9)
    for j in range(3):
        for i in range(3):
            out[3 * j + i] = (A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1]) + A[3 * i + 2] * B[3 * j + 2]
    return out


def delta_pose(xc, bl):
    """delta_R = xc.R^T bl.R (column-major 9), delta_p = xc.R^T (bl.p - xc.p)   (:1948-1949)"""
    xc = np.asarray(xc, dtype=np.float64); bl = np.asarray(bl, dtype=np.float64)
    dR = mat_tmul(xc[:9], bl[:9])
    d = bl[9:] - xc[9:]
    dp = np.array([(xc[3 * i] * d[0] + xc[3 * i + 1] * d[1]) + xc[3 * i + 2] * d[2] for i in range(3)])
    return dR, dp


def transform(dR, dp, pnt):
    """q = delta_R pnt + delta_p per row of pnt (n, 3)   (:1952)"""
    p = np.asarray(pnt, dtype=np.float64).reshape(-1, 3)
    q = np.empty_like(p)
    for i in range(3):
        q[:, i] = ((dR[i] * p[:, 0] + dR[3 + i] * p[:, 1]) + dR[6 + i] * p[:, 2]) + dp[i]
    return q


def voxel_index(q, vs):
    """Upstream's voxel index per coordinate (voxel_map.hpp:32-37) and the mask of coordinates that are finite with an index inside (-2^20, 2^20)."""
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(all="ignore"):
        l0 = (q / np.float64(vs)).astype(np.float32)
        ok = (l0 > np.float32(-KEY_OFF)) & (l0 < np.float32(KEY_OFF))
        l = np.where(l0 < 0, (l0.astype(np.float64) - 1.0).astype(np.float32), l0)
        idx = np.trunc(np.where(ok, l, np.float32(0))).astype(np.int64)
    ok &= (idx > -KEY_OFF) & (idx < KEY_OFF)
    return np.where(ok, idx, 0), ok


def voxel_keys(q, vs):
    """63-bit key per point (x most significant) and the per-point validity."""
    idx, ok = voxel_index(np.asarray(q, dtype=np.float64).reshape(-1, 3), vs)
    good = ok.all(axis=1)
    u = (idx + KEY_OFF).astype(np.uint64)
    key = (u[:, 0] << np.uint64(2 * KEY_BITS)) | (u[:, 1] << np.uint64(KEY_BITS)) | u[:, 2]
    return np.where(good, key, np.uint64(0)), good


def mean_step(m, c, v):
    return (m * float(c) + v) / float(c + 1)


def down_sampling_pvec(q, var3, vs):
    """(down (n_down, 6) float32 ascending by voxel index, keys (n_down,), points per voxel)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    rows = np.concatenate([q, np.asarray(var3, dtype=np.float64).reshape(-1, 3)], axis=1)
    n = rows.shape[0]
    if n == 0:
        return np.zeros((0, 6), np.float32), np.zeros(0, np.uint64), np.zeros(0, np.int64)
    key, good = voxel_keys(q, vs)
    if not good.all():
        raise ValueError("a merged point is not finite or lies 2^20 voxels or more from the origin")
    order = np.argsort(key, kind="stable")
    ks = key[order]; rows = rows[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    counts = np.diff(np.concatenate([starts, [n]]))
    m = rows[starts].copy()
    with np.errstate(all="ignore"):
        for r in range(1, int(counts.max())):
            live = np.flatnonzero(counts > r)
            m[live] = mean_step(m[live], r, rows[starts[live] + r])
        return m.astype(np.float32), ks[starts], counts


def down_sampling_pvec_map(q, var3, vs):
    """The same as the literal loop over a map from voxel index to (running mean, count); output sorted by voxel index."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3); var3 = np.asarray(var3, dtype=np.float64).reshape(-1, 3)
    idx, ok = voxel_index(q, vs)
    if not ok.all():
        raise ValueError("a merged point is not finite or lies 2^20 voxels or more from the origin")
    feat = {}
    for k in range(q.shape[0]):
        pos = (int(idx[k, 0]), int(idx[k, 1]), int(idx[k, 2]))
        row = np.concatenate([q[k], var3[k]])
        if pos not in feat:
            feat[pos] = [row, 1]
        else:
            pp = feat[pos]
            pp[0] = (pp[0] * float(pp[1]) + row) / float(pp[1] + 1)
            pp[1] += 1
    keys = sorted(feat)
    return (np.array([feat[k][0] for k in keys], dtype=np.float64).reshape(-1, 6).astype(np.float32), np.array(keys, dtype=np.int64).reshape(-1, 3),
            np.array([feat[k][1] for k in keys], dtype=np.int64))


def rule_metrics(x_key, xc):
    """(ang, len) of :1932-1933 with Log of tools.hpp:86-91."""
    x_key = np.asarray(x_key, dtype=np.float64); xc = np.asarray(xc, dtype=np.float64)
    M = [float(v) for v in mat_tmul(x_key[:9], xc[:9])]
    tr = (M[0] + M[4]) + M[8]
    theta = 0.0 if tr > 3.0 - 1e-6 else math.acos(0.5 * (tr - 1))
    K = (M[5] - M[7], M[6] - M[2], M[1] - M[3])
    s = 0.5 if abs(theta) < 0.001 else 0.5 * theta / math.sin(theta)
    w = [s * k for k in K]
    ang = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) * 57.3
    d = [float(xc[9 + k]) - float(x_key[9 + k]) for k in range(3)]
    return ang, math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def var_diagonal(var, n):
    if var is None:
        return np.zeros((n, 3))
    v = np.asarray(var, dtype=np.float64).reshape(n, 9)
    return np.ascontiguousarray(v[:, [0, 4, 8]])


def assemble(poses, scans, variances=None):
    """The merged cloud of buffered scans (oldest first) in the frame of the LAST pose: (q (N, 3) float64, var diagonal (N, 3), full (N, 3) float32).
    The variances are carried over unrotated, as upstream does."""
    xc = poses[-1]
    qs, vs_ = [], []
    for k, (P, S) in enumerate(zip(poses, scans)):
        S = np.asarray(S, dtype=np.float64).reshape(-1, 3)
        dR, dp = delta_pose(xc, P)
        qs.append(transform(dR, dp, S))
        vs_.append(var_diagonal(None if variances is None else variances[k], S.shape[0]))
    q = np.concatenate(qs) if qs else np.zeros((0, 3)); v = np.concatenate(vs_) if vs_ else np.zeros((0, 3))
    with np.errstate(all="ignore"):
        return q, v, q.astype(np.float32)


class KeyframeRef:
    """The rule of :1928-1942 over a ScanPose buffer; ``push_scan`` returns True when a keyframe was emitted (``self.keyframe``).  ``self.action`` of
    the last push: "buffer", "drop" or "emit".  Bad input raises ValueError and leaves everything as it was."""

    def __init__(self, win_size=10, voxel_size=1.0, ang_deg=5.0, len_thr=0.1):
        self.win, self.voxel_size, self.ang_deg, self.len_thr = int(win_size), float(voxel_size), float(ang_deg), float(len_thr)
        self.clear()

    def clear(self):
        self.poses, self.v6s, self.ring = [], [], []
        self.buf_base, self.jour, self.x_key, self.keyframe, self.action = 0, 0.0, None, None, None

    def num_scans(self):
        return len(self.poses)

    def push_scan(self, pose, v6, pnt_body, var=None):
        pose = np.array(pose, dtype=np.float64).reshape(12); v6 = np.array(v6, dtype=np.float64).reshape(6)
        pts = np.array(pnt_body, dtype=np.float64).reshape(-1, 3)
        if not np.isfinite(pts).all() or not np.isfinite(pose).all():
            raise ValueError("a point is not finite")
        ring = self.ring + [(len(self.poses), pts, var_diagonal(var, pts.shape[0]))]
        x_key = pose if self.buf_base == 0 else self.x_key
        buf_base = self.buf_base + 1
        action, keyframe, jour = "buffer", self.keyframe, self.jour
        if len(ring) >= self.win:
            ang, ln = rule_metrics(x_key, pose)
            if ang < self.ang_deg and ln < self.len_thr and buf_base > self.win:
                action = "drop"
                ring = ring[1:]
            else:
                action = "emit"
                all_poses = self.poses + [pose]
                q, v, full = assemble([all_poses[i] for i, _, _ in ring], [p for _, p, _ in ring])
                v = np.concatenate([d for _, _, d in ring])
                down, keys, counts = down_sampling_pvec(q, v, self.voxel_size / 10)      # raises before anything is changed
                jour = jour + ln
                x_key = pose
                keyframe = dict(id=buf_base - 1, pose=pose.copy(), jour=jour, full=full, down=down, keys=keys, counts=counts, q=q, var=v)
                ring = []
        self.poses.append(pose); self.v6s.append(v6)
        self.ring, self.x_key, self.buf_base, self.jour, self.keyframe, self.action = ring, x_key, buf_base, jour, keyframe, action
        return action == "emit"

    def scan_poses(self):
        return np.array(self.poses).reshape(-1, 12), np.array(self.v6s).reshape(-1, 6)
