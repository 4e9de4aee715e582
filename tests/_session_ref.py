"""Plain numpy / Python checker of the saved-session unit (include/vxba.h: vxba_session_*, vxba_globalmap), written loop by loop against the
reference's text: the two merge loops of previous_map_read (voxelslam.cpp:331-372, 376-400), its window schedule (:377) and pub_globalmap (:108-150).

The merge expressions are tests/_keyframe_ref.py's ``delta_pose`` / ``transform`` (pinned to the reference by tests/golden/keyframe/); every point is
rounded to float32 where the reference stores it in a PointXYZI / PointType.  The voxel filter is a loop restatement of down_sampling_voxel
(tools.hpp:201-238) -- a map from the float-typed voxel index to a float running mean, visited in input order -- with the output sorted by voxel index,
the order vxba_down_sampling_voxel gives.
"""
import numpy as np

from tests import _keyframe_ref as K

KEY_OFF = 1 << 20


def voxel_index_f32(xyz, vs):
    """tools.hpp:211-214 on float32 points: (index (n, 3) int64, ok (n,)): ok is False where a coordinate is not finite or outside [-2^20, 2^20)."""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        loc = (p.astype(np.float64) / np.float64(vs)).astype(np.float32)
        loc = np.where(loc < 0, (loc.astype(np.float64) - 1.0).astype(np.float32), loc)
        inside = (loc > np.float32(-KEY_OFF - 1)) & (loc < np.float32(KEY_OFF))
        idx = np.trunc(np.where(inside, loc, np.float32(0))).astype(np.int64)
    ok = inside & (idx >= -KEY_OFF) & (idx < KEY_OFF)
    return idx, ok.all(axis=1)


def voxel_keys_f32(xyz, vs):
    idx, ok = voxel_index_f32(xyz, vs)
    u = (idx + KEY_OFF).astype(np.uint64)
    key = (u[:, 0] << np.uint64(42)) | (u[:, 1] << np.uint64(21)) | u[:, 2]
    return np.where(ok, key, np.uint64(0)), ok


def down_sampling_voxel(xyz, vs):
    """down_sampling_voxel as the literal loop; rows ascend by (x, y, z) voxel index.  ValueError for a point the GPU filter refuses."""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    if vs < 0.001:
        return p.copy()
    idx, ok = voxel_index_f32(p, vs)
    if not ok.all():
        raise ValueError("a point is not finite or lies 2^20 voxels or more from the origin")
    feat = {}
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        for k in range(p.shape[0]):
            pos = (int(idx[k, 0]), int(idx[k, 1]), int(idx[k, 2]))
            if pos not in feat:
                feat[pos] = [p[k].copy(), one]
            else:
                pp = feat[pos]
                pp[0] = (pp[0] * pp[1] + p[k]) / (pp[1] + one)      # float32 throughout: numpy keeps float32 op float32 in float32
                pp[1] = pp[1] + one
    return np.array([feat[k][0] for k in sorted(feat)], dtype=np.float32).reshape(-1, 3)


def move(xc, xj, pts):
    """One inner loop of either merge (:350-358, :385-393): float32 points of frame xj in frame xc, float32."""
    dR, dp = K.delta_pose(xc, xj)
    with np.errstate(all="ignore"):
        return K.transform(dR, dp, np.asarray(pts, dtype=np.float32).reshape(-1, 3).astype(np.float64)).astype(np.float32)


def merge_scans(scans, poses, win_size):
    """The merged clouds before the filter: (list of K (n, 3) float32, ids (K,), x0 (K, 12))."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    merged, ids, x0 = [], [], []
    plbuf, xxbuf = [], []
    for i in range(poses.shape[0]):
        xc = poses[i]
        xxbuf.append(xc); plbuf.append(scans[i])
        if len(xxbuf) < win_size:
            continue
        parts = [move(xc, xxbuf[j], plbuf[j]) for j in range(win_size)]
        merged.append(np.concatenate(parts) if parts else np.zeros((0, 3), np.float32))
        ids.append(i); x0.append(xc.copy())
        plbuf, xxbuf = [], []
    return merged, np.array(ids, dtype=np.int64), np.array(x0, dtype=np.float64).reshape(-1, 12)


def build_keyframes(scans, poses, win_size, voxel_size):
    """(clouds: list of K (n_k, 3) float32, ids, x0)."""
    merged, ids, x0 = merge_scans(scans, poses, win_size)
    return [down_sampling_voxel(m, voxel_size / 10) for m in merged], ids, x0


def windows(K_, acsize, mgsize):
    """:377: the first keyframe of every descriptor window."""
    out = []
    i = 0
    while i + acsize < K_:
        out.append(i)
        i += mgsize
    return out


def window_cloud(clouds, x0, ids, i, acsize):
    """:379-395: (cloud (n, 3) float32 in the frame of keyframe i + acsize - 1, that keyframe's id)."""
    up = i + acsize
    xc = x0[up - 1]
    parts = [move(xc, x0[j], clouds[j]) for j in range(i, up)]
    return np.concatenate(parts), int(ids[up - 1])


def globalmap(sets, interval_size):
    """pub_globalmap over ``sets`` = [(clouds, x0, id), ...]: dict(xyzi (n, 4) float32, chunk_ptr, jump, counts per keyframe).  psize in Python
    integers (the 64-bit deviation)."""
    psize = sum(int(np.asarray(c).reshape(-1, 3).shape[0]) for clouds, _, _ in sets for c in clouds)
    jump = psize // (10 * int(interval_size)) + 1
    rows, chunks, counts = [], [0], []
    total = pending = 0
    for clouds, x0, sid in sets:
        for i, c in enumerate(clouds):
            c = np.asarray(c, dtype=np.float32).reshape(-1, 3)
            xx = np.asarray(x0[i], dtype=np.float64)
            R_cm, p = xx[:9], xx[9:12]
            cnt = 0
            for j in range(0, c.shape[0], jump):
                vv = K.transform(R_cm, p, c[j].astype(np.float64)[None])[0]      # vv = xx.R * vv + xx.p
                rows.append([np.float32(vv[0]), np.float32(vv[1]), np.float32(vv[2]), np.float32(sid)])
                cnt += 1
            counts.append(cnt)
            total += cnt; pending += cnt
            if pending > interval_size:
                chunks.append(total); pending = 0
    chunks.append(total)
    return dict(xyzi=np.array(rows, dtype=np.float32).reshape(-1, 4), chunk_ptr=np.array(chunks, dtype=np.int64), jump=jump, counts=np.array(counts, dtype=np.int64))


def descriptor_frames(scans, poses, win_size, voxel_size, acsize, mgsize):
    """The whole chain up to the clouds the corner extraction takes: (window clouds with their frame ids, keyframe clouds, ids, x0)."""
    clouds, ids, x0 = build_keyframes(scans, poses, win_size, voxel_size)
    return [window_cloud(clouds, x0, ids, i, acsize) for i in windows(len(clouds), acsize, mgsize)], clouds, ids, x0
