"""The loop hand-back: the optimised pose graph back into the local map (the host bookkeeping of loop_update, voxelslam.cpp:1116-1159, and of the
tail of thd_loop_closure's optimisation branch, :2100-2129, around ``vxba.KeyframeArchive`` and ``LocalMap.loop_update_device``).

Every cloud stays on the device: keyframes enter the archive device to device, the world points of ``map_loop`` and of the buffered scans come out of
one launch, and ``loop_update_device`` reads them where they lie.  The 3 x 3 algebra here is written out -- every inner product
``(a0 b0 + a1 b1) + a2 b2``, no ``@`` -- so that tests/_handback_ref.py reproduces it for equality.
"""
from __future__ import annotations

import numpy as np

from . import vxba


def _mv(A, b):
    """A b for a 3 x 3 and a 3-vector, each row's product summed as written."""
    return (A[:, 0] * b[0] + A[:, 1] * b[1]) + A[:, 2] * b[2]


def _mm(A, B):
    return np.stack([_mv(A, B[:, j]) for j in range(3)], axis=1)


def _R(rec):
    """The rotation of a pose or state record [R column-major 9 | p 3 | ...]."""
    return np.asarray(rec[:9], dtype=np.float64).reshape(3, 3).T


def loop_delta(x1, x3):
    """dx of :2126-2128 from the newest scan pose before (x1) and after (x3) the optimisation: dx.R = x3.R x1.R^T, dx.p = x3.p - (x3.R x1.R^T) x1.p.
    Returns (R (3, 3), p (3,))."""
    x1 = np.asarray(x1, dtype=np.float64); x3 = np.asarray(x3, dtype=np.float64)
    dR = _mm(_R(x3), _R(x1).T)
    return dR, x3[9:12] - _mv(dR, x1[9:12])


def turn_pose(dx, rec):
    """ScanPose::update / the x_buf loop of loop_update on one record: p = dx.R p + dx.p, R = dx.R R, and v = dx.R v where the record has one."""
    dR, dp = dx
    out = np.array(rec, dtype=np.float64)
    out[:9] = _mm(dR, _R(rec)).T.reshape(9)
    out[9:12] = _mv(dR, out[9:12]) + dp
    if out.shape[0] >= 15:
        out[12:15] = _mv(dR, out[12:15])
    return out


class LoopHandback:
    """The running session's keyframe archive and the state the hand-back carries between the loop thread and local mapping: ``dx``, ``loop_detect``,
    the optimised scan poses of the path.  ``init_num`` and ``radius`` are the reference's 5 and 10; ``cumulative`` True is upstream's map_loop as written."""

    def __init__(self, init_num: int = 5, radius: float = 10.0, cumulative: bool = True, device: int = 0):
        self.archive = vxba.KeyframeArchive(device=device)
        self.init_num, self.radius, self.cumulative = int(init_num), float(radius), bool(cumulative)
        self.dx = (np.eye(3), np.zeros(3))
        self.loop_detect = 0
        self.scan_poses = np.zeros((0, 12))

    def close(self):
        self.archive.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def clear(self):
        """system_reset."""
        self.archive.clear()
        self.dx = (np.eye(3), np.zeros(3)); self.loop_detect = 0; self.scan_poses = np.zeros((0, 12))

    def on_keyframe(self, builder: "vxba.KeyframeBuilder"):
        """The builder's last keyframe into the archive, device to device (what ``hba.keyframe_stream(archive=...)`` calls)."""
        self.archive.add_from(builder)

    def on_optimised(self, scan_poses, before):
        """:2100-2167 after the pose graph has run.  ``scan_poses`` (n_scans, 12): every ScanPose after ``set_state``; ``before``: the same before it
        (or just the newest one, (12,)).  Keyframes take ``x0 = scan_poses[id]``, ``dx`` comes from the newest scan pose before and after, the history
        is armed and ``loop_detect`` raised.  Returns dx."""
        sp = np.ascontiguousarray(scan_poses, dtype=np.float64).reshape(-1, 12)
        b = np.asarray(before, dtype=np.float64)
        x1 = b.reshape(-1, 12)[-1]
        ids = self.archive.ids()
        if ids.size and (ids.min() < 0 or ids.max() >= sp.shape[0]):
            raise ValueError("on_optimised: a keyframe's id has no scan pose")
        if ids.size:
            self.archive.set_poses(sp[ids])
        self.dx = loop_delta(x1, sp[-1])
        self.scan_poses = sp
        self.archive.arm_history(self.init_num)
        self.loop_detect = 1
        return self.dx

    def keyframe_loading(self, p_curr, jour: float, local_map: "vxba.LocalMap") -> int:
        """keyframe_loading(jour) (:1189-1228): at most one history keyframe near ``p_curr`` enters ``local_map`` as fixed points with zero variances.
        Returns its index, or -1."""
        r = self.archive.load_near(p_curr, self.radius)
        if r["k"] >= 0:
            local_map.cut_voxel_fix_device(r["n"], r["pnt_world"], None, float(jour))
        return r["k"]

    def loop_update(self, local_map: "vxba.LocalMap", states, x_curr, g_update: int, est=None, pending=()):
        """loop_update (:1101-1186).  ``states`` (win_count, >= 15) window states [R | p | v | bg | ba | g], ``x_curr`` one such record,
        ``pending`` the buffered scans (``buf_lba2loop``) as (pose or state record, n, d_pnt_body, d_var) with raw device addresses.  Every window
        state, ``x_curr.v`` and the pending poses are turned by dx (gravity too while ``g_update == 1``); the map is rebuilt from the archive's last
        ``init_num`` keyframes, then the pending scans, then the window's resident scans, in ONE ``loop_update_device``.
        Returns dict(states, x_curr, g_update, path (float32 positions: scan poses, pending, window), pending_poses)."""
        dR, dp = self.dx
        st = np.array(states, dtype=np.float64).reshape(len(states), -1)
        xc = np.array(x_curr, dtype=np.float64)
        path = [self.scan_poses[:, 9:12]]
        pend = [turn_pose(self.dx, s[0]) for s in pending]
        path.append(np.array([q[9:12] for q in pend]).reshape(-1, 3))
        for i in range(st.shape[0]):
            g = _mv(dR, st[i, 21:24]) if g_update == 1 and st.shape[1] >= 24 else None
            st[i] = turn_pose(self.dx, st[i])
            if g is not None:
                st[i, 21:24] = g
        path.append(st[:, 9:12])
        if st.shape[0]:
            xc[:12] = st[-1, :12]
            xc[12:15] = _mv(dR, xc[12:15])
            if xc.shape[0] >= 24 and st.shape[1] >= 24:
                xc[21:24] = st[-1, 21:24]
        ml = self.archive.map_loop(self.init_num, self.cumulative, [(q[:12], s[1], s[2], s[3]) for q, s in zip(pend, pending)])
        local_map.loop_update_device(ml["cloud_ptr"], ml["pnt_world"], ml["var"], st[:, :12], est=est, jour=0.0)
        self.loop_detect = 0
        return dict(states=st, x_curr=xc, g_update=2 if g_update == 1 else g_update, path=np.concatenate(path).astype(np.float32), pending_poses=pend)
