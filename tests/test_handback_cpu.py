"""CPU suite of the loop hand-back: the numpy checker (tests/_handback_ref.py) against clouds computed by hand, a vectorised restatement and the host
build of csrc/vxba_handback_math.hpp; dx against mathematics; the honesty of the loading scenarios' inputs; and four degraded checkers that the
equality criteria of tests/test_gpu_handback.py must reject -- on the very inputs that file uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _handback_ref as H

HERE = os.path.dirname(os.path.abspath(__file__))
INIT = 5
RADIUS = 10.0


# ---- the checker against clouds computed by hand ----
def test_two_keyframes_of_two_points_by_hand():
    """A quarter turn about z and a translation: every product is exact, so the expected numbers are written down, not computed."""
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    a = H.Archive()
    a.add(2, H.pose_rec(Rz, [1.0, 2.0, 3.0]), 0.0, [[1.0, 0.0, 0.0, 0.5, 0.25, 0.125], [0.0, 2.0, -1.0, 1.0, 2.0, 4.0]])
    a.add(5, H.pose_rec(np.eye(3), [-10.0, 0.0, 0.5]), 0.1, [[-1.5, 2.0, 0.25, 0.0, 0.5, 0.0], [3.0, -4.0, 8.0, 0.75, 0.0, 1.5]])
    kf0 = [[1.0, 3.0, 3.0], [-1.0, 2.0, 2.0]]
    kf1 = [[-11.5, 2.0, 0.75], [-7.0, -4.0, 8.5]]
    d0 = [[0.5, 0.25, 0.125], [1.0, 2.0, 4.0]]; d1 = [[0.0, 0.5, 0.0], [0.75, 0.0, 1.5]]
    cptr, P, V = a.map_loop(INIT, cumulative=True)                       # pvec_tem is never cleared: the second cloud starts with the first keyframe again
    assert cptr.tolist() == [0, 2, 6] and P.tolist() == kf0 + kf0 + kf1
    assert [np.diag(v).tolist() for v in V] == d0 + d0 + d1 and all((v - np.diag(np.diag(v)) == 0).all() for v in V)
    cptr, P, V = a.map_loop(INIT, cumulative=False)
    assert cptr.tolist() == [0, 2, 4] and P.tolist() == kf0 + kf1 and [np.diag(v).tolist() for v in V] == d0 + d1
    cptr, P, V = a.map_loop(1, cumulative=True)                          # only the last keyframe
    assert cptr.tolist() == [0, 2] and P.tolist() == kf1
    cptr, P, V = a.map_loop(INIT, True, pending=[(H.pose_rec(Rz, [0.0, 0.0, 1.0]), [[2.0, 1.0, 0.0]], [np.arange(9.0).reshape(3, 3)])])
    assert cptr.tolist() == [0, 2, 6, 7] and P[6].tolist() == [-1.0, 2.0, 1.0] and V[6].tolist() == np.arange(9.0).reshape(3, 3).tolist()    # the full var, unrotated


@pytest.mark.parametrize("seed", range(3))
def test_loop_and_vectorised_restatement_agree(seed):
    for kid, pose, _, down in H.make_keyframes(9, seed):
        assert H.world_cloud(pose, down[:, :3]).tobytes() == H.world_cloud_vec(pose, down[:, :3]).tobytes()


# ---- the host build of the device header against the checker's bits ----
@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "handback_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libhandback_hostcheck.so")
    hdrs = [os.path.join(HERE, "..", "voxel-slam_amd", "csrc", h) for h in ("vxba_handback_math.hpp", "vxba_session_math.hpp", "vxba_keyframe_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"); f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    L.hbh_keyframe.argtypes = [C.c_int, f64p, f32p, f64p, f64p]
    L.hbh_scan.argtypes = [C.c_int, f64p, f64p, f64p]
    L.hbh_dist2.argtypes = [C.c_int, f32p, f32p, f32p]
    L.hbh_nearest.argtypes = [f32p, C.c_longlong, np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS"), f32p, C.c_float]
    L.hbh_nearest.restype = C.c_longlong
    L.hbh_owner.argtypes = [np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS"), C.c_longlong, C.c_longlong]
    L.hbh_owner.restype = C.c_longlong
    return L


def test_hostcheck_world_points_and_variances(hm):
    rng = np.random.default_rng(4)
    for kid, pose, _, down in H.make_keyframes(9, 1):
        n = down.shape[0]
        pnt = np.zeros((max(n, 1), 3)); var = np.zeros((max(n, 1), 9))
        hm.hbh_keyframe(n, pose, np.ascontiguousarray(down) if n else np.zeros((1, 6), dtype=np.float32), pnt, var)
        a = H.fill(H.Archive(), [(kid, pose, 0.0, down)])
        _, P, V = a.map_loop(1)
        assert pnt[:n].tobytes() == P.tobytes() and var[:n].tobytes() == V.reshape(n, 9).tobytes()
        body = rng.normal(size=(17, 3)) * 30
        out = np.zeros((17, 3))
        hm.hbh_scan(17, pose, body, out)
        assert out.tobytes() == H.world_cloud(pose, body).tobytes()


def test_hostcheck_distances_walk_and_owner(hm):
    kfs, steps = H.make_history()
    a = H.fill(H.Archive(), kfs); a.arm_history(INIT)
    for p, _ in steps:
        pc = np.asarray(p, dtype=np.float32)
        d = np.zeros(len(a.snap), dtype=np.float32)
        hm.hbh_dist2(len(a.snap), a.snap, pc, d)
        assert d.tobytes() == a.distances(p).tobytes()
        ex = np.ascontiguousarray(a.exist()[:len(a.snap)].astype(np.uint8))
        k_host = hm.hbh_nearest(a.snap, len(a.snap), ex, pc, np.float32(RADIUS * RADIUS))
        assert k_host == a.load_near(p, RADIUS)[0]
    ptr = np.array([0, 0, 3, 3, 3, 10, 11], dtype=np.int64)           # empty owners are skipped
    assert [hm.hbh_owner(ptr, 6, g) for g in range(11)] == [1, 1, 1, 4, 4, 4, 4, 4, 4, 4, 5]


def test_map_loop_cases_hold_what_they_claim():
    """Every keyframe size at which the kernel's workgroup of 256 rows can go wrong, an empty keyframe inside the range, coordinates of both signs,
    poses tens of metres out."""
    seen, empty_inside = set(), False
    for K, seed in H.MAP_LOOP_SEED.items():
        kfs = H.make_keyframes(K, seed=seed)
        sizes = [k[3].shape[0] for k in kfs[-INIT:]]
        seen |= set(sizes)
        empty_inside |= 0 in sizes[1:-1]
        if K >= 4:
            assert min(k[3][:, :3].min() for k in kfs if k[3].size) < -1 and max(np.abs(k[1][9:]).max() for k in kfs) > 20
    assert {0, 1, 63, 64, 65, 255, 256, 257} <= seen and empty_inside and sorted(H.MAP_LOOP_SEED) == [0, 1, 4, 5, 6, 9]


# ---- the loading scenarios: what they exercise, and the honesty of their inputs ----
def test_loading_scenario_walk_and_honest_inputs():
    kfs, steps = H.make_history()
    a = H.fill(H.Archive(), kfs)
    assert a.load_near(steps[0][0], RADIUS)[0] == -1                   # not armed: history_kfsize <= 0
    a.arm_history(INIT)
    assert a.history_kfsize == 8 and a.exist().tolist() == [1] * 8 + [0] * 5
    r2 = np.float32(RADIUS * RADIUS)
    ties = 0
    for p, _ in steps:
        d2 = a.distances(p).astype(np.float64)
        assert (np.abs(d2 - float(r2)) >= 1e-3).all(), "a test distance sits on the boundary d2 == r2, which is not pinned"
        inside = np.sort(d2[d2 < float(r2)])
        gaps = np.diff(inside)
        ties += int((gaps == 0).sum())
        assert ((gaps == 0) | (gaps > 1e-3)).all(), "two distinct candidates closer than 1e-3 in d2"
        a.load_near(p, RADIUS)
    assert ties >= 1                                                   # the deliberate one (keyframes 2 and 3 mirrored about the query), seen while both are candidates
    b = H.fill(H.Archive(), kfs); b.arm_history(INIT)
    got = [b.load_near(p, RADIUS)[0] for p, _ in steps]
    assert got == [2, 3, 1, -1, 7, 0] and b.history_kfsize == 3 and b.exist().tolist() == [0, 0, 0, 0, 1, 1, 1, 0] + [0] * 5
    few = H.fill(H.Archive(), kfs[:INIT]); few.arm_history(INIT)       # K <= init_num: nothing is armed
    assert few.history_kfsize == 0 and few.load_near(steps[0][0], RADIUS)[0] == -1 and not few.exist().any()


def test_snapshot_is_what_the_search_reads_and_x0_what_the_transform_reads():
    kfs, steps = H.make_history()
    a = H.fill(H.Archive(), kfs); a.arm_history(INIT)
    moved = np.array([k[1] for k in kfs]); moved[:, 9:] += 1000.0       # set_poses after arming
    a.set_poses(moved)
    k, pts = a.load_near(steps[0][0], RADIUS)
    assert k == 2 and pts.tobytes() == H.world_cloud(moved[2], kfs[2][3][:, :3]).tobytes()


# ---- dx against mathematics ----
def _states(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        s = np.zeros(24)
        s[:12] = H.pose_rec(H.rodrigues(rng.normal(size=3) * 0.5), rng.normal(size=3) * 20)
        s[12:24] = rng.normal(size=12)
        out.append(s)
    return np.array(out)


def _compose(dx, rec):
    R = np.array(dx[0]) @ rec[:9].reshape(3, 3).T
    return R, np.array(dx[0]) @ rec[9:12] + np.array(dx[1])


def test_dx_composes_preserves_relative_poses_and_follows_the_g_update_rule():
    from voxel_slam_amd import handback as HB
    st = _states(6, 3)
    x1 = st[-1, :12]
    x3 = H.pose_rec(H.rodrigues([0.02, -0.01, 0.3]) @ x1[:9].reshape(3, 3).T, x1[9:12] + np.array([0.5, -0.3, 0.1]))
    dx = H.loop_delta(x1, x3)
    R, p = _compose(dx, x1)                                            # dx o x1 == x3 to rounding
    assert np.abs(R - x3[:9].reshape(3, 3).T).max() < 1e-14 and np.abs(p - x3[9:]).max() < 1e-13
    ident = H.loop_delta(x1, x1)                                       # an identity optimisation gives the identity
    assert np.abs(np.array(ident[0]) - np.eye(3)).max() < 1e-15 and np.abs(ident[1]).max() < 1e-13
    got = H.loop_update(dx, st[:4, :12], st, st[-1], 1, pending_poses=[st[1, :12], st[2, :12]])
    new = got["states"]
    for i in range(1, len(st)):                                        # relative poses survive
        rel0 = st[i - 1, :9].reshape(3, 3) @ st[i, :9].reshape(3, 3).T          # R_{i-1}^T R_i with the records column-major
        rel1 = new[i - 1, :9].reshape(3, 3) @ new[i, :9].reshape(3, 3).T
        t0 = st[i - 1, :9].reshape(3, 3) @ (st[i, 9:12] - st[i - 1, 9:12]); t1 = new[i - 1, :9].reshape(3, 3) @ (new[i, 9:12] - new[i - 1, 9:12])
        assert np.abs(rel0 - rel1).max() < 1e-13 and np.abs(t0 - t1).max() < 1e-12
    assert got["g_update"] == 2 and np.abs(new[:, 21:24] - st[:, 21:24] @ np.array(dx[0]).T).max() < 1e-14
    assert (new[:, 15:21] == st[:, 15:21]).all()                       # the biases are not touched
    assert (got["x_curr"][:12] == new[-1, :12]).all() and (got["x_curr"][21:24] == new[-1, 21:24]).all()
    assert got["path"].shape == (4 + 2 + 6, 3) and got["path"].dtype == np.float32
    again = H.loop_update(dx, st[:4, :12], st, st[-1], 2)              # g_update != 1: gravity stays, the flag stays
    assert again["g_update"] == 2 and (again["states"][:, 21:24] == st[:, 21:24]).all()
    assert H.loop_update(dx, st[:4, :12], st, st[-1], 0)["g_update"] == 0
    # the product's host algebra is the checker's, bit for bit
    pdx = HB.loop_delta(x1, x3)
    assert np.array(pdx[0]).tobytes() == np.array(dx[0]).tobytes() and np.array(pdx[1]).tobytes() == np.array(dx[1]).tobytes()
    for s in st:
        assert HB.turn_pose(pdx, s).tobytes() == H.turn(dx, s).tobytes() and HB.turn_pose(pdx, s[:12]).tobytes() == H.turn(dx, s[:12]).tobytes()


# ---- degraded checkers: each must differ from the checker on the GPU suite's own inputs, so an implementation that made the mistake fails there ----
@pytest.mark.parametrize("K", [1, 4, 5, 6, 9])
def test_rotated_variances_are_rejected(K):
    kfs = H.make_keyframes(K, seed=H.MAP_LOOP_SEED[K])
    good = H.fill(H.Archive(), kfs).map_loop(INIT, True)
    bad = H.fill(H.Archive("rotated_var"), kfs).map_loop(INIT, True)
    assert good[1].tobytes() == bad[1].tobytes() and good[2].tobytes() != bad[2].tobytes()


@pytest.mark.parametrize("K", [4, 5, 6, 9])
def test_non_cumulative_where_cumulative_is_asked_is_rejected(K):
    kfs = H.make_keyframes(K, seed=H.MAP_LOOP_SEED[K])
    good = H.fill(H.Archive(), kfs).map_loop(INIT, True)
    bad = H.fill(H.Archive("not_cumulative"), kfs).map_loop(INIT, True)
    assert good[0].tolist() != bad[0].tolist() and good[1].shape != bad[1].shape


@pytest.mark.parametrize("degrade", ["stop_at_first", "f64_distances"])
def test_degraded_walks_are_rejected(degrade):
    kfs, steps = H.make_history()
    good = H.fill(H.Archive(), kfs); good.arm_history(INIT)
    bad = H.fill(H.Archive(degrade), kfs); bad.arm_history(INIT)
    assert [good.load_near(p, RADIUS)[0] for p, _ in steps] != [bad.load_near(p, RADIUS)[0] for p, _ in steps]
