"""Initialisation (scan-to-cloud odometry), CPU side: the checker (tests/_init_ref.py) against mathematics, the host build of
csrc/vxba_init_math.hpp against the checker, and the honesty of every session tests/test_gpu_init.py uses -- no decision of theirs may hang on
the rounding by which the checker (lstsq, inv) and the product (pivoted QR, Gauss-Jordan) differ."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _init_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "init_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libinit_hostcheck.so")
    hdr = os.path.join(HERE, "..", "voxel-slam_amd", "csrc", "vxba_init_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.inh_fit.argtypes = [C.c_int, f64p, f64p, u8p, f64p, f64p]
    L.inh_rows.argtypes = [C.c_int, f64p, f64p, f64p, f64p, f64p, f64p]
    L.inh_knn.argtypes = [C.c_int, f32p, C.c_int, f32p, i32p, f32p]
    L.inh_deskew.argtypes = [C.c_int, f64p, i32p, f64p, f64p, f32p, f64p, f64p]
    L.inh_midpoint.argtypes = [C.c_int, f64p, f64p, f64p, f64p, C.c_double, f64p, f64p]
    L.inh_pointvar.argtypes = [C.c_int, f64p, C.c_float, C.c_double, f64p, f64p, f64p, f64p, f64p]
    L.inh_align_gravity.argtypes = [f64p, C.c_int]
    return L


def _fit(hm, A):
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 15)
    n = A.shape[0]
    direct = np.zeros((n, 3)); ok = np.zeros(n, dtype=np.uint8); worst = np.zeros(n); plane = np.zeros((n, 4))
    hm.inh_fit(n, A, direct, ok, worst, plane)
    return direct, ok.astype(bool), worst, plane


# ---- the checker against mathematics -------------------------------------------------------------------------------------------------
def test_knn_equals_a_sort_with_planted_ties():
    rng = np.random.default_rng(5)
    c = rng.normal(size=(700, 3)).astype(np.float32)
    c[300] = c[12]; c[650] = c[12]; c[13] = c[500]                          # exact duplicates: equal distances to every query
    q = np.concatenate([c[12:13], c[500:501], rng.normal(size=(40, 3)).astype(np.float32)])
    idx, sqd, nxt = R.knn(c, q, with_next=True)
    for i in range(q.shape[0]):
        d = R.sqdist(c, q[i])
        o = np.lexsort((np.arange(c.shape[0]), d))
        assert np.array_equal(idx[i], o[:5]) and np.array_equal(sqd[i], d[o[:5]]) and nxt[i] == d[o[5]]
    assert list(idx[0][:3]) == [12, 300, 650] and list(idx[1][:2]) == [13, 500]
    few, fd = R.knn(c[:3], q[:2])
    assert (few[:, 3:] == -1).all() and np.isinf(fd[:, 3:]).all() and (few[:, :3] >= 0).all()
    none, _ = R.knn(c[:0], q[:2])
    assert (none == -1).all()


def test_planted_case_moves_towards_the_truth():
    case = R.make_step_case(n_cloud=4000, n_scan=800, seed=3)
    ref = R.InitOdometryRef()
    assert ref.step(case["seed_pts"], R.pack_state(np.eye(3), np.zeros(3)), case["cov"])["seeded"] and ref.cloud_size() == 4000
    r = ref.step(case["scan_body"], case["state_init"], case["cov"])
    assert not r["seeded"] and 1 <= r["iterations"] <= 4 and r["refind"][0]

    def err(s):
        Ra, Rb = s[:9].reshape(3, 3).T, case["state_true"][:9].reshape(3, 3).T
        return np.linalg.norm(s[9:12] - case["state_true"][9:12]), np.linalg.norm(R.so3_log(Ra.T @ Rb))
    (t0, r0), (t1, r1) = err(case["state_init"]), err(r["state"])
    assert t1 < 0.5 * t0 and r1 < 0.5 * r0, (t0, r0, t1, r1)
    assert ref.cloud_size() < 4000 + 800                                      # the filter merged the appended scan into occupied voxels


def test_seeding_appends_without_a_filter_until_100_points():
    ref = R.InitOdometryRef()
    s = R.pack_state(R.so3_exp(np.array([0.1, 0.2, -0.1])), np.array([1.0, -2.0, 0.5]))
    p = np.random.default_rng(1).normal(size=(60, 3)) * 0.01                  # all inside one filter voxel: a filter would leave one point
    a = ref.step(p, s, np.eye(15)); b = ref.step(p, s, np.eye(15))
    assert a["seeded"] and b["seeded"] and ref.cloud_size() == 120 and np.array_equal(a["state"], s)
    assert np.array_equal(ref.cloud()[:60], R.world_points(s, p).astype(np.float32))


# ---- vxba_init_math.hpp on the host --------------------------------------------------------------------------------------------------
def test_host_pivoted_qr_against_lstsq(hm):
    rng = np.random.default_rng(7)
    n = 2000
    c = rng.uniform(-20, 20, (n, 1, 3)) * rng.choice([1.0, 0.05], (n, 1, 1))       # far from the origin and near it: the gate residual is the offset over the range
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    sp = rng.normal(size=(n, 5, 3)) * 0.3
    sp -= (sp @ nrm[:, :, None]) * nrm[:, None, :] * rng.choice([1.0, 0.98, 0.5], (n, 1, 1))     # planar, nearly planar, thick
    A = (c + sp).astype(np.float32).astype(np.float64)
    direct, ok, worst, plane = _fit(hm, A)
    for k in range(n):
        want, w, svr = R.fit_plane(A[k])
        assert svr > 1e-6
        assert np.allclose(direct[k], want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()) / svr), (k, direct[k], want)
        assert abs(worst[k] - w) < 1e-9 / svr
        if abs(w - 0.1) > 1e-9 / svr:
            assert ok[k] == (w <= 0.1)
        d = 1.0 / np.linalg.norm(direct[k])
        assert np.allclose(plane[k], np.concatenate([direct[k] * d, [d]]), rtol=1e-14, atol=0)
    assert 0.05 < ok.mean() < 0.95                                             # both verdicts occur


def test_host_qr_rank_deficient_neighbourhoods_are_finite_and_deterministic(hm):
    line = np.array([[1.0, 2.0, 3.0]]) + np.arange(5)[:, None] * np.array([[0.5, -0.25, 0.125]])
    same = np.tile([[3.0, -1.0, 2.0]], (5, 1))
    zero = np.zeros((5, 3))
    A = np.stack([line, same, zero])
    d1, ok1, w1, _ = _fit(hm, A)
    d2, ok2, w2, _ = _fit(hm, A)
    assert np.isfinite(d1).all() and np.array_equal(d1, d2) and np.array_equal(ok1, ok2)
    assert np.array_equal(d1[2], np.zeros(3)) and not ok1[2]                  # A == 0: x == 0, |0 + 1| > 0.1
    assert np.count_nonzero(d1[1]) == 1 and abs(d1[1] @ same[0] + 1) < 1e-12  # rank 1: the basic solution on the largest column
    assert np.count_nonzero(d1[0]) == 2 and np.abs(line @ d1[0] + 1).max() < 1e-9   # rank 2: a collinear set is fitted exactly by a basic solution


def test_host_world_point_and_jacobian_row(hm):
    rng = np.random.default_rng(9)
    n = 500
    s = R.pack_state(R.so3_exp(np.array([0.3, -0.2, 0.5])), np.array([1.5, -0.5, 2.0]))
    p = rng.uniform(-10, 10, (n, 3))
    nr = rng.normal(size=(n, 3)); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    plane = np.ascontiguousarray(np.concatenate([nr, rng.uniform(0, 5, (n, 1))], axis=1))
    wld = np.zeros((n, 3)); jac = np.zeros((n, 6)); resid = np.zeros(n)
    hm.inh_rows(n, s, np.ascontiguousarray(p), plane, wld, jac, resid)
    assert np.array_equal(wld, R.world_points(s, p))                          # the same expression: bit for bit
    Rm = s[:9].reshape(3, 3).T
    hat = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    for k in range(n):
        want = np.concatenate([hat(p[k]) @ Rm.T @ nr[k], nr[k]])              # jac_s as upstream writes it
        assert np.allclose(jac[k], want, rtol=0, atol=1e-13)
        j, r = R.jac_row(s, p[k], nr[k], plane[k, 3], wld[k])
        assert np.allclose(jac[k], j, rtol=0, atol=1e-13) and abs(resid[k] - r) < 1e-13


def test_host_search_order_equals_the_checkers(hm):
    rng = np.random.default_rng(11)
    c = np.ascontiguousarray(rng.normal(size=(1500, 3)).astype(np.float32)); c[900] = c[3]; c[4] = c[1200]
    q = np.ascontiguousarray(np.concatenate([c[3:4], c[1200:1201], rng.normal(size=(60, 3)).astype(np.float32)]))
    for M in (0, 4, 5, 1500):
        idx = np.zeros((q.shape[0], 5), dtype=np.int32); sqd = np.zeros((q.shape[0], 5), dtype=np.float32)
        hm.inh_knn(M, c, q.shape[0], q, idx, sqd)
        want_i, want_d = R.knn(c[:M], q)
        assert np.array_equal(idx, want_i) and np.array_equal(sqd, want_d), M


# ---- honesty of every session the GPU tests use ----------------------------------------------------------------------------------------
def _assert_honest(records):
    assert records
    for it, rec in records.items():
        assert np.min(np.abs(rec["worst"] - 0.1)) > 1e-9, (it, np.min(np.abs(rec["worst"] - 0.1)))
        assert rec["sv_ratio"].min() > 1e-6, (it, rec["sv_ratio"].min())
        assert R.near_tie_share(rec) <= 0.01, (it, R.near_tie_share(rec))


def test_honesty_one_step_session():
    _assert_honest(R.reference_step()["records"])


def test_honesty_window_session():
    for k, st in enumerate(R.reference_window()):
        if not st["result"]["seeded"]:
            _assert_honest(st["records"])


# ---- motion_init's pieces: the checker against mathematics ---------------------------------------------------------------------------------
def _to_world(xc, P):
    return P @ xc[:9].reshape(3, 3) + xc[9:12]          # R P + p, row-wise (reshape(3, 3) of the column-major block is R^T)


def test_deskew_puts_plane_points_back_on_the_plane_and_without_it_they_are_off_by_the_motion():
    c = R.make_motion_scan(400, seed=2, t_lo=1e-4)                              # every point later than the earliest head: none dropped
    P, src = R.motion_blur(c["xyz"], c["toff"], c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], c["bias_from"], c["ext"])
    assert P.shape[0] == 400 and np.array_equal(src, np.arange(399, -1, -1))
    w = _to_world(c["xc"], P)
    assert np.abs(w - c["meas"][src]).max() < 1e-12                             # the world point the float32 measurement names: to float64 rounding
    assert np.abs(w[:, 2] - 2.0).max() < 1e-6                                   # ... which lies on the plane to the float32 rounding of a measurement (6e-8 of <= 9 m)
    raw, _ = R.motion_blur(c["xyz"], None, None, None, None, 0.0, c["xc"], None, c["ext"], point_notime=True)
    off = np.abs(_to_world(c["xc"], raw)[:, 2] - 2.0)
    early = c["toff"] < 0.02                                                    # 0.08 s before the scan's end: ~0.1 m of travel, ~0.05 rad of turn
    assert off[early].min() > 5e-3 and off.max() > 0.05 and off[c["toff"] > 0.0999].max() < 1e-3


def test_upstreams_deskew_behaviours_on_three_messages_and_six_points():
    c = R.make_motion_scan(6, K=3, seed=4)
    # heads: message 1 (offt 0.05), then message 0 (offt 0).  Ascending times; every point later than 0.05: the walk reaches the first point under head 0
    toff = np.array([0.06, 0.07, 0.08, 0.09, 0.095, 0.099], dtype=np.float32)
    P, src = R.motion_blur(c["xyz"], toff, c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], c["bias_from"], c["ext"])
    assert list(src) == [5, 4, 3, 2, 1, 0, 0]                                   # descending time; the first point AGAIN under the earlier head
    tab = R.pose_table(c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], c["bias_from"])
    assert [round(e["t"], 12) for e in tab] == [0.05, 0.0]
    assert np.abs(P[5] - P[6]).max() < 1e-12 and not np.array_equal(P[5], P[6])   # the same point through two poses of one exact trajectory
    # two points at or before the earliest offset are dropped; the first point is never reached, so nothing repeats
    toff = np.array([-0.01, 0.0, 0.02, 0.04, 0.06, 0.09], dtype=np.float32)
    P, src = R.motion_blur(c["xyz"], toff, c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], c["bias_from"], c["ext"])
    assert list(src) == [5, 4, 3, 2]
    # the first point later than head 0 but not than head 1... cannot be (offsets descend); the first point between the heads: emitted once, under head 1
    toff = np.array([0.01, 0.02, 0.03, 0.06, 0.07, 0.08], dtype=np.float32)
    P, src = R.motion_blur(c["xyz"], toff, c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], c["bias_from"], c["ext"])
    assert list(src) == [5, 4, 3, 2, 1, 0]
    # one message: no pose, no output
    P, src = R.motion_blur(c["xyz"], toff, c["stamps"][:1], c["gyr"][:1], c["acc"][:1], c["beg_time"], c["xc"], c["bias_from"], c["ext"])
    assert P.shape == (0, 3)


def test_align_gravity_turns_g_onto_z_and_keeps_relative_poses():
    rng = np.random.default_rng(3)
    for sign in (1.0, -1.0):
        g = sign * 9.8 * R.so3_exp(np.array([0.05, -0.08, 0.0])) @ np.array([0, 0, 1.0])
        xs = []
        for k in range(5):
            s = np.zeros(24)
            s[:9] = R.so3_exp(rng.normal(size=3) * 0.3).T.reshape(9); s[9:12] = rng.normal(size=3); s[12:15] = rng.normal(size=3); s[15:21] = rng.normal(size=6) * 0.01
            s[21:24] = g
            xs.append(s)
        xs = np.array(xs)
        ys = R.align_gravity(xs)
        assert np.allclose(ys[:, 21:24], [0, 0, sign * 9.8], atol=1e-12)
        assert np.array_equal(ys[0, 9:12], xs[0, 9:12]) and np.array_equal(ys[:, 15:21], xs[:, 15:21])
        for k in range(1, 5):
            Ra, Rb, Sa, Sb = (z[:9].reshape(3, 3).T for z in (xs[0], xs[k], ys[0], ys[k]))
            assert np.allclose(Ra.T @ Rb, Sa.T @ Sb, atol=1e-12)
            assert np.allclose(Ra.T @ (xs[k, 9:12] - xs[0, 9:12]), Sa.T @ (ys[k, 9:12] - ys[0, 9:12]), atol=1e-12)
            assert np.allclose(Rb.T @ xs[k, 12:15], Sb.T @ ys[k, 12:15], atol=1e-12)       # body-frame velocity


# ---- ... and the host build / host entry points against the checker -----------------------------------------------------------------------------
def test_host_deskew_arithmetic_and_pose_table_against_the_checker(hm):
    from voxel_slam_amd import vxba
    c = R.make_motion_scan(300, K=7, seed=6)
    c["acc"] = c["acc"] + np.random.default_rng(1).normal(size=c["acc"].shape)          # any readings: the table is compared, not the physics
    c["gyr"] = c["gyr"] + np.random.default_rng(2).normal(size=c["gyr"].shape) * 0.1
    bias = c["xc"].copy(); bias[15:21] += 0.01
    tab = R.pose_table(c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], bias, scale=0.98)
    rows = R.pose_table_rows(tab)
    got = vxba.init_pose_table(c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], bias, scale=0.98)   # host code of the library: needs no GPU
    assert got.shape == rows.shape == (6, 22) and np.allclose(got, rows, rtol=0, atol=1e-13)
    P, src = R.motion_blur(c["xyz"], c["toff"], c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], bias, c["ext"], scale=0.98)
    assert 0 < P.shape[0] < 300                                                        # some points precede the first message
    heads = np.array([next(k for k, e in enumerate(tab) if float(c["toff"][i]) > e["t"]) for i in src])   # no repeat here: the first head a point is later than
    out = np.zeros_like(P)
    xyz32 = np.ascontiguousarray(c["xyz"].astype(np.float32)[src])
    hm.inh_deskew(P.shape[0], np.ascontiguousarray(rows[heads]), np.ones(P.shape[0], dtype=np.int32), c["xc"], c["ext"], xyz32,
                  np.ascontiguousarray(c["toff"][src].astype(np.float64)), out)
    assert np.abs(out - P).max() < 1e-12
    hm.inh_deskew(P.shape[0], np.ascontiguousarray(rows[heads]), np.zeros(P.shape[0], dtype=np.int32), c["xc"], c["ext"], xyz32,
                  np.ascontiguousarray(c["toff"][src].astype(np.float64)), out)
    assert np.array_equal(out, R.world_points(c["ext"], xyz32.astype(np.float64)))


def test_host_push_imu_against_the_checker(hm):
    from tests import _oracle as O
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(8)
    K = 12
    stamps = 5.0 + np.cumsum(rng.uniform(0.004, 0.006, K)); gyr = rng.normal(size=(K, 3)) * 0.3; acc = rng.normal(size=(K, 3)) + [0, 0, 1.0]
    bg, ba = rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05
    g, a, dt = R.push_imu_samples(stamps, gyr, acc, bg, ba, scale=9.8)
    rate = np.zeros((K - 1, 3)); am = np.zeros((K - 1, 3))
    hm.inh_midpoint(K, np.ascontiguousarray(gyr), np.ascontiguousarray(acc), bg, ba, 9.8, rate, am)
    assert np.array_equal(rate, g) and np.array_equal(am, a)
    nm = np.diag([1e-4] * 3 + [1e-2] * 3); nw = np.diag([1e-8] * 3 + [1e-6] * 3)
    f = vxba.IMU_PRE(bg, ba)
    f.push_imu(stamps, gyr, acc, 9.8, nm, nw)
    by_hand = vxba.IMU_PRE(bg, ba)
    for k in range(K - 1):
        by_hand.add_imu(g[k], a[k], dt[k], nm, nw)
    assert np.array_equal(f.blob, by_hand.blob)
    ref = O.imu_preintegrate([(g, a, dt)], nm, nw, bg, ba)[0]
    assert np.allclose(f.blob, ref, rtol=1e-9, atol=1e-12)


# ---- motion_init: the checker's new pieces, the host build of the driver's arithmetic, the honesty of its sessions --------------------------
def test_host_point_variances_and_align_gravity_against_the_checker(hm):
    rng = np.random.default_rng(31)
    pnt = rng.normal(size=(50, 3)) * 4
    pnt[7, 2] = 0.0                                                            # calcBodyVar rewrites a zero z in the point itself
    st = R.pack_state(R.so3_exp(np.array([0.3, -0.2, 0.5])), np.array([1.0, 2.0, -0.5]))
    A = rng.normal(size=(15, 15)); cov = A @ A.T * 1e-4
    want_b = [R.calc_body_var(q, 0.02, 0.05) for q in pnt]
    body = np.array([a for a, _ in want_b]); vb = np.array([b for _, b in want_b])
    vw, _ = R.pvec_update(body, vb, st, cov)
    p = pnt.copy(); bv = np.zeros((50, 9)); wv = np.zeros((50, 9))
    dir_var = np.sin(float(np.float32(0.05)) * 0.017453293) ** 2
    hm.inh_pointvar(50, p, 0.02, dir_var, np.ascontiguousarray(st[:9]), np.ascontiguousarray(cov[:3, :3].T.reshape(9)), np.ascontiguousarray(cov[3:6, 3:6].T.reshape(9)), bv, wv)
    assert np.array_equal(p, body) and p[7, 2] == 0.0001
    assert np.allclose(bv.reshape(50, 3, 3).transpose(0, 2, 1), vb, rtol=1e-12, atol=1e-18)
    assert np.allclose(wv.reshape(50, 3, 3).transpose(0, 2, 1), vw, rtol=1e-12, atol=1e-18)
    xs = np.stack([np.concatenate([R.pack_state(R.so3_exp(rng.normal(size=3) * 0.3), rng.normal(size=3))[:12], rng.normal(size=9), [0.4, -0.3, -9.7]]) for _ in range(5)])
    got = xs.copy()
    hm.inh_align_gravity(got, 5)
    assert np.allclose(got, R.align_gravity(xs), rtol=0, atol=1e-13)
    assert abs(got[0, 21]) < 1e-13 and abs(got[0, 22]) < 1e-13 and got[0, 23] < 0


def test_down_sampling_close_keeps_the_point_nearest_each_voxels_mean():
    rng = np.random.default_rng(8)
    xyz = (rng.normal(size=(3000, 3)) * 2).astype(np.float32)
    pts, sel = R.down_sampling_close(xyz, 0.5)
    keys = R.voxel_keys(xyz, 0.5)
    assert np.array_equal(pts, xyz[sel]) and len(set(map(tuple, keys))) == len(sel)
    assert [tuple(k) for k in keys[sel]] == sorted(set(map(tuple, keys)))         # one per occupied voxel, ascending voxel index
    for i in sel[:200]:
        mates = xyz[(keys == keys[i]).all(axis=1)].astype(np.float64)
        d = np.linalg.norm(mates - mates.mean(axis=0), axis=1)
        assert np.linalg.norm(xyz[i] - mates.mean(axis=0)) <= d.min() + 1e-5


def test_scatter_of_normals_counts_voxels_per_direction():
    U = np.tile(np.eye(3).T.reshape(9), (7, 1))                                   # column 0 = x for every voxel
    assert np.allclose(R.normal_scatter(U), np.diag([7.0, 0, 0]))


def _margin(value, bound):
    return abs(value - bound) / bound


@pytest.mark.parametrize("kind", ["room", "parallel", "sparse", "gravity", "initializer"])
def test_honesty_of_every_motion_init_decision(kind):
    """Every decision motion_init takes on the GPU sessions holds by a relative margin of 1e-3: the convergence ratio against the threshold in force (from
    round 2 on, where the rule is read), lambda0 against 15, |g| against 9.6 and 10.0, the factor-voxel count against 10."""
    ref = R.reference_initializer()["motion"] if kind == "initializer" else R.reference_motion(kind)
    for k, rec in enumerate(ref["rounds"]):
        assert _margin(rec["n_vox"], 10) > 1e-3 and rec["n_vox"] != 10, (k, rec["n_vox"])
        if rec["resis"] is not None and k >= 2:
            assert _margin(rec["ratio"], rec["thre"]) > 1e-3, (k, rec["ratio"], rec["thre"])
    if any(r["fired"] for r in ref["rounds"]):
        assert _margin(ref["eig"][0], 15) > 1e-3, ref["eig"]
    assert _margin(ref["gnorm"], 9.6) > 1e-3 and _margin(ref["gnorm"], 10.0) > 1e-3, ref["gnorm"]
    want = {"room": 1, "initializer": 1, "parallel": 0, "sparse": 0, "gravity": 0}[kind]
    assert ref["flag"] == want
    if kind == "parallel":
        assert ref["eig"][0] < 15 and 9.6 < ref["gnorm"] < 10.0
    if kind == "sparse":
        assert len(ref["rounds"]) == 1 and ref["rounds"][0]["n_vox"] < 10
    if kind == "gravity":
        assert ref["eig"][0] > 15 and ref["gnorm"] > 10.0


def test_honesty_initializer_session():
    for st in R.reference_initializer()["odom"]:
        if not st["result"]["seeded"]:
            _assert_honest(st["records"])


def test_motion_init_on_the_checker_recovers_gravity_and_improves_the_poses():
    """Against mathematics: from a gravity guess 3 degrees off, the converged window's gravity lies within half a degree of -z (align_gravity put it there
    exactly after the first phase; the two converged rounds behind it refine it), one vector for the whole window, and the relative poses of the window
    are nearer the truth than the propagated ones."""
    s, ref = R.motion_session("room"), R.reference_motion("room")
    g = ref["states"][0, 21:24]
    assert np.degrees(np.arctan2(np.hypot(g[0], g[1]), -g[2])) < 0.5 and (ref["states"][:, 21:24] == g).all()

    def rel_err(x):
        e = 0.0
        for i in range(1, s.win_size):
            Ra, Rb = x[0, :9].reshape(3, 3).T, x[i, :9].reshape(3, 3).T
            Ga, Gb = s.states_gt[0, :9].reshape(3, 3).T, s.states_gt[i, :9].reshape(3, 3).T
            e = max(e, np.linalg.norm(Ra.T @ (x[i, 9:12] - x[0, 9:12]) - Ga.T @ (s.states_gt[i, 9:12] - s.states_gt[0, 9:12])))
        return e
    assert rel_err(ref["states"]) < 0.5 * rel_err(s.states_init), (rel_err(ref["states"]), rel_err(s.states_init))
