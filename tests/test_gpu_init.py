"""Initialisation on the GPU: the scan-to-cloud odometry (vxba.InitOdometry, csrc/vxba_init.hip) against the numpy checker tests/_init_ref.py.
The sessions are the ones tests/test_init_cpu.py proves honest: no gate verdict within 1e-9 of its threshold, no neighbourhood of singular-value
ratio below 1e-6, at most 1 % of points with a 5th / 6th neighbour tie within 4 float32 ulps."""
import numpy as np
import pytest

from tests import _init_ref as R

pytestmark = pytest.mark.gpu

IDENT = R.pack_state(np.eye(3), np.zeros(3))
COV = np.eye(15) * 1e-2


def _pose_diff(a, b):
    Ra, Rb = a[:9].reshape(3, 3).T, b[:9].reshape(3, 3).T
    return float(np.linalg.norm(a[9:12] - b[9:12])), float(np.linalg.norm(R.so3_log(Ra.T @ Rb)))


def _seeded(vxba, cloud32):
    """A handle whose resident cloud is exactly cloud32 (one seeding step under the identity: no filter in that branch)."""
    g = vxba.InitOdometry()
    if cloud32.shape[0]:
        r = g.step(cloud32.astype(np.float64), IDENT, COV)
        assert r["seeded"] and r["iterations"] == 0
    assert g.cloud_size() == cloud32.shape[0] and np.array_equal(g.cloud(), cloud32)
    return g


# 2500 = two LDS tiles of 1024 and a remainder of 452
@pytest.mark.parametrize("M", [0, 4, 5, 99, 100, 101, 2500])
def test_search_alone_equals_the_checker(M):
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(100 + M)
    cloud = rng.normal(size=(M, 3)).astype(np.float32) * 3
    if M >= 100:                                                              # exact duplicates, far apart in index and across tiles
        cloud[M - 1] = cloud[2]; cloud[57] = cloud[2]; cloud[3] = cloud[M - 7]
    g = _seeded(vxba, cloud)
    for nq in (1, 63, 64, 65, 200):                                           # 200: three workgroups of 64 queries and a remainder
        q = rng.normal(size=(nq, 3)).astype(np.float32) * 3
        if M >= 100:
            q[0] = cloud[2]
            if nq > 1:
                q[nq - 1] = cloud[3]
        idx, sqd = g.search(q)
        want_i, want_d = R.knn(cloud, q)
        assert np.array_equal(idx, want_i), (M, nq)
        assert np.array_equal(sqd, want_d), (M, nq)
        if M >= 100:
            assert list(idx[0][:3]) == [2, 57, M - 1] and (sqd[0][:3] == 0).all()            # equal distances: the lower index first
            if nq > 1:
                assert list(idx[nq - 1][:2]) == [3, M - 7]
        if M < 5:
            assert (idx[:, M:] == -1).all() and np.isinf(sqd[:, M:]).all()
    g.close()


def test_fewer_than_100_points_seed_and_100_align():
    from voxel_slam_amd import vxba
    room = R.make_room(400, seed=21, extent=3.0).astype(np.float32)
    g = _seeded(vxba, room[:99])
    s = R.pack_state(R.so3_exp(np.array([0.02, -0.01, 0.03])), np.array([0.1, 0.0, -0.1]))
    one = np.array([[0.5, 0.25, -3.0]])
    r = g.step(one, s, COV)                                                   # 99 < 100: appended under the state, no filter, state untouched
    assert r["seeded"] and np.array_equal(r["state"], s) and np.array_equal(r["cov"], COV) and g.cloud_size() == 100
    assert np.array_equal(g.cloud()[99], R.world_points(s, one).astype(np.float32)[0])
    ref = R.InitOdometryRef(); ref.cloud_ = g.cloud()
    scan = room[100:400].astype(np.float64)
    r = g.step(scan, IDENT, COV); w = ref.step(scan, IDENT, COV)             # 100: the EKF branch
    assert not r["seeded"] and r["iterations"] == w["iterations"] and r["valid"] == w["valid"] and r["refind"] == w["refind"]
    assert g.cloud_size() == ref.cloud_size() < 400
    g.clear()
    assert g.cloud_size() == 0 and g.step(one, s, COV)["seeded"] and g.cloud_size() == 1
    g.close()


@pytest.fixture(scope="module")
def one_step():
    from voxel_slam_amd import vxba
    ref = R.reference_step()
    case = ref["case"]
    g = _seeded(vxba, ref["cloud_before"])
    got = g.step(case["scan_body"], case["state_init"], case["cov"])
    rec = {it: g.inspect(it) for it in range(got["iterations"]) if got["refind"][it]}
    out = dict(ref=ref, got=got, rec=rec, cloud=g.cloud(), stats=g.stats())
    with pytest.raises(vxba.VxbaError):
        g.inspect(1 if not got["refind"][1] else 3)
    g.close()
    return out


def test_one_step_first_refind_is_the_checkers(one_step):
    """6 000 scan points against 20 000 cloud points: same float inputs, so indices, order, verdicts and valid are equal with no exclusions."""
    ref, got, rec = one_step["ref"], one_step["got"], one_step["rec"]
    want = ref["records"][0]
    assert ref["cloud_before"].shape[0] == 20000 and want["nn"].shape == (6000, 5)
    assert np.array_equal(rec[0]["nn"], want["nn"])
    assert np.array_equal(rec[0]["ok"], want["ok"])
    assert got["valid"][0] == ref["result"]["valid"][0] == int(want["ok"].sum())
    acc = want["ok"]
    assert np.allclose(rec[0]["n"][acc], want["n"][acc], rtol=0, atol=1e-9) and np.allclose(rec[0]["d"][acc], want["d"][acc], rtol=1e-9, atol=0)


def test_one_step_schedule_later_refinds_and_result(one_step):
    ref, got, rec = one_step["ref"], one_step["got"], one_step["rec"]
    want = ref["result"]
    assert got["iterations"] == want["iterations"] and got["refind"] == want["refind"] and got["rematch_num"] == want["rematch_num"]
    assert got["valid"] == want["valid"]
    assert sorted(rec) == sorted(ref["records"]) and len(rec) >= 2           # the session searches again at least once
    for it in sorted(rec)[1:]:
        w = ref["records"][it]
        keep = ~R.near_tie_mask(w)                                            # the only points a set comparison may leave out: <= 1 % (CPU suite)
        assert keep.mean() >= 0.99
        assert np.array_equal(np.sort(rec[it]["nn"][keep], axis=1), np.sort(w["nn"][keep], axis=1)), it
        assert np.array_equal(rec[it]["ok"][keep], w["ok"][keep]), it
    for k in range(got["iterations"]):
        assert np.allclose(got["sweeps"][k]["HTH"], want["sweeps"][k]["HTH"], rtol=1e-9, atol=1e-9 * np.abs(want["sweeps"][k]["HTH"]).max())
    et, er = _pose_diff(got["state"], want["state"])
    print(f"one step: pose diff vs the checker {et:.3e} m / {er:.3e} rad; |v,bg,ba| diff {np.abs(got['state'][12:21] - want['state'][12:21]).max():.3e}")
    assert et < 1e-7 and er < 1e-7
    assert np.abs(got["state"][12:21] - want["state"][12:21]).max() < 1e-6
    assert np.array_equal(got["state"][21:24], want["state"][21:24])         # gravity is not estimated here
    sd = np.sqrt(np.abs(np.diag(want["cov"])))
    assert np.all(np.abs(got["cov"] - want["cov"]) <= 1e-6 * np.outer(sd, sd))      # rtol 1e-6 of what bounds the entry, sqrt(c_ii c_jj): no fixed atol
    assert np.abs(got["cov"] - want["cov"]).max() <= 1e-6 * np.abs(want["cov"]).max()


def test_one_step_cloud_after_append_and_filter(one_step):
    ref, cloud = one_step["ref"], one_step["cloud"]
    assert cloud.shape == ref["cloud_after"].shape
    assert np.abs(cloud - ref["cloud_after"]).max() <= 1e-6


def test_window_of_steps_keeps_the_checkers_cloud():
    """Five steps from an empty handle.  Which case holds: measured on the MI355X the poses of checker and product differ by at most 7.9e-16 m /
    1.1e-16 rad, far inside the float rounding of an appended point (6e-8 relative), and the resident cloud was bit-identical to the checker's
    after every one of the five steps (1 500, 2 382, 3 267, 3 919, 4 451 points).  Asserted: equal counts and every coordinate within 1e-6 always, and
    bit for bit whenever the poses agree within 1e-10 -- three orders below the float rounding of an appended point."""
    from voxel_slam_amd import vxba
    ref = R.reference_window()
    g = vxba.InitOdometry()
    exact = []
    for k, st in enumerate(ref):
        got = g.step(st["inp"]["scan_body"], st["inp"]["state_init"], st["inp"]["cov"])
        want = st["result"]
        assert got["seeded"] == want["seeded"] == (k == 0)
        assert got["iterations"] == want["iterations"] and got["refind"] == want["refind"] and got["valid"] == want["valid"], k
        et, er = _pose_diff(got["state"], want["state"])
        assert et < 1e-7 and er < 1e-7, (k, et, er)
        cloud = g.cloud()
        assert cloud.shape == st["cloud"].shape, k
        assert np.abs(cloud - st["cloud"]).max() <= 1e-6, k
        exact.append(bool(np.array_equal(cloud, st["cloud"])))
        if max(et, er) < 1e-10:                                               # three orders below the float rounding of an appended point (6e-8 relative of metres)
            assert exact[-1], k
        print(f"window step {k}: pose diff {et:.2e} m / {er:.2e} rad, cloud {cloud.shape[0]} points, bit-identical: {exact[-1]}")
    assert exact[0]                                                           # the seeding step involves no estimate
    g.close()


def test_launches_and_waits_do_not_depend_on_the_cloud_size(one_step):
    from voxel_slam_amd import vxba
    case = one_step["ref"]["case"]
    small = _seeded(vxba, one_step["ref"]["cloud_before"][:300])
    r = small.step(case["scan_body"][:500], case["state_init"], case["cov"])
    assert not r["seeded"]
    a, b = small.stats(), one_step["stats"]
    assert (a["launches"], a["syncs"]) == (b["launches"], b["syncs"]) == (13, 1)
    small.close()


# ---- the map's threshold switch (the two phases of motion_init) ------------------------------------------------------------------------
def test_map_set_plane_thresholds_equals_a_map_created_with_them():
    from tests import _oracle as O
    from tests.test_oracle_octree import point_vars, to_world
    from voxel_slam_amd import synth, vxba
    base = dict(voxel_size=1.0, max_layer=2, min_point=(20, 20, 15, 10), win_size=3, thread_num=1)
    first = dict(min_eigen_value=0.02, plane_eigen_value_thre=(0.25, 0.25, 0.25, 0.25))          # motion_init's first phase
    later = dict(min_eigen_value=0.0025, plane_eigen_value_thre=(1 / 16, 1 / 16, 1 / 9, 1 / 9))  # a caller's own
    xyz, fp, poses, _ = synth.make_scans(win_size=3, pts_per_scan=6000, seed=synth.MASTER_SEED + 77)
    var = point_vars(xyz.shape[0], 5)

    def build(m, f):
        for k in range(3):
            s = slice(fp[k], fp[k + 1])
            m.cut_voxel(k, xyz[s], var[s], to_world(poses[k], xyz[s]))
        m.recut(3, poses[:3], f)
        lv = m.leaves()
        o = np.argsort(lv["node_id"], kind="stable")
        return {k: v[o] for k, v in lv.items() if isinstance(v, np.ndarray) and v.shape[:1] == o.shape}

    switched, created, other = vxba.LocalMap(**base, **first), vxba.LocalMap(**base, **later), vxba.LocalMap(**base, **first)
    switched.set_plane_thresholds(later["min_eigen_value"], later["plane_eigen_value_thre"])     # a new map is empty
    fs, fc, fo = vxba.LidarFactor(3), vxba.LidarFactor(3), vxba.LidarFactor(3)
    a, b, c = build(switched, fs), build(created, fc), build(other, fo)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert fs.size() == fc.size() > 10
    chk = O.LocalMapOracle(**base, **later); fchk = O.Oracle(3)
    w = build(chk, fchk)
    assert np.array_equal(a["node_id"], w["node_id"]) and np.array_equal(a["is_plane"].astype(bool), np.asarray(w["is_plane"]).astype(bool))
    assert not (np.array_equal(a["node_id"], c["node_id"]) and np.array_equal(a["is_plane"], c["is_plane"]))   # the thresholds matter on this scene
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_STATE"):
        switched.set_plane_thresholds(0.02, (0.25,) * 4)                                         # refused on a map that holds anything
    assert switched.leaves()["node_id"].shape == a["node_id"].shape                              # ... and nothing changed
    switched.clear(); fs.clear()
    switched.set_plane_thresholds(first["min_eigen_value"], first["plane_eigen_value_thre"])     # after a clear it is legal again
    d = build(switched, fs)
    for k in c:
        assert np.array_equal(c[k], d[k]), k
    with pytest.raises(vxba.VxbaError):
        switched.set_plane_thresholds(-1.0, (0.25,) * 4)
    for m in (switched, created, other):
        m.close()


def test_bad_input_is_turned_away_before_any_launch():
    from voxel_slam_amd import vxba
    room = R.make_room(300, seed=5, extent=3.0).astype(np.float32)
    g = _seeded(vxba, room[:200])
    bad = room[200:260].astype(np.float64); bad[7, 1] = np.nan
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        g.step(bad, IDENT, COV)
    bad[7, 1] = np.inf
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        g.step(bad, IDENT, COV)
    s = IDENT.copy(); s[9] = np.nan
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        g.step(room[200:260].astype(np.float64), s, COV)
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        g.step(room[200:260].astype(np.float64), IDENT, np.zeros((15, 15)))   # singular covariance
    assert g.cloud_size() == 200 and np.array_equal(g.cloud(), room[:200])    # nothing happened to the cloud
    assert not g.step(room[200:260].astype(np.float64), IDENT, COV)["seeded"]
    g.close()


# ---- pieces of motion_init: the de-skew kernel and the normals' scatter ---------------------------------------------------------------------
def _deskew_both(vxba, c, toff, **kw):
    args = (c["stamps"], c["gyr"], c["acc"], c["beg_time"], c["xc"], c["bias_from"], c["ext"])
    got = vxba.init_deskew(c["xyz"], toff, *args, **kw)
    want = R.motion_blur(c["xyz"], toff, *args, **kw)
    assert got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert np.array_equal(got[1], want[1])                                    # the same points in the same order
    if want[0].size:
        assert np.abs(got[0] - want[0]).max() < 1e-12
    return got


@pytest.mark.parametrize("n", [1, 2, 65, 5000])
def test_deskew_kernel_writes_upstreams_sequence(n):
    """A 7-message table (six poses, offsets 0.1 * k / 6).  Three time layouts per size: spread from before the first message (points dropped; the first
    point is never reached); all later than the last head (the walk reaches the first point under head 0 and emits it again under all five earlier heads);
    the first point between two heads.  Then point_notime."""
    from voxel_slam_amd import vxba
    c = R.make_motion_scan(n, K=7, seed=30 + n)
    c["gyr"] = c["gyr"] + np.random.default_rng(n).normal(size=c["gyr"].shape) * 0.05    # any readings: sequence and arithmetic are compared, not the physics
    c["acc"] = c["acc"] + np.random.default_rng(n + 1).normal(size=c["acc"].shape) * 0.5
    rng = np.random.default_rng(n + 2)
    spread = c["toff"]
    late = np.sort(rng.uniform(0.085, 0.0999, n)).astype(np.float32)          # every point later than the last head (offset 5/6 * 0.1)
    between = np.sort(np.concatenate([[0.04], rng.uniform(0.04, 0.0999, n - 1)])).astype(np.float32)
    P, src = _deskew_both(vxba, c, spread)
    if n >= 65:
        assert 0 < src.shape[0] < n and src[-1] > 0                            # dropped points, no repeat
    P, src = _deskew_both(vxba, c, late)
    assert src.shape[0] == n + 5 and list(src[-6:]) == [0] * 6                 # the first point six times: once per head
    P, src = _deskew_both(vxba, c, between)
    assert src.shape[0] == n + 2 and list(src[-3:]) == [0] * 3                 # 0.04 lies after the heads at 0.0333, 0.0167 and 0
    P, src = _deskew_both(vxba, c, None, point_notime=True)
    assert np.array_equal(src, np.arange(n))


@pytest.mark.parametrize("V", [1, 63, 64, 65, 3000])
def test_normal_scatter_kernel_sums_the_cached_normals(V):
    from voxel_slam_amd import synth, vxba
    sc = synth.make_scene(win_size=3, pts_per_scan=max(40 * V, 200), n_voxels=V, seed=500 + V)
    f = vxba.LidarFactor(sc.win_size)
    f.push_points(sc.n_voxels, sc.points_body, sc.cell_ptr)
    f.evaluate_only_residual(sc.poses_init)                                   # fills eig_values / eig_vectors / pcr_adds, as upstream
    assert f.size() == V
    _, U, _ = f.read_cache()
    nrm = U[:, :3]                                                            # column 0 of the column-major 3 x 3
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
    got = vxba.init_normal_scatter(f)
    want = nrm.T @ nrm
    assert np.abs(got - want).max() <= 1e-12 * V and np.array_equal(got, got.T)
    assert np.array_equal(got, vxba.init_normal_scatter(f))                   # a fixed tree: the same bits again
    f.close()


# ---- motion_init end to end ------------------------------------------------------------------------------------------------------------------
def _run_motion(kind):
    from voxel_slam_amd import vxba
    s, ref = R.motion_session(kind), R.reference_motion(kind)
    W = s.win_size
    m = vxba.LocalMap(win_size=W, thread_num=1, **R.MOTION_MAP)
    f = vxba.LidarFactor(W)
    x = s.states_init
    facs = []
    for i in range(1, W):
        fac = vxba.IMU_PRE(x[i - 1, 15:18], x[i - 1, 18:21])
        fac.push_imu(*s.imus[i], s.imupre_scale_gravity, s.noise_meas, s.noise_walk)
        facs.append(fac)
    got = vxba.motion_init(m, f, s.scans, s.beg_times, s.imus, x, s.covs, s.ext, facs, s.noise_meas, s.noise_walk, R.MOTION_MAP["min_eigen_value"],
                           R.MOTION_MAP["plane_eigen_value_thre"], imupre_scale_gravity=s.imupre_scale_gravity)
    return s, ref, got, m, f, facs


def _same_rounds(got, ref):
    assert len(got["rounds"]) == len(ref["rounds"]), (len(got["rounds"]), len(ref["rounds"]))
    for k, (a, b) in enumerate(zip(got["rounds"], ref["rounds"])):
        print("round", k, a["n_vox"], b["n_vox"], a["phase"], b["phase"], a["resis"], b["resis"], a["fired"], b["fired"])
        assert a["n_vox"] == b["n_vox"] and a["phase"] == b["phase"] and a["fired"] == b["fired"] and a["thre"] == b["thre"], k
        assert a["solved"] == (b["resis"] is not None), k
        if a["solved"]:
            assert np.array_equal(a["trace"][:, 6:], b["trace"][:, 6:]), k
            assert np.allclose(a["resis"], b["resis"], rtol=1e-7, atol=0), (k, a["resis"], b["resis"])


def test_motion_init_end_to_end_equals_the_checker():
    """The smallest converging session found: win_size 6, 1 500 points per scan (a tilted six-wall room of 6.6 m, 5 % clutter) -- five rounds, 88-103 factor
    voxels per round, smallest scatter eigenvalue 23.9 against 15.  At 1 000 points per scan the same room leaves 48 converged-phase voxels and the smallest
    eigenvalue falls to 14.3: degenerate.  (win_size 5 at 1 500 points converges too, with 76-83 voxels; 6 is kept so that the Initializer test shares it.)"""
    s, ref, got, m, f, facs = _run_motion("room")
    assert got["flag"] == ref["flag"] == 1
    _same_rounds(got, ref)
    W = s.win_size
    dp = max(_pose_diff(got["states"][i], ref["states"][i])[0] for i in range(W)); dr = max(_pose_diff(got["states"][i], ref["states"][i])[1] for i in range(W))
    dv = np.abs(got["states"][:, 12:24] - ref["states"][:, 12:24]).max()
    print("pose diff", dp, dr, "v/bg/ba/g diff", dv, "eig", got["eig"], ref["eig"])
    assert dp < 1e-7 and dr < 1e-7, (dp, dr)
    assert dv < 1e-6, dv
    assert 9.6 <= np.linalg.norm(got["states"][W - 1, 21:24]) <= 10.0
    assert np.allclose(got["eig"], ref["eig"], rtol=1e-6)
    assert np.allclose(np.stack([fc.blob for fc in facs]), ref["blobs"], rtol=1e-6, atol=1e-9)
    lv, want = m.leaves(), ref["leaves"]
    assert np.array_equal(np.sort(lv["node_id"]), np.sort(want["node_id"]))                    # the map's leaf set after success
    o, p = np.argsort(lv["node_id"]), np.argsort(want["node_id"])
    assert np.array_equal(lv["is_plane"][o], want["is_plane"][p])
    assert f.size() == ref["rounds"][-1]["n_vox"]


@pytest.mark.parametrize("kind", ["parallel", "sparse", "gravity"])
def test_motion_init_exits(kind):
    """parallel: floor and ceiling only, the normals' scatter is degenerate; sparse: clutter only, fewer than 10 factor voxels in round 0; gravity: the IMU
    senses 10.3 m/s^2, so the estimated norm ends outside [9.6, 10.0].  Flag 0, map and factor empty, as the checker."""
    s, ref, got, m, f, facs = _run_motion(kind)
    assert ref["flag"] == 0 and got["flag"] == 0
    _same_rounds(got, ref)
    if kind == "sparse":
        assert len(got["rounds"]) == 1 and not got["rounds"][0]["solved"] and got["rounds"][0]["n_vox"] < 10
    if kind == "parallel":
        assert got["eig"][0] < 15 and np.allclose(got["eig"], ref["eig"], rtol=1e-6, atol=1e-9)
    if kind == "gravity":
        gn = np.linalg.norm(got["states"][-1, 21:24])
        assert got["eig"][0] >= 15 and gn > 10.0 and abs(gn - ref["gnorm"]) < 1e-6
    c = m.counts()
    assert c["leaves"] == 0 and c["roots"] == 0 and f.size() == 0


@pytest.mark.parametrize("n", [1, 65, 3000])
def test_down_sampling_close_equals_the_checker(n):
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(60 + n)
    xyz = (rng.normal(size=(n, 3)) * 2).astype(np.float32)
    if n > 10:
        xyz[5] = xyz[9]                                                         # equal distances to the mean: the first in cloud order
    for size in (0.5, 0.13, 0.0005):                                            # below 0.001 the cloud passes through
        pts, sel = vxba.down_sampling_close(xyz, size)
        want_p, want_s = R.down_sampling_close(xyz, size)
        assert np.array_equal(sel, want_s) and np.array_equal(pts, want_p), (n, size)


def test_initializer_end_to_end_and_hand_over_to_the_regular_loop():
    """Raw scans, raw IMU and propagated states in: 0 for the first win_size - 1 scans, 1 on the last; the states motion_init received and returned agree
    with the checker's driver; then LI_BA_Optimizer.damping_iter on the returned map's factor, states and IMU factors agrees with the oracle."""
    from tests import _oracle as O
    from voxel_slam_amd import vxba
    from voxel_slam_amd.init import Initializer
    s, ref = R.motion_session("room"), R.reference_initializer()
    ini = Initializer(s.win_size, s.ext, s.noise_meas, s.noise_walk, imupre_scale_gravity=s.imupre_scale_gravity, **R.MOTION_MAP)
    rets = []
    for i in range(s.win_size):
        rets.append(ini.push_scan(s.scans[i], s.imus[i], s.states_init[i], s.covs[i], s.beg_times[i]))
        if i < s.win_size - 1:
            dp, dr = _pose_diff(ini.states[i], ref["states_in"][i])
            print("odom", i, dp, dr)
            assert dp < 1e-7 and dr < 1e-7, (i, dp, dr)
            assert np.array_equal(ini.scans[i][0], ref["scans"][i][0]) and np.array_equal(ini.scans[i][1], ref["scans"][i][1])
    assert rets == ref["returns"] == [0] * (s.win_size - 1) + [1]
    mot = ref["motion"]
    _same_rounds(ini.report, mot)
    got = np.stack(ini.states)
    dp = max(_pose_diff(got[i], mot["states"][i])[0] for i in range(s.win_size)); dr = max(_pose_diff(got[i], mot["states"][i])[1] for i in range(s.win_size))
    dv = np.abs(got[:, 12:24] - mot["states"][:, 12:24]).max()
    print("initializer pose diff", dp, dr, "v/bg/ba/g", dv)
    assert dp < 1e-7 and dr < 1e-7 and dv < 1e-6, (dp, dr, dv)
    # the hand-over: the regular LiDAR-inertial BA on what the initialisation left
    want = O.li_damping_iter(mot["factor"], mot["states"], mot["blobs"], max_iter=3, thd_num=1, imu_coef=1e-4)
    have = vxba.LI_BA_Optimizer(imu_coef=1e-4).damping_iter(got, ini.factor, ini.imus_factor, max_iter=3)
    assert np.array_equal(have["trace"][:, 6:], want["trace"][:, 6:]) and np.allclose(have["trace"][:, :2], want["trace"][:, :2], rtol=1e-6)
    dp = max(_pose_diff(have["states"][i], want["states"][i])[0] for i in range(s.win_size)); dr = max(_pose_diff(have["states"][i], want["states"][i])[1] for i in range(s.win_size))
    assert dp < 1e-6 and dr < 1e-6, (dp, dr)
