"""Loop-edge registration on the GPU (vxba_loopreg_*, vxba.LoopRegistration, hba.loop_registration) against the numpy checker
tests/_loopreg_ref.py and the reference's icp_normal (tests/golden/loop_icp).  Nearest indices, gate verdicts, match counts, iteration counts and
accept flags are compared for EQUALITY; tests/test_loopreg_cpu.py holds the conditions that make that fair on every input used here (no exact
float32 distance ties outside the one input built to have them, every verdict and step norm at least 1e-6 from its threshold)."""
import numpy as np
import pytest

from tests import _loopreg_cases as K
from tests import _loopreg_ref as R
from tests.test_loopreg_cpu import G  # noqa: F401  (the fixture that loads the golden's generator module)
from voxel_slam_amd import hba

pytestmark = pytest.mark.gpu

POSE_CONTRACT = (1e-7, 1e-7)     # m, rad: the project's standing pose contract (README)
# Largest deviation of the GPU's final poses measured on an MI355X: golden cases 5.4e-14 m / 3.1e-15 rad (case c, twenty iterations
# without convergence; a, b: 4e-16 m), 32-pair batch 6.7e-15 m / 1.7e-16 rad, the revisit's edges 5.4e-16 m / 1.0e-16 rad.
F32_ULP1 = float(np.finfo(np.float32).eps)          # one float32 ulp of a value in [1, 2): the largest a unit normal's component can have
# A plane row is the float64 centre / eigenvector ROUNDED to float32.  Checker and device agree on the float64 values to ~1e-13 (summation order,
# Jacobi against LAPACK), so the rounded outputs differ only where the float64 value sits on a float32 rounding boundary: by one ulp of that
# component, at most 6e-8 for a component below 1.  Bounds: centres 1 ulp of the component; normal components 2 ulps of 1.0 (2.4e-7: four times the
# largest single flip).  Measured on an MI355X: NORMAL_DIFF_MEASURED -- one ulp of a component of ~4e-3, in two of 11 388 rows; every other row is equal.
NORMAL_BOUND = 2 * F32_ULP1
NORMAL_DIFF_MEASURED = 4.66e-10        # largest component difference over the six clouds of test_add_keyframe_equals_the_checkers_plane_cloud


def reg():
    from voxel_slam_amd import vxba
    return vxba.LoopRegistration()


def dev(a, b):
    return R.pose_diff(a, b)


def check_report(tag, got, b, ref, pose_ref=None):
    """accept, is_converge, iterations and match_num equal; eigenvalues and resi to rounding; pose inside the contract."""
    row = got["report"][b]
    want = K.report_row(ref)
    assert row[:4].tolist() == want[:4].tolist(), (tag, row, want)
    scale = max(1.0, float(np.abs(want[4:7]).max()))
    assert np.allclose(row[4:7], want[4:7], rtol=1e-10, atol=1e-10 * scale), (tag, row, want)
    assert np.isclose(row[7], want[7], rtol=1e-9, atol=1e-15), (tag, row, want)
    dt, dr = dev(got["poses"][b], ref["pose"] if pose_ref is None else pose_ref)
    assert dt < POSE_CONTRACT[0] and dr < POSE_CONTRACT[1], (tag, dt, dr)
    return dt, dr


# ---- associate ---------------------------------------------------------------------------------------------------------------------
def test_associate_equals_the_checker_point_for_point(G):  # noqa: F811
    g = G.load_fixture()
    src, tar = g["src"], g["tar"]
    conv = R.icp(src, tar, g["a_pose0"])["pose"]
    with reg() as r:
        s, t = r.add_cloud(src), r.add_cloud(tar)
        assert (r.cloud_size(s), r.cloud_size(t)) == (src.shape[0], tar.shape[0]) and np.array_equal(r.read_cloud(s), src)
        for tag, pose in (("initial", g["a_pose0"]), ("converged", conv)):
            for gates in (R.GATES0, R.GATES1):
                nn, m = r.associate(s, t, pose, gates)
                want = R.associate(src, tar, pose, gates)
                print(f"associate {tag} {gates}: {int(m.sum())} matched of {src.shape[0]}")
                assert np.array_equal(nn, want["nn"]) and np.array_equal(m, want["matched"]) and 100 < m.sum() < src.shape[0]


def test_associate_ties_go_to_the_lowest_index(G):  # noqa: F811
    g = G.load_fixture()
    src, tar = g["src"], g["tar"]
    dup = K.duplicated_target(tar)
    with reg() as r:
        s, t = r.add_cloud(src), r.add_cloud(dup)
        nn, m = r.associate(s, t, g["a_pose0"], R.GATES0)
    want = R.associate(src, dup, g["a_pose0"], R.GATES0)
    assert want["ties"] == src.shape[0]
    assert np.array_equal(nn, want["nn"]) and np.all(nn < tar.shape[0]) and np.array_equal(m, want["matched"])


def test_associate_50000_by_50000():
    src, tar, pose = K.big_pair()
    with reg() as r:
        s, t = r.add_cloud(src), r.add_cloud(tar)
        nn, m = r.associate(s, t, pose, R.GATES0)
    want = R.associate(src, tar, pose, R.GATES0)
    assert np.array_equal(nn, want["nn"]) and np.array_equal(m, want["matched"]) and m.sum() > 100
    assert np.unique(nn // 1024).size == (tar.shape[0] + 1023) // 1024                # every LDS tile holds somebody's nearest neighbour


# ---- plane clouds --------------------------------------------------------------------------------------------------------------------
def test_add_keyframe_equals_the_checkers_plane_cloud():
    kf = K.keyframes()
    rv = K.revisit()
    clouds = dict(kf0=kf["clouds"][0], kf1=kf["clouds"][1], kf2=kf["clouds"][2], kf3=kf["clouds"][3], boundary=K.boundary_cloud(), revisit_cur=rv["cloud_cur"])
    worst_n = 0.0
    with reg() as r:
        for name, c in clouds.items():
            cid = r.add_keyframe(c)
            got = r.read_cloud(cid)
            want = R.plane_cloud(c)
            rows, lam = want["rows"], want["lam"]
            assert got.shape == rows.shape, (name, got.shape, rows.shape)                 # the same plane voxels ...
            assert np.array_equal(R.voxel_coords(got[:, :3].astype(np.float64), 1.0), want["coords"]) or name == "boundary"     # ... in the same order
            ulp_c = np.spacing(np.abs(rows[:, :3]))
            assert np.all(np.abs(got[:, :3] - rows[:, :3]) <= ulp_c), name
            well = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
            assert well.mean() >= 0.99
            dn = float(np.abs(got[well, 3:].astype(np.float64) - rows[well, 3:].astype(np.float64)).max())
            lead = got[np.arange(got.shape[0]), 3 + np.argmax(np.abs(got[:, 3:]), axis=1)]
            assert np.all(lead[well] > 0), name                                            # the sign rule
            print(f"{name}: {got.shape[0]} planes; centres differ in {int(np.any(got[:, :3] != rows[:, :3], axis=1).sum())} rows (<= 1 ulp); "
                  f"largest normal component difference {dn:.3e} ({dn / F32_ULP1:.2f} ulp of 1.0)")
            worst_n = max(worst_n, dn)
            assert dn <= NORMAL_BOUND, (name, dn)
    print(f"largest normal component difference over all clouds: {worst_n:.3e}")


def test_add_keyframe_boundaries_negative_side_and_parameters():
    from voxel_slam_amd import vxba
    pts = K.boundary_cloud()
    want = R.plane_cloud(pts)
    with reg() as r:
        got = r.read_cloud(r.add_keyframe(pts))
        assert got.shape == want["rows"].shape and np.all(np.abs(got[:, :3] - want["rows"][:, :3]) <= np.spacing(np.abs(want["rows"][:, :3])))
        # the voxel of a row is known from the checker's grouping (a centre may round onto a boundary): the count per x-cell must match
        assert want["coords"][:, 0].min() == -3 and (want["coords"][:, 0] == -3).sum() == (got[:, 0] < -2.0).sum()
        # other parameters: a coarser grid, a stricter count, a looser threshold
        kf = K.keyframes()
        for prm in (dict(voxel_size=2.0, voxel_init_num=10, plane_detection_thre=0.05), dict(voxel_size=0.5, voxel_init_num=20, plane_detection_thre=0.005)):
            got = r.read_cloud(r.add_keyframe(kf["clouds"][1], vxba.PlaneCloudParams(**prm)))
            w = R.plane_cloud(kf["clouds"][1], **prm)
            assert got.shape == w["rows"].shape and got.shape[0] > 100
            assert np.array_equal(R.voxel_coords(got[:, :3].astype(np.float64), prm["voxel_size"]), w["coords"])
        # an empty keyframe is an empty cloud; a point that is not finite is an error and adds nothing
        e = r.add_keyframe(np.zeros((0, 3)))
        assert r.cloud_size(e) == 0
        n = r.num_clouds()
        bad = pts.copy(); bad[5, 1] = np.nan
        with pytest.raises(vxba.VxbaError, match="not finite"):
            r.add_keyframe(bad)
        assert r.num_clouds() == n


# ---- score ---------------------------------------------------------------------------------------------------------------------------
def test_score_useful_counts_equal_the_checker_over_64_hypotheses():
    kf = K.keyframes()
    st, poses = K.score_batch()
    nt, dt = K.SCORE_THRESHOLDS
    with reg() as r:
        ids = [r.add_cloud(p["rows"]) for p in kf["planes"]]
        assert ids == [0, 1, 2, 3]
        sc, useful = r.score(st, poses, nt, dt)
        stats = r.stats()
        one_sc, one_useful = r.score(st[5:6], poses[5:6], nt, dt)
        stats1 = r.stats()
    want = [R.score(kf["planes"][s]["rows"], kf["planes"][t]["rows"], P, nt, dt) for (s, t), P in zip(st, poses)]
    assert useful.tolist() == [w["useful"] for w in want]
    assert np.array_equal(sc, np.array([w["score"] for w in want]))
    assert one_useful[0] == useful[5] and one_sc[0] == sc[5]
    assert (stats["launches"], stats["host_syncs"]) == (stats1["launches"], stats1["host_syncs"])


# ---- icp -----------------------------------------------------------------------------------------------------------------------------
def test_icp_golden_cases_against_the_checker_and_the_reference(G):  # noqa: F811
    g = G.load_fixture()
    worst = np.zeros(2)
    with reg() as r:
        s = r.add_cloud(g["src"])
        for c in G.CASES:
            t = r.add_cloud(G.case_target(g, c))
            eigval = float(g[f"{c}_icp_eigval"])
            got = r.icp([[s, t]], g[f"{c}_pose0"][None], icp_eigval=eigval)
            ref = R.icp(g["src"], G.case_target(g, c), g[f"{c}_pose0"], icp_eigval=eigval)
            assert bool(got["accept"][0]) == bool(int(g[f"{c}_accept"])) == ref["accept"], c
            assert np.all(np.isfinite(got["poses"])) and np.all(np.isfinite(got["report"])), c
            if c == "d":                                   # fewer than six matches: the reference is undefined beyond its verdict
                assert got["report"][0, :4].tolist() == [0.0, 0.0, 1.0, float(ref["match_num"])] and np.array_equal(got["poses"][0], g["d_pose0"])
                continue
            d1 = check_report(f"golden {c} vs checker", got, 0, ref)
            d2 = check_report(f"golden {c} vs reference", got, 0, ref, pose_ref=g[f"{c}_pose"])
            print(f"golden {c}: GPU vs checker {d1[0]:.2e} m {d1[1]:.2e} rad; vs reference {d2[0]:.2e} m {d2[1]:.2e} rad; "
                  f"iterations {int(got['iterations'][0])}, match_num {int(got['match_num'][0])}, eig {got['eig'][0]}")
            worst = np.maximum(worst, np.maximum(d1, d2))
    print(f"golden cases: largest pose deviation {worst[0]:.2e} m {worst[1]:.2e} rad")


def _run_batch(r, ids, st, poses, **kw):
    return r.icp(np.array([[ids[s], ids[t]] for s, t in st], dtype=np.int32), poses, **kw)


def test_icp_batch_of_32_against_the_checker_and_alone():
    cl = K.icp_clouds()
    st, poses = K.icp_batch()
    with reg() as r:
        ids = [r.add_cloud(c) for c in cl]
        got = _run_batch(r, ids, st, poses)
        again = _run_batch(r, ids, st, poses)
        assert np.array_equal(got["poses"], again["poses"]) and np.array_equal(got["report"], again["report"])          # two runs: the same bits
        worst = np.zeros(2)
        for b, ((s, t), P) in enumerate(zip(st, poses)):
            ref = R.icp(cl[s], cl[t], P)
            worst = np.maximum(worst, check_report(f"pair {b}", got, b, ref))
        print(f"32-pair batch: largest pose deviation from the checker {worst[0]:.2e} m {worst[1]:.2e} rad; iterations {sorted(set(got['iterations'].tolist()))}; "
              f"accepted {int(got['accept'].sum())}; launches {got['launches']}, host synchronisations {got['host_syncs']}")
        # a pair alone, and inside other batches: the same bits
        for b in (0, 7, 13, 31):
            one = _run_batch(r, ids, st[b:b + 1], poses[b:b + 1])
            assert np.array_equal(one["poses"][0], got["poses"][b]) and np.array_equal(one["report"][0], got["report"][b]), b
            assert (one["launches"], one["host_syncs"]) == (got["launches"], got["host_syncs"])                          # B = 1 and B = 32
        sub = [31, 2, 13, 13, 20]
        part = _run_batch(r, ids, st[sub], poses[sub])
        assert np.array_equal(part["poses"], got["poses"][sub]) and np.array_equal(part["report"], got["report"][sub])
        # 5 and 20 iterations: the launch plan depends on max_iter alone
        its = got["iterations"]
        assert its.min() <= 5 and its.max() == 20
        few, many = int(np.argmin(its)), int(np.argmax(its))
        a = _run_batch(r, ids, st[few:few + 1], poses[few:few + 1]); b_ = _run_batch(r, ids, st[many:many + 1], poses[many:many + 1])
        assert (a["launches"], a["host_syncs"]) == (b_["launches"], b_["host_syncs"]) == (got["launches"], got["host_syncs"]) and got["launches"] == 40


def test_icp_options_reach_the_device(G):  # noqa: F811
    g = G.load_fixture()
    with reg() as r:
        s, t = r.add_cloud(g["src"]), r.add_cloud(g["tar"])
        for kw in (dict(max_iter=3), dict(gates0=(0.3, 0.3, 0.8, 4.0), gates1=(0.15, 0.15, 0.2, 1.5)), dict(step_tol=5e-3)):
            got = r.icp([[s, t]], g["a_pose0"][None], **kw)
            ref = R.icp(g["src"], g["tar"], g["a_pose0"], **kw)
            assert ref["margin"] >= 1e-6 and ref["step_margin"] >= 1e-6 and ref["ties"] == 0, (kw, ref["margin"], ref["step_margin"])
            check_report(str(kw), got, 0, ref)
            if "max_iter" in kw:
                assert got["launches"] == 6 and int(got["iterations"][0]) == 3


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges_empty_clouds_few_matches_and_bad_ids(G):  # noqa: F811
    from voxel_slam_amd import vxba
    g = G.load_fixture()
    with reg() as r:
        s, t = r.add_cloud(g["src"]), r.add_cloud(g["tar"])
        e = r.add_cloud(np.zeros((0, 6), np.float32))
        few = r.add_cloud(G.case_target(g, "d"))
        P = g["a_pose0"]
        got = r.icp([[e, t], [s, e], [s, few], [s, t]], np.stack([P] * 4))
        assert got["accept"].tolist() == [False, False, False, True] and got["is_converge"].tolist() == [False, False, False, True]
        assert np.all(np.isfinite(got["poses"])) and np.all(np.isfinite(got["report"]))
        for b in range(3):
            assert np.array_equal(got["poses"][b], P) and got["iterations"][b] == 1
        assert got["match_num"].tolist()[:3] == [0, 0, R.icp(g["src"], G.case_target(g, "d"), P)["match_num"]]
        alone = r.icp([[s, t]], P[None])
        assert np.array_equal(alone["poses"][0], got["poses"][3]) and np.array_equal(alone["report"][0], got["report"][3])
        sc, us = r.score([[e, t], [s, e]], np.stack([P] * 2), *K.SCORE_THRESHOLDS)
        assert sc.tolist() == [0.0, 0.0] and us.tolist() == [0, 0]
        nn, m = r.associate(s, e, P, R.GATES0)
        assert np.all(nn == -1) and not m.any()
        nn, m = r.associate(e, t, P, R.GATES0)
        assert nn.size == 0 and m.size == 0
        for bad in ([[s, 99]], [[-1, t]]):
            with pytest.raises(vxba.VxbaError, match="out of range"):
                r.icp(bad, P[None])
            with pytest.raises(vxba.VxbaError, match="out of range"):
                r.score(bad, P[None])
        with pytest.raises(vxba.VxbaError, match="out of range"):
            r.associate(s, 99, P, R.GATES0)
        with pytest.raises(vxba.VxbaError, match="not finite"):
            r.icp([[s, t]], np.full((1, 12), np.nan))
        assert r.cloud_size(99) == -1
        r.clear()
        assert r.num_clouds() == 0 and r.add_cloud(g["src"]) == 0


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_end_to_end_revisit_registration_graph_poses():
    rv = K.revisit()
    got = hba.loop_registration(rv["cloud_cur"], rv["candidates"], rv["guesses"], rv["cur_index"])
    chk = K.CheckerRegistration()
    ref = hba.loop_registration(rv["cloud_cur"], rv["candidates"], rv["guesses"], rv["cur_index"], reg_cls=lambda: chk)
    assert got["useful"].tolist() == ref["useful"].tolist() and got["tried"].all() and got["accept"].tolist() == ref["accept"].tolist() and got["accept"].all()
    assert got["report"][:, :4].tolist() == ref["report"][:, :4].tolist()
    worst = np.zeros(2)
    for a, b in zip(got["edges"], ref["edges"]):
        assert (a["i"], a["j"]) == (b["i"], b["j"])
        worst = np.maximum(worst, dev(R.pose_of(a["rot"], a["tra"]), R.pose_of(b["rot"], b["tra"])))
    assert worst[0] < POSE_CONTRACT[0] and worst[1] < POSE_CONTRACT[1], worst
    out = hba.loop_graph(rv["poses"], got["edges"], K.E2E["v6"])
    before = float(np.linalg.norm(rv["poses"][-1, 9:] - rv["gt"][-1, 9:]))
    after = float(np.linalg.norm(out["poses"][-1, 9:] - rv["gt"][-1, 9:]))
    drifts = [hba.loop_drift(rv["poses"][e["i"]], rv["poses"][e["j"]], e["tra"]) for e in got["edges"]]
    print(f"revisit: registered edges differ from the checker's by {worst[0]:.2e} m {worst[1]:.2e} rad; drift seen by the edges {np.round(drifts, 3).tolist()} m; "
          f"end-point error {before:.4f} m before the loop, {after:.4f} m after")
    assert after < before
