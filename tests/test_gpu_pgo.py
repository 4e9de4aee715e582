"""Pose-graph optimisation on the GPU (vxba_pgo_*, vxba.PoseGraph, hba.top_down / loop_graph) against the numpy checker tests/_pgo_ref.py.
tests/test_pgo_cpu.py holds the condition these tests rest on: on every graph used here the model of the device's CG finishes inside the
default cap, the checker stops at the optimum, and none of its accept / reject decisions is taken by rounding."""
import numpy as np
import pytest

from tests import _pgo_ref as P
from tests.test_pgo_cpu import GRAPHS, RUN, make_graph
from voxel_slam_amd import synth

pytestmark = pytest.mark.gpu

# Largest deviation of the GPU's final poses from the checker's over the four graphs of test_final_poses_match_the_checkers_optimum, measured on
# an MI355X: POSE_DEV_MEASURED (translation m, rotation rad).  Asserted: ten times that (head-room for where CG stops and for the summation
# order of another ROCm), never looser than the project's contract of 1e-4 m / 1e-4 rad.
POSE_DEV_MEASURED = (7.6e-13, 1.8e-13)      # real105: 7.57e-13 m; hba1000: 1.79e-13 rad (random20 1.5e-14 / 1.5e-15, loop500 5.7e-14 / 1.6e-15)
POSE_BOUND = tuple(min(1e-4, 10 * x) for x in POSE_DEV_MEASURED)


def gpu_graph(d, poses=None):
    from voxel_slam_amd import vxba
    g = vxba.PoseGraph(d.poses if poses is None else poses)
    g.add_edges(d.edge_ij, d.edge_data)
    g.add_priors(d.prior_node, d.prior_pose, d.prior_v6)
    return g


def max_dev(a, b):
    """Largest translation [m] and rotation [rad] difference between two pose sets."""
    Ra, pa = P.unpack(a); Rb, pb = P.unpack(b)
    return float(np.linalg.norm(pa - pb, axis=1).max()), float(np.linalg.norm(P.so3_log(np.transpose(Ra, (0, 2, 1)) @ Rb), axis=1).max())


def check_against_checker(name, got, ref):
    dt, dr = max_dev(got["poses"], ref["poses"])
    print(f"{name}: GPU vs checker {dt:.3e} m {dr:.3e} rad; outer {len(got['report'])}; CG iterations {[r['cg_iterations'] for r in got['report']]}; "
          f"accepted {[r['accepted'] for r in got['report']]}; launches {got['launches']}, host synchronisations {got['host_syncs']}")
    assert not any(r["cg_capped"] for r in got["report"])
    assert [r["accepted"] for r in got["report"]] == [r["accepted"] for r in ref["report"]]
    for a, b in zip(got["report"], ref["report"]):
        assert np.isclose(a["cost_before"], b["cost_before"], rtol=1e-6) and np.isclose(a["cost_after"], b["cost_after"], rtol=1e-6)
    assert dt < POSE_BOUND[0] and dr < POSE_BOUND[1], (dt, dr)
    return dt, dr


def test_cost_and_residuals_match_the_checker():
    rng = np.random.default_rng(21)
    for d in (synth.random_pose_graph(K=20, extra_edges=30), synth.pose_graph(**GRAPHS["hba105"])):
        K = d.poses.shape[0]
        X = P.retract(d.poses, rng.normal(size=(K, 6)) * np.array([0.3] * 3 + [1.0] * 3))
        ref = make_graph(d)
        with gpu_graph(d, X) as g:
            cost, res = g.cost(want_residuals=True)
        e = ref.residuals(X)
        assert np.allclose(res, e, rtol=1e-9, atol=1e-9 * np.abs(e).max(axis=1, keepdims=True))
        assert np.isclose(cost, ref.cost(X), rtol=1e-9)


def test_one_undamped_step_is_the_dense_gauss_newton_step():
    """max_iter = 1, u tiny, CG run to 1e-12: block-Jacobi CG's error is at most sqrt(cond) x 1e-12 of the step (cond of the preconditioned
    system < 1e4 on this graph, step ~0.3): 3e-11; asserted 1e-9."""
    d = synth.random_pose_graph(K=20, extra_edges=30)
    ref = P.dense_lm(make_graph(d), d.poses, max_iter=1, u0=1e-12)
    with gpu_graph(d) as g:
        got = g.optimize(max_iter=1, u0=1e-12, cg_tol=1e-12)
    assert len(got["report"]) == 1 and got["report"][0]["accepted"] and not got["report"][0]["cg_capped"]
    dt, dr = max_dev(got["poses"], ref["poses"])
    assert dt < 1e-9 and dr < 1e-9, (dt, dr)
    assert np.isclose(got["report"][0]["predicted_decrease"], ref["report"][0]["predicted_decrease"], rtol=1e-8)


@pytest.mark.parametrize("name", ["random20", "loop500", "hba1000"])
def test_final_poses_match_the_checkers_optimum(name):
    """random20: a random connected graph; loop500: drifting chain, one prior, three loop edges; hba1000: the global-BA shape, 6 000 unknowns -- the
    CG vectors in global memory instead of LDS.  Reports: no solve ended by the cap, the checker's accept / reject sequence."""
    d = synth.random_pose_graph(K=20, extra_edges=30) if name == "random20" else synth.pose_graph(**GRAPHS[name])
    ref = P.dense_lm(make_graph(d), d.poses, **RUN)
    with gpu_graph(d) as g:
        got = g.optimize(**RUN)
        assert np.array_equal(g.read_poses(), got["poses"])
    check_against_checker(name, got, ref)
    if name == "loop500":
        R, p = P.unpack(got["poses"]); R0, p0 = P.unpack(d.poses); Rg, pg = P.unpack(d.gt)
        gap = lambda pp: np.linalg.norm((pp[499] - pp[0]) - (pg[499] - pg[0]))
        print(f"loop gap {gap(p0):.3f} m -> {gap(p):.5f} m")
        assert gap(p) < 0.05 * gap(p0)
        e0, e1 = synth.pose_errors(d.poses, d.gt), synth.pose_errors(got["poses"], d.gt)
        assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)


def test_global_ba_top_down_on_the_edges_of_a_real_pass():
    """hba.hierarchical_ba at K = 105, wdsize 10, mgsize 5 set up as in test_gpu_hba.py; its GPU edges through hba.top_down against the checker on the
    same edges; the keyframe poses end closer to the truth than the input in translation and in rotation.  Chain variances: the input poses are
    the truth perturbed independently by 0.1 deg / 0.02 m per keyframe, so a relative pose between neighbours is off by sqrt(2) of that."""
    from voxel_slam_amd import hba, vxba
    K, wdsize, mgsize = 105, 10, 5
    xyz, fp, poses, gt = synth.make_scans(win_size=K, pts_per_scan=4000, extent=24.0, noise=0.005, seed=synth.MASTER_SEED + 950 + K, rot_sigma_deg=0.1, trans_sigma=0.02)
    clouds = [xyz[fp[i]:fp[i + 1]].astype(np.float32) for i in range(K)]
    coarse = vxba.VoxelizeParams(voxel_size=2.0, max_layer=2, min_points=10, min_eigen_value=0.02, eigen_ratio=(1 / 9, 1 / 9, 1 / 9, 1 / 9))
    fine = vxba.VoxelizeParams(voxel_size=1.0, max_layer=2, min_points=10, min_eigen_value=0.01, eigen_ratio=(1 / 16, 1 / 16, 1 / 9, 1 / 9))
    up = hba.hierarchical_ba(clouds, poses, coarse, fine, wdsize=wdsize, mgsize=mgsize, top_max_iter=2)
    odom_v6 = np.array([2 * np.deg2rad(0.1) ** 2] * 3 + [2 * 0.02 ** 2] * 3)
    opt = vxba.PgoOptions(**RUN)
    got = hba.top_down(poses, odom_v6, up["edges1"], up["edges2"], options=opt)
    ref = hba.top_down(poses, odom_v6, up["edges1"], up["edges2"], options=opt, graph_cls=P.RefPoseGraph)
    check_against_checker("real105 (%d + %d BA edges)" % (len(up["edges1"]), len(up["edges2"])), got, ref)
    e0, e1 = synth.pose_errors(poses, gt), synth.pose_errors(got["poses"], gt)
    print(f"keyframes vs truth: {e0[0]:.4f} m {e0[1]:.5f} rad -> {e1[0]:.4f} m {e1[1]:.5f} rad")
    assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)
    # the whole thing in one call, and the velocity rotation of ScanPose::set_state
    both = hba.global_ba(clouds, poses, odom_v6, coarse, fine, wdsize=wdsize, mgsize=mgsize, top_max_iter=2, options=opt)
    assert np.array_equal(both["poses"], got["poses"])
    v = hba.rotate_velocities(poses, got["poses"], np.tile([1.0, 0.0, 0.0], (K, 1)))
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-12)


def test_loop_graph_driver_matches_a_hand_built_graph():
    from voxel_slam_amd import hba, vxba
    d = synth.pose_graph(**GRAPHS["loop200"])
    v6 = np.array([1e-6] * 3 + [1e-4] * 3)
    n = d.n_chain
    loops = [dict(i=int(i), j=int(j), rot=r[:9].reshape(3, 3), tra=r[9:12]) for (i, j), r in zip(d.edge_ij[n:], d.edge_data[n:])]
    got = hba.loop_graph(d.poses, loops, v6, options=vxba.PgoOptions(**RUN))
    ref = hba.loop_graph(d.poses, loops, v6, options=vxba.PgoOptions(**RUN), graph_cls=P.RefPoseGraph)
    check_against_checker("loop_graph200", got, ref)
    e0, e1 = synth.pose_errors(d.poses, d.gt), synth.pose_errors(got["poses"], d.gt)
    assert e1[0] < e0[0] and e1[1] < e0[1]


def test_structure_of_the_input():
    from voxel_slam_amd import vxba
    d = synth.random_pose_graph(K=20, extra_edges=30)
    K = 20
    with gpu_graph(d) as g:
        base = g.optimize(**RUN)
    # a repeated edge is one edge with the summed weight
    dup = d.edge_data.copy(); dup[:, 12:] *= 2
    with vxba.PoseGraph(d.poses) as g:
        g.add_edges(d.edge_ij, dup); g.add_priors(d.prior_node, d.prior_pose, d.prior_v6); g.add_edges(d.edge_ij, dup)
        twice = g.optimize(**RUN)
    dt, dr = max_dev(twice["poses"], base["poses"])
    assert dt < 1e-9 and dr < 1e-9, (dt, dr)
    # i > j: the factor (j, i, Z^-1) measures the same relative pose from the other end.  Its residual Log(Z X_j^-1 X_i) is the original's carried
    # into the frame of the other node (E' = Z E^-1 Z^-1), so with diagonal variances the two COSTS agree only where the residual vanishes;
    # what is equal is the optimum of consistent measurements: both forms must bring a perturbed guess back to the same poses, the truth.
    c = synth.random_pose_graph(K=20, extra_edges=30, noise_rot=0.0, noise_tr=0.0)
    assert (c.edge_ij[:, 0] > c.edge_ij[:, 1]).any() and (c.edge_ij[:, 0] < c.edge_ij[:, 1]).any()
    with gpu_graph(c) as g:
        fwd = g.optimize(**RUN)
    with vxba.PoseGraph(c.poses) as g:
        g.add_edges(c.edge_ij[:, ::-1].copy(), P.invert_measurement(c.edge_data)); g.add_priors(c.prior_node, c.prior_pose, c.prior_v6)
        rev = g.optimize(**RUN)
    for out in (fwd, rev):
        dt, dr = max_dev(out["poses"], c.gt)
        assert dt < 1e-9 and dr < 1e-9, (dt, dr)
    # node offsets are pre-shifted indices: bit for bit
    with vxba.PoseGraph(d.poses) as g:
        lo = d.edge_ij.copy(); lo[:, 0] -= 3; lo[:, 1] += 2
        g.add_edges(lo, d.edge_data, node_offset_i=3, node_offset_j=-2); g.add_priors(d.prior_node, d.prior_pose, d.prior_v6)
        off = g.optimize(**RUN)
    assert np.array_equal(off["poses"], base["poses"])
    # nodes without any factor keep their poses bit for bit; the others are not disturbed by them
    extra = np.concatenate([d.poses, synth.random_pose_graph(K=3, extra_edges=0, seed=5).poses])
    with vxba.PoseGraph(extra) as g:
        g.add_edges(d.edge_ij, d.edge_data); g.add_priors(d.prior_node, d.prior_pose, d.prior_v6)
        more = g.optimize(**RUN)
    assert np.array_equal(more["poses"][K:], extra[K:])
    dt, dr = max_dev(more["poses"][:K], base["poses"])
    assert dt < 1e-9 and dr < 1e-9


def test_bad_input_fails_loudly_on_the_host():
    """Input validation on the host; each case is VXBA_ERR_ARG with a message and nothing is launched."""
    from voxel_slam_amd import vxba
    d = synth.random_pose_graph(K=20, extra_edges=30)
    rec = d.edge_data[:1].copy()
    with vxba.PoseGraph(d.poses) as g:
        for ij, data, what in (([[4, 4]], rec, "itself"), ([[0, 20]], rec, "out of range"), ([[-1, 3]], rec, "out of range")):
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*" + what):
                g.add_edges(np.array(ij, dtype=np.int32), data)
        for k, v in ((12, 0.0), (17, -1.0), (14, np.nan)):
            bad = rec.copy(); bad[0, k] = v
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
                g.add_edges(np.array([[0, 1]], dtype=np.int32), bad)
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*variance"):
            g.add_priors([0], d.poses[:1], np.zeros((1, 6)))
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*out of range"):
            g.add_priors([20], d.poses[:1], np.ones((1, 6)))
        assert g.num_factors() == 0                     # nothing of a refused call was added
        # two components, a prior on one of them only: the other one is gauge-free
        g.add_edges(np.array([[0, 1], [1, 2], [10, 11]], dtype=np.int32), np.repeat(rec, 3, axis=0))
        g.add_priors([1], d.poses[1:2], np.full((1, 6), 1e-6))
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*node 10 has no prior"):
            g.optimize()
        assert np.array_equal(g.read_poses(), d.poses)
        g.add_priors([11], d.poses[11:12], np.full((1, 6), 1e-6))
        out = g.optimize()
        assert out["launches"] > 0 and np.array_equal(out["poses"][12:], d.poses[12:])
    nan = d.poses.copy(); nan[7, 10] = np.nan
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*not finite"):
        vxba.PoseGraph(nan)
    with vxba.PoseGraph(d.poses) as g:
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            g.set_poses(np.full((20, 12), np.inf))


def test_two_runs_give_identical_bits():
    d = synth.pose_graph(**GRAPHS["loop500"])
    outs = []
    for _ in range(2):
        with gpu_graph(d) as g:
            outs.append(g.optimize(**RUN))
    assert np.array_equal(outs[0]["poses"], outs[1]["poses"])
    assert outs[0]["report"] == outs[1]["report"]


def test_launch_count_does_not_depend_on_the_cg_iteration_count():
    d = synth.pose_graph(**GRAPHS["hba105"])
    with gpu_graph(d) as g:
        loose = g.optimize(max_iter=3, rel_cost_tol=0.0, cg_tol=1e-2)
    with gpu_graph(d) as g:
        tight = g.optimize(max_iter=3, rel_cost_tol=0.0, cg_tol=1e-12)
    n_loose, n_tight = sum(r["cg_iterations"] for r in loose["report"]), sum(r["cg_iterations"] for r in tight["report"])
    print(f"CG iterations {n_loose} -> {n_tight}; launches {loose['launches']} / {tight['launches']}; host synchronisations {loose['host_syncs']} / {tight['host_syncs']}")
    assert len(loose["report"]) == len(tight["report"]) == 3 and n_tight >= 2 * n_loose
    assert loose["launches"] == tight["launches"] == 6 * 3 and loose["host_syncs"] == tight["host_syncs"] == 1
