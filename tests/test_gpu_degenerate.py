"""Degenerate voxels and non-finite residuals through every LiDAR-only LM path and the LiDAR-inertial shells (tests/_degenerate.py).

Two families of inputs no other GPU test builds: a voxel whose two smallest covariance eigenvalues are EQUAL (one point, exactly
collinear points: the gap scale sqrt(2 / (lambda_1 - lambda_0)) is infinite), and a residual sum that is NaN (a NaN or infinite
coordinate).  What the reference does with them (tests/test_oracle_degenerate.py pins the oracle to it): a non-finite residual is an
ordinary rejected step (voxel_map.hpp:423-438), the terms of a degenerate voxel land only in the blocks of the frames that observe it
(voxel_map.hpp:178, 217, 221).  So, on every path:

  * the call returns (no VXBA_ERR_STATE, no retry without fusion, no fallback counted) and returns quickly -- the waits for a residual
    that "has not arrived" used NaN as their sentinel and took a NaN sum for a missing one;
  * the accept / recompute columns of the trace are the checkers', residuals equal where finite and non-finite where theirs are;
  * poses bit-identical to the input where every step is rejected, within the neighbouring tests' tolerance otherwise.

Hessian exports: equal to the checkers' where theirs is finite (gauge rows / columns zeroed); where the reference's is poisoned, the
GPU's non-finite 6 x 6 blocks include the reference's -- the dense product of the rank-3 rows multiplies the observing frame's
non-finite row by the exact zeros of the others ("Non-finite residuals and degenerate voxels")."""
import time

import numpy as np
import pytest

from tests import _degenerate as D
from tests import _oracle as O
from tests import _ref
from voxel_slam_amd import synth

pytestmark = pytest.mark.gpu

ITERS = 4
WALL_S = 2.0          # per call: a guard against a spinning wait, not a benchmark


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


@pytest.fixture(autouse=True)
def _quiet():
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        yield


def checkers():
    out = [("oracle", O)]
    R = _ref.backend()
    if R is not None:
        out.append(("reference", R))
    return out


_CASES, _REFS = {}, {}


def case_of(name, W=5, V=300):
    key = (name, W, V)
    if key not in _CASES:
        _CASES[key] = D.make(name, W=W, V=V)
    return _CASES[key]


def ref_lm(case):
    """The checkers' damping_iter on the case (cached per case)."""
    key = (case.name, case.win_size, case.n_voxels)
    if key not in _REFS:
        out = []
        for cname, B in checkers():
            f = B.Oracle(case.win_size)
            f.push_voxels(case.clusters, case.fix, case.coe)
            f.evaluate_only_residual(case.poses_init)
            out.append((cname, f.damping_iter(case.poses_init, max_iter=ITERS, thd_num=2)))
        _REFS[key] = out
    return _REFS[key]


def gpu_factor(vx, case, **opts):
    f = vx.LidarFactor(case.win_size)
    f.push_voxels(case.clusters, case.fix, case.coe)
    for k, v in opts.items():
        if k == "precision":
            f.set_precision(v)
        else:
            f.set_option(k, v)
    f.evaluate_only_residual(case.poses_init)
    return f


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    dt = time.perf_counter() - t0
    assert dt < WALL_S, f"call took {dt:.2f} s"
    return out


def zero_gauge(H, dim=6):
    H = H.copy()
    H[:dim, :] = 0.0
    H[:, :dim] = 0.0
    return H


def check_lm(got, ref, case, tag, tol=1e-7, rtol=1e-9):
    tg, tr = got["trace"], ref["trace"]
    assert tg.shape == tr.shape, (tag, tg, tr)
    assert np.array_equal(tg[:, 6:8], tr[:, 6:8]), (tag, tg[:, 6:8], tr[:, 6:8])       # accepted / Hessian recomputed
    assert D.close_where_finite(tg[:, :2], tr[:, :2], rtol=rtol, atol=1e-15), (tag, tg[:, :2], tr[:, :2])
    if D.all_rejected(ref):
        assert np.array_equal(got["poses"], case.poses_init), tag                         # nothing moved, bit for bit
    else:
        et, er = synth.pose_errors(got["poses"], ref["poses"])
        assert et < tol and er < tol, (tag, et, er)
    if "resis" in got and "resis" in ref:
        assert D.finite_mask_equal(got["resis"], ref["resis"]), (tag, got["resis"], ref["resis"])


def check_hess_export(Hg, Hr, W, tag, rtol=1e-9):
    Hg, Hr = zero_gauge(Hg), zero_gauge(Hr)
    if np.all(np.isfinite(Hr)):
        assert np.all(np.isfinite(Hg)), (tag, D.nonfinite_blocks(Hg, W))
        assert np.allclose(Hg, Hr, rtol=rtol, atol=rtol * np.abs(Hr).max()), tag
    else:
        assert D.nonfinite_blocks(Hr, W) <= D.nonfinite_blocks(Hg, W), tag


def stats(f):
    return f.get_option("stat_fused_fallbacks"), f.get_option("stat_li_device_fallbacks")


# ---- LiDAR-only paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.CASES)
@pytest.mark.parametrize("fused_solve,fused_sweeps", [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)])
def test_damping_iter_on_degenerate_windows(vx, name, fused_solve, fused_sweeps):
    case = case_of(name)
    f = gpu_factor(vx, case, fused_solve=fused_solve, fused_sweeps=fused_sweeps)
    s0 = stats(f)
    got = timed(lambda: vx.Lidar_BA_Optimizer().damping_iter(case.poses_init, f, max_iter=ITERS))
    assert stats(f) == s0                                   # no retry without fusion, no fallback
    for cname, ref in ref_lm(case):
        check_lm(got, ref, case, (name, cname, fused_solve, fused_sweeps))
        check_hess_export(got["hess"], ref["hess"], case.win_size, (name, cname))
    # the factor is still usable afterwards: a second call from the same start gives the same answer
    f.evaluate_only_residual(case.poses_init)
    again = timed(lambda: vx.Lidar_BA_Optimizer().damping_iter(case.poses_init, f, max_iter=ITERS))
    assert np.array_equal(again["trace"][:, 6:], got["trace"][:, 6:]) and D.close_where_finite(again["poses"], got["poses"], rtol=1e-12, atol=1e-12)
    assert stats(f) == s0


@pytest.mark.parametrize("name", D.CASES)
def test_lm_steps_on_degenerate_windows(vx, name):
    """The bench driver (vxba_lm_steps): one solve of ITERS iterations is damping_iter's schedule."""
    case = case_of(name)
    f = gpu_factor(vx, case)
    f.snapshot_cache()
    s0 = stats(f)
    poses, resis, st = timed(lambda: f.lm_steps(case.poses_init, ITERS, ITERS))
    assert stats(f) == s0
    for cname, ref in ref_lm(case):
        acc = int(ref["trace"][:, 6].sum())
        if ref["trace"].shape[0] == ITERS:
            assert st == dict(iters=ITERS, accepted=acc, rejected=ITERS - acc), (cname, st)
        if D.all_rejected(ref):
            assert np.array_equal(poses, case.poses_init), cname
        else:
            et, er = synth.pose_errors(poses, ref["poses"])
            assert et < 1e-7 and er < 1e-7, (cname, et, er)


@pytest.mark.parametrize("name", D.CASES)
def test_host_driver_on_degenerate_windows(vx, name):
    """damping_iter_generic: the reference's loop on the host over the GPU's sweeps."""
    case = case_of(name)
    f = gpu_factor(vx, case)
    got = timed(lambda: vx.damping_iter_generic(case.win_size, case.poses_init, lambda xs: f.acc_evaluate2(xs), lambda xs: f.evaluate_only_residual(xs),
                                                max_iter=ITERS))
    for cname, ref in ref_lm(case):
        check_lm(got, ref, case, (name, cname))


@pytest.mark.parametrize("name", D.CASES)
@pytest.mark.parametrize("precision", ["mixed", "mixed_f32_clusters"])
def test_reduced_precision_on_degenerate_windows(vx, name, precision):
    """Mixed precision (f32 rows on the matrix cores) and the f32 re-centred cluster records: the same decisions as the checkers, poses
    within the mixed-precision tests' tolerance where steps are taken."""
    case = case_of(name)
    f = gpu_factor(vx, case, precision=precision)
    s0 = stats(f)
    got = timed(lambda: vx.Lidar_BA_Optimizer().damping_iter(case.poses_init, f, max_iter=ITERS))
    assert stats(f) == s0
    for cname, ref in ref_lm(case):
        tg, tr = got["trace"], ref["trace"]
        assert tg.shape == tr.shape and np.array_equal(tg[:, 6:8], tr[:, 6:8]), (name, cname, tg, tr)
        assert D.finite_mask_equal(tg[:, :2], tr[:, :2]), (name, cname)
        if D.all_rejected(ref):
            assert np.array_equal(got["poses"], case.poses_init)
        else:
            et, er = synth.pose_errors(got["poses"], ref["poses"])
            assert et < 1e-4 and er < 1e-4, (name, cname, et, er)


@pytest.mark.parametrize("name", ["gauge_only", "collinear", "single_point", "nan_point", "zero_residual"])
def test_wide_window_with_degenerate_voxels(vx, name):
    """W = 12 (> VXBA_MAX_WIN): the compressed-row store and the pair-major Hessian assembly."""
    case = case_of(name, W=12, V=400)
    f = gpu_factor(vx, case)
    got = timed(lambda: vx.Lidar_BA_Optimizer().damping_iter(case.poses_init, f, max_iter=ITERS))
    for cname, ref in ref_lm(case):
        check_lm(got, ref, case, (name, cname))


@pytest.mark.parametrize("name", D.CASES)
@pytest.mark.parametrize("spec", [0, 1])
def test_two_voxel_shards_on_degenerate_windows(vx, name, spec):
    """The in-process two-shard emulation (tests/test_gpu_parity.py::run_two_shards), with and without the speculative collective."""
    from tests.test_gpu_parity import run_two_shards
    case = case_of(name)
    out, calls, facs = run_two_shards(vx, case, ITERS, options=dict(spec_collective=spec))
    a, b = out
    assert np.array_equal(a["trace"][:, 6:], b["trace"][:, 6:]) and D.close_where_finite(a["poses"], b["poses"], rtol=0)
    for cname, ref in ref_lm(case):
        check_lm(a, ref, case, (name, cname, spec))
    for f in facs:
        assert f.get_option("stat_fused_fallbacks") == 0            # (a spinning wait for a residual would end in a retry without fusion)
        f.set_allreduce(None)
        f.use_external_buffers(None, None)
        f.close()


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.CASES)
def test_residual_sweep_eigenvalues_and_hessian_export(vx, name):
    """K2: per-voxel eigenvalues with the oracle's finite mask, equal where finite; residual likewise.  K3: the exported Hessian after
    the gauge is zeroed is finite and equal to the oracle's where that is finite, a superset of its non-finite blocks otherwise."""
    case = case_of(name)
    W = case.win_size
    f = gpu_factor(vx, case)
    fo = O.Oracle(W)
    fo.push_voxels(case.clusters, case.fix, case.coe)
    rg, ro = f.evaluate_only_residual(case.poses_init), fo.evaluate_only_residual(case.poses_init)
    assert D.close_where_finite(rg, ro, rtol=1e-9, atol=1e-15), (rg, ro)
    evg, _, _ = f.read_cache()
    evo, _, _ = fo.read_cache()
    assert D.close_where_finite(evg, evo, rtol=1e-6, atol=1e-11), name
    for a in case.deg:
        assert D.finite_mask_equal(evg[a], evo[a]) and (not np.all(np.isfinite(evo[a])) or np.allclose(evg[a], evo[a], rtol=1e-9, atol=1e-15)), (a, evg[a], evo[a])
    Hg, Jg, sg = f.acc_evaluate2(case.poses_init)
    Ho, Jo, so = fo.acc_evaluate2(case.poses_init)
    assert D.close_where_finite(sg, so, rtol=1e-9, atol=1e-15)
    check_hess_export(Hg, Ho, W, name)
    if name in ("gauge_only", "zero_residual"):
        assert np.all(np.isfinite(zero_gauge(Hg))) and D.close_where_finite(Jg[6:], Jo[6:], rtol=1e-9, atol=1e-9 * max(np.abs(Jo[6:]).max(), 1e-300))


def test_subranges_around_a_degenerate_voxel(vx):
    """divide_thread-style sub-ranges through acc_evaluate2(xs, head, end) / evaluate_only_residual: [0, a) in front of the collinear
    voxel is finite and equal to the oracle's sub-range -- the voxel's infinite gap scale must not reach the lanes that hold it masked."""
    case = case_of("subrange")
    W, V, a = case.win_size, case.n_voxels, case.deg[0]
    f = gpu_factor(vx, case)
    fo = O.Oracle(W)
    fo.push_voxels(case.clusters, case.fix, case.coe)
    fo.evaluate_only_residual(case.poses_init)
    for head, end in ((0, a), (a + 1, V), (0, a + 1), (a, V), (a - 5, a), (a + 1, a + 9)):
        rg, ro = f.evaluate_only_residual(case.poses_init, head, end), fo.evaluate_only_residual(case.poses_init, head, end)
        assert np.isfinite(rg) and np.isclose(rg, ro, rtol=1e-9), (head, end, rg, ro)
        Hg, Jg, sg = f.acc_evaluate2(case.poses_init, head, end)
        Ho, Jo, so = fo.acc_evaluate2(case.poses_init, head, end)
        if not head <= a < end:
            assert np.all(np.isfinite(Hg)) and np.all(np.isfinite(Jg)), (head, end, D.nonfinite_blocks(Hg, W))
            assert np.allclose(Hg, Ho, rtol=1e-9, atol=1e-9 * np.abs(Ho).max()) and np.allclose(Jg, Jo, rtol=1e-9, atol=1e-9 * np.abs(Jo).max())
        else:
            assert D.nonfinite_blocks(Ho, W) <= D.nonfinite_blocks(Hg, W), (head, end)
        assert np.isclose(sg, so, rtol=1e-9), (head, end)


def test_plane_fit_judge_on_degenerate_clusters(vx):
    """K4 on the merged clusters of the degenerate voxels (one point, collinear points, a NaN point) next to ordinary ones: the flags
    agree with the reference's criteria evaluated on the oracle's eigenvalues, NaN ratios included."""
    cl = [D.cluster_of(D.LINE), D.cluster_of(D.POINT), D.cluster_of(D.LINE * 2), D.cluster_of([(1.0, 2.0, 3.0)] * 7)]
    sc = case_of("nan_point")
    cl += [sc.clusters[sc.deg[0]].sum(axis=0)] + list(sc.clusters[:40].sum(axis=1))
    cl = np.ascontiguousarray(np.stack(cl))
    ev, _, fl = vx.plane_fit_judge(cl, min_point=5, min_eigen_value=0.0025, eigen_ratio_thre=0.05, factor_ratio_max=0.12)
    ev_ref, _ = O.plane_fit(cl)
    N = cl[:, 9]
    ref = (N > 5).astype(np.uint8) | (((ev_ref[:, 0] < 0.0025) & (ev_ref[:, 0] / ev_ref[:, 2] < 0.05)).astype(np.uint8) << 1) \
        | ((~(ev_ref[:, 0] / ev_ref[:, 1] > 0.12)).astype(np.uint8) << 2)
    assert D.finite_mask_equal(ev, ev_ref)
    assert np.array_equal(fl[:5], ref[:5]), (fl[:5], ref[:5], ev[:5], ev_ref[:5])
    margin = (np.abs(ev_ref[:, 0] - 0.0025) > 1e-9) & (np.abs(ev_ref[:, 0] / ev_ref[:, 1] - 0.12) > 1e-9)
    assert np.array_equal(fl[5:][margin[5:]], ref[5:][margin[5:]])


# ---- LiDAR-inertial shells ---------------------------------------------------------------------------------------------------------------
LI_MODES = ["host_shell_queued_sweeps", "host_shell_queued_host_pose_solve", "host_shell_plain", "host_shell_dense_solve"]


def li_setup(vx, case):
    iw, st = D.li_window(case)
    bg, ba = st[0, 15:18], st[0, 18:21]
    blobs = O.imu_preintegrate(iw.samples, iw.noise_meas, iw.noise_walk, bg, ba)
    facs = []
    for gyr, acc, dts in iw.samples:
        fac = vx.IMU_PRE(bg, ba)
        for g, a, dt in zip(gyr, acc, dts):
            fac.add_imu(g, a, dt, iw.noise_meas, iw.noise_walk)
        facs.append(fac)
    return st, blobs, facs


@pytest.mark.parametrize("name", D.LI_CASES)
@pytest.mark.parametrize("mode", LI_MODES)
@pytest.mark.parametrize("gravity", [False, True])
def test_li_shells_on_degenerate_windows(vx, name, mode, gravity):
    case = case_of(name)
    st, blobs, facs = li_setup(vx, case)
    f = gpu_factor(vx, case, li_queued_sweeps=1 if mode.startswith("host_shell_queued") else 0,
                   li_device_pose_solve=0 if mode == "host_shell_queued_host_pose_solve" else 1,
                   li_structured_solve=0 if mode == "host_shell_dense_solve" else 1)
    fused0 = f.get_option("stat_fused_fallbacks")
    iters = 3
    opt = vx.LI_BA_OptimizerGravity(imu_coef=1e-4) if gravity else vx.LI_BA_Optimizer(imu_coef=1e-4)
    got = timed(lambda: opt.damping_iter(st, f, facs, max_iter=iters))
    assert f.get_option("stat_fused_fallbacks") == fused0
    for cname, B in checkers():
        fo = B.Oracle(case.win_size)
        fo.push_voxels(case.clusters, case.fix, case.coe)
        fo.evaluate_only_residual(case.poses_init)
        ref = (B.li_damping_iter_gravity if gravity else B.li_damping_iter)(fo, st, blobs, max_iter=iters, thd_num=5, imu_coef=1e-4)
        tg, tr = got["trace"], ref["trace"]
        if tr.shape[0]:          # (the reference's own LI_BA_Optimizer keeps no trace: its states are compared below)
            assert tg.shape == tr.shape and np.array_equal(tg[:, 6:], tr[:, 6:]), (name, cname, tg, tr)
            assert D.close_where_finite(tg[:, :2], tr[:, :2], rtol=1e-7), (name, cname, tg[:, :2], tr[:, :2])
        if np.array_equal(ref["states"][:, :21], st[:, :21]):          # every step rejected
            assert D.all_rejected(got), (name, cname, tg)
            assert np.array_equal(got["states"][:, :21], st[:, :21]), (name, cname)
        else:
            et, er = synth.pose_errors(got["states"][:, :12], ref["states"][:, :12])
            assert et < 1e-7 and er < 1e-7, (name, cname, et, er)
            assert np.allclose(got["states"][:, 12:21], ref["states"][:, 12:21], atol=1e-6)
    if name == "gauge_only":
        # nothing non-finite reaches the LI shell here: not even a device-step fallback
        assert f.get_option("stat_li_device_fallbacks") == 0
