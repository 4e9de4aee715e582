"""Windows with degenerate voxels and non-finite residuals (test fixtures, no GPU needed to build them).

The synthetic windows of voxel_slam_amd.synth are well-conditioned planes: three distinct covariance eigenvalues per voxel, finite
residual sums.  The cases here put one or two hand-built voxels into such a window (or build a whole window by hand) so that

  * a voxel's two smallest eigenvalues are EQUAL (a single point, or collinear points): the gap scale sqrt(2 / (lambda_1 - lambda_0))
    is infinite;
  * a cluster carries a NaN or an infinite coordinate: the residual sum is not finite;
  * every voxel is an exact plane at exact poses: residual1 == 0 and the relative-change test is 0 / 0.

Every degenerate voxel is built from exactly representable numbers -- small-integer coordinates along an axis, seen from a frame whose
initial pose has the identity rotation and an integer translation -- so the equalities hold bit for bit in every implementation, not
up to round-off (check_exact() verifies that through the oracle).

A case is a plain namespace with the fields the LidarFactor / Oracle calls take: win_size, n_voxels, clusters (V, W, 10), fix (V, 10),
coe (V,), poses_init (W, 12), plus `deg` (indices of the hand-built voxels) and `observers` (the frames that see them).
"""
import types

import numpy as np

from voxel_slam_amd import synth

CASES = ("gauge_only", "collinear", "single_point", "nan_point", "inf_point", "subrange", "zero_residual")
LI_CASES = ("collinear", "nan_point", "gauge_only")


def cluster_of(points):
    """PointCluster::push over a few points: [xx xy xz yy yz zz | x y z | n] (exact for small integers)."""
    c = np.zeros(10)
    with np.errstate(invalid="ignore", over="ignore"):
        for x, y, z in np.asarray(points, dtype=np.float64):
            c += [x * x, x * y, x * z, y * y, y * z, z * z, x, y, z, 1.0]
    return c


def _identity_pose(p):
    out = np.zeros(12)
    out[[0, 4, 8]] = 1.0           # column-major R = I
    out[9:] = p
    return out


def _base(W, V, seed):
    # p_obs < 1: unobserved (voxel, frame) slots everywhere, the masked lanes of the Hessian sweep
    return synth.make_scene(win_size=W, pts_per_scan=60 * V, n_voxels=V, p_obs=0.8, seed=seed, rot_sigma_deg=0.2, trans_sigma=0.03)


def _case(sc, clusters, fix, coe, poses, deg, observers, name):
    return types.SimpleNamespace(name=name, win_size=sc.win_size if sc is not None else poses.shape[0], n_voxels=clusters.shape[0],
                                 clusters=np.ascontiguousarray(clusters), fix=np.ascontiguousarray(fix), coe=np.ascontiguousarray(coe),
                                 poses_init=np.ascontiguousarray(poses), deg=list(deg), observers=list(observers))


def _insert(sc, at, extra_clusters, name, observers, poses=None):
    """sc's voxels with the hand-built ones inserted in front of voxel `at` (so a sub-range boundary can fall on them)."""
    cl = np.concatenate([sc.clusters[:at], extra_clusters, sc.clusters[at:]])
    k = extra_clusters.shape[0]
    fix = np.concatenate([sc.fix[:at], np.zeros((k, 10)), sc.fix[at:]])
    coe = np.concatenate([sc.coe[:at], np.ones(k), sc.coe[at:]])
    return _case(sc, cl, fix, coe, sc.poses_init.copy() if poses is None else poses, range(at, at + k), observers, name)


# world points of the degenerate voxels: collinear along x (y, z fixed), N = 4 with sum x / N exact
LINE = [(2.0, 1.0, -1.0), (3.0, 1.0, -1.0), (4.0, 1.0, -1.0), (5.0, 1.0, -1.0)]
POINT = [(3.0, -2.0, 1.0)]


def _seen_by(world_pts, W, j, p):
    """Clusters (1, W, 10) of a voxel seen only by frame j, whose pose is (I, p) with p integer: body = world - p, exactly."""
    cl = np.zeros((1, W, 10))
    cl[0, j] = cluster_of(np.asarray(world_pts) - np.asarray(p))
    return cl


def make(name, W=5, V=300, seed=7101):
    """One case of CASES on a W-frame window of about V synthetic voxels."""
    if name == "zero_residual":
        return zero_residual_window(W, V, seed)
    sc = _base(W, V, seed)
    at = V // 2 + 3
    if name == "gauge_only":
        return _insert(sc, at, _seen_by(LINE, W, 0, np.zeros(3)), name, [0])
    # frame j >= 1 observes the degenerate voxel: its initial pose becomes (I, integer translation)
    j = W - 2
    poses = sc.poses_init.copy()
    p = np.round(poses[j, 9:])
    poses[j] = _identity_pose(p)
    if name in ("collinear", "subrange"):
        return _insert(sc, at, _seen_by(LINE, W, j, p), name, [j], poses)
    if name == "single_point":
        return _insert(sc, at, _seen_by(POINT, W, j, p), name, [j], poses)
    if name in ("nan_point", "inf_point"):
        bad = np.nan if name == "nan_point" else np.inf
        c = sc.clusters.copy()
        a = at
        i = int(np.nonzero(c[a, :, 9])[0][-1])          # one observed cluster of voxel a gets one more point with x = bad
        c[a, i] += cluster_of([(bad, 0.25, -0.5)])
        return _case(sc, c, sc.fix, sc.coe, sc.poses_init.copy(), [a], [i], name)
    raise KeyError(name)


def zero_residual_window(W=4, V=120, seed=7102):
    """Every voxel an exact plane (four points, integer in-plane coordinates) seen by four consecutive frames, every pose (I, integer p):
    residual1 == 0 bit for bit, and -- N = 16 points per voxel, so 1 / N and every mean are exact -- a gradient of exact zeros as well
    (with N = 4 W at W = 5, 1 / 20 rounds, and the kernels' gradient form leaves ~1e-15 where the reference's leaves 0)."""
    rng = np.random.default_rng(seed)
    poses = np.stack([_identity_pose([float(i), float(i % 2), 0.0]) for i in range(W)])
    cl = np.zeros((V, W, 10))
    quad = np.array([(0.0, 0.0), (2.0, 0.0), (0.0, 1.0), (2.0, 1.0)])     # in-plane spreads 1 and 1/4: distinct eigenvalues
    for a in range(V):
        ax = (a // max(W - 3, 1)) % 3          # every frame sees planes of all three orientations
        off = float(rng.integers(-6, 7))
        base = rng.integers(-8, 9, size=2).astype(np.float64)
        pts = np.zeros((4, 3))
        pts[:, ax] = off
        pts[:, (ax + 1) % 3] = base[0] + quad[:, 0]
        pts[:, (ax + 2) % 3] = base[1] + quad[:, 1]
        i0 = a % (W - 3) if W > 4 else 0
        for i in range(i0, min(i0 + 4, W)):
            cl[a, i] = cluster_of(pts - poses[i, 9:])
    return _case(None, cl, np.zeros((V, 10)), np.ones(V), poses, range(V), range(W), "zero_residual")


def check_exact(case, O):
    """The premise of a case, on the CPU through the oracle: equal eigenvalues bit for bit where the case says so."""
    f = O.Oracle(case.win_size)
    f.push_voxels(case.clusters, case.fix, case.coe)
    r = f.evaluate_only_residual(case.poses_init)
    ev, _, _ = f.read_cache()
    if case.name in ("gauge_only", "collinear", "subrange"):
        for a in case.deg:
            assert ev[a, 0] == 0.0 and ev[a, 1] == 0.0 and ev[a, 2] > 0, ev[a]
    elif case.name == "single_point":
        for a in case.deg:
            assert np.all(ev[a] == 0.0), ev[a]
    elif case.name == "zero_residual":
        assert r == 0.0 and np.all(ev[:, 0] == 0.0) and np.all(ev[:, 1] > 0)
    elif case.name in ("nan_point", "inf_point"):
        assert not np.isfinite(r)
    return r, ev


def li_window(case, seed=7103):
    """IMU factors and initial states for a case's window (synth.make_imu on the same trajectory), the states' poses replaced by the
    case's initial poses so the degenerate voxels keep their exact premise."""
    sc = types.SimpleNamespace(win_size=case.win_size, poses_init=case.poses_init, poses_gt=case.poses_init)
    iw = synth.make_imu(sc, seed=seed)
    st = iw.states_init.copy()
    st[:, :12] = case.poses_init
    return iw, st


# ---- NaN-aware comparisons ------------------------------------------------------------------------------------------------------------
def finite_mask_equal(a, b):
    return np.array_equal(np.isfinite(a), np.isfinite(b))


def close_where_finite(a, b, rtol=1e-9, atol=0.0):
    """Same finite / non-finite mask (NaN and inf are not told apart), and equal to rtol where finite."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not finite_mask_equal(a, b):
        return False
    m = np.isfinite(b)
    return bool(np.allclose(a[m], b[m], rtol=rtol, atol=atol))


def nonfinite_blocks(H, W, dim=6):
    """Set of (i, j) frame blocks of a (dim W)^2 matrix holding a non-finite entry."""
    return {(i, j) for i in range(W) for j in range(W) if not np.all(np.isfinite(H[dim * i:dim * i + dim, dim * j:dim * j + dim]))}


def all_rejected(lm):
    return bool(np.all(lm["trace"][:, 6] == 0))
