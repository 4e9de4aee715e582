"""Deterministic synthetic sliding-window scenes for the local-BA hot path.

Input synthesis only (no BA arithmetic lives here): a voxel lattice of planar
patches observed from W poses, emitted in the formats the boundary consumes --
body-frame points bucketed per (frame, voxel) cell for K1, or pre-built
per-(voxel, frame) clusters for ``push_voxels``.  Follows the recipe of
SURVEY.md section 8(d): voxel_size 1 m (reference voxelslam.cpp:795), range noise
sigma 0.02 m along the normal (``dept_err``, voxelslam.cpp:793), three near-
orthogonal normal families so the window is fully constrained, trajectory
p_i = (0.5 i, 0.1 sin i, 0), R_i = Exp(0.02 i a), frame 0 exact (gauge).

Packed formats (same as include/vxba.h):
  cluster : 10 f64 [Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N]
  pose    : 12 f64 [R col-major (9) | p (3)]
"""
from __future__ import annotations

import dataclasses

import numpy as np

MASTER_SEED = 20250410

# name -> (W, pts/scan, voxels); BASELINE.json configs[0..3]
CONFIGS = {
    "cfg1": dict(win_size=5, pts_per_scan=20_000, n_voxels=5_000),
    "cfg2": dict(win_size=10, pts_per_scan=100_000, n_voxels=50_000),
    "cfg3": dict(win_size=10, pts_per_scan=200_000, n_voxels=100_000),
    "cfg4": dict(win_size=10, pts_per_scan=1_000_000, n_voxels=400_000),
    # SURVEY 8d's secondary runs of cfg2: half the (voxel, frame) incidences missing; 30 % of the voxels with a world-frame fix cluster
    "cfg2_sparse": dict(win_size=10, pts_per_scan=100_000, n_voxels=50_000, p_obs=0.5),
    "cfg2_fix": dict(win_size=10, pts_per_scan=100_000, n_voxels=50_000, fix_frac=0.3),
    # development: cfg2 with a voxel count that fills whole steps of the Hessian sweep on 256 CUs (256 x 4 x 48 voxels: no ragged step) -- what the ragged step costs
    "cfg2_even": dict(win_size=10, pts_per_scan=100_000, n_voxels=49_152),
}


def rodrigues(ang: np.ndarray) -> np.ndarray:
    """Exp map, same 1e-11 cut-off as the reference (tools.hpp:51-66)."""
    ang = np.asarray(ang, dtype=np.float64)
    th = np.linalg.norm(ang)
    if th < 1e-11:
        return np.eye(3)
    k = ang / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pack_poses(Rs: np.ndarray, ps: np.ndarray) -> np.ndarray:
    W = Rs.shape[0]
    out = np.empty((W, 12))
    out[:, :9] = np.transpose(Rs, (0, 2, 1)).reshape(W, 9)  # column-major
    out[:, 9:] = ps
    return out


def unpack_poses(Rp: np.ndarray):
    Rp = np.asarray(Rp, dtype=np.float64).reshape(-1, 12)
    Rs = np.transpose(Rp[:, :9].reshape(-1, 3, 3), (0, 2, 1))
    return Rs.copy(), Rp[:, 9:].copy()


def clusters_from_points(xyz: np.ndarray, cell_ptr: np.ndarray) -> np.ndarray:
    """numpy restatement of PointCluster::push over bucketed points (independent of the oracle)."""
    n_cells = cell_ptr.shape[0] - 1
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    feats = np.stack([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z, np.ones_like(x)], axis=1)
    cs = np.zeros((xyz.shape[0] + 1, 10))
    np.cumsum(feats, axis=0, out=cs[1:])
    # cumulative sums lose a few ulps; fine for an input generator (the K1 parity tests use their own sums)
    return cs[cell_ptr[1:]] - cs[cell_ptr[:-1]] if n_cells else np.zeros((0, 10))


@dataclasses.dataclass
class Scene:
    win_size: int
    n_voxels: int
    points_body: np.ndarray   # (Npts, 3) f64, sorted by cell = frame * V + voxel
    cell_ptr: np.ndarray      # (W*V + 1,) int64
    clusters: np.ndarray      # (V, W, 10) f64 body-frame clusters (N = 0 -> unobserved)
    fix: np.ndarray           # (V, 10) world-frame fix clusters (N = 0 -> none)
    coe: np.ndarray           # (V,)
    poses_gt: np.ndarray      # (W, 12)
    poses_init: np.ndarray    # (W, 12) perturbed initial guess, frame 0 exact
    normals: np.ndarray       # (V, 3)

    @property
    def nnz(self) -> int:
        return int(np.count_nonzero(self.clusters[:, :, 9]))


def make_scene(win_size=5, pts_per_scan=20_000, n_voxels=5_000, p_obs=1.0, fix_frac=0.0, noise=0.02,
               rot_sigma_deg=0.05, trans_sigma=0.02, seed=MASTER_SEED, exact_clusters=True, pose_seed=None) -> Scene:
    """Build one window.  ``exact_clusters`` sums clusters per cell with np.add.reduceat
    (sequential per-cell order) instead of the cumulative-sum difference.  ``pose_seed`` draws the initial-guess
    perturbation from its own stream so voxel shards generated with different ``seed`` share one window."""
    rng = np.random.Generator(np.random.PCG64(seed))
    prng = np.random.Generator(np.random.PCG64([seed if pose_seed is None else pose_seed, 7919]))
    W, V = win_size, n_voxels

    # occupied cells in a slab around the trajectory (surfaces: ground/walls within a few metres of height)
    L = max(4, int(np.ceil(np.sqrt(V / (8 * 0.3)))))
    n_lattice = L * L * 8
    flat = rng.choice(n_lattice, size=V, replace=False)
    flat.sort()
    ix, iy, iz = flat // (L * 8), (flat // 8) % L, flat % 8
    centres = np.stack([ix - L / 2 + 0.5, iy - L / 2 + 0.5, iz - 2 + 0.5], axis=1).astype(np.float64)

    # normals: +-x / +-y / +-z families tilted by <= 10 degrees
    fam = rng.integers(0, 3, size=V)
    sign = rng.choice([-1.0, 1.0], size=V)
    base = np.zeros((V, 3))
    base[np.arange(V), fam] = sign
    tilt = np.deg2rad(10.0) * rng.uniform(0, 1, size=V)
    az = rng.uniform(0, 2 * np.pi, size=V)
    t1 = np.zeros((V, 3)); t1[np.arange(V), (fam + 1) % 3] = 1.0
    t2 = np.zeros((V, 3)); t2[np.arange(V), (fam + 2) % 3] = 1.0
    normals = np.cos(tilt)[:, None] * base + np.sin(tilt)[:, None] * (np.cos(az)[:, None] * t1 + np.sin(az)[:, None] * t2)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    b1 = np.cross(normals, t1); b1 /= np.linalg.norm(b1, axis=1, keepdims=True)
    b2 = np.cross(normals, b1)
    origin = centres + rng.uniform(-0.3, 0.3, size=V)[:, None] * normals

    # trajectory
    axis = np.array([0.2, 0.1, 1.0]); axis /= np.linalg.norm(axis)
    Rs = np.stack([rodrigues(0.02 * i * axis) for i in range(W)])
    ps = np.stack([np.array([0.5 * i, 0.1 * np.sin(i), 0.0]) for i in range(W)])
    Rs_init, ps_init = Rs.copy(), ps.copy()
    for i in range(1, W):
        Rs_init[i] = Rs[i] @ rodrigues(prng.normal(0, np.deg2rad(rot_sigma_deg), size=3))
        ps_init[i] = ps[i] + prng.normal(0, trans_sigma, size=3)

    # per-frame observation pattern and point counts: every observed cell gets >= 1 point, and every voxel is
    # seen from >= min(2, W) frames (the reference drops voxels with too few points / observers:
    # voxel_map.hpp:1155, loop_refine.hpp:371-376)
    if p_obs < 1.0:
        seen_mask = rng.uniform(size=(W, V)) < p_obs
        need = min(2, W)
        for a in np.nonzero(seen_mask.sum(axis=0) < need)[0]:
            missing = np.nonzero(~seen_mask[:, a])[0]
            seen_mask[rng.choice(missing, size=need - int(seen_mask[:, a].sum()), replace=False), a] = True
    else:
        seen_mask = np.ones((W, V), dtype=bool)
    counts = np.zeros((W, V), dtype=np.int64)
    for i in range(W):
        seen = np.nonzero(seen_mask[i])[0]
        if seen.size == 0:
            continue
        extra = max(0, pts_per_scan - seen.size)
        counts[i, seen] = 1 + rng.multinomial(extra, np.full(seen.size, 1.0 / seen.size))
    cell_ptr = np.zeros(W * V + 1, dtype=np.int64)
    np.cumsum(counts.reshape(-1), out=cell_ptr[1:])
    npts = int(cell_ptr[-1])
    cell_of_pt = np.repeat(np.arange(W * V, dtype=np.int64), counts.reshape(-1))
    vox_of_pt = cell_of_pt % V
    frm_of_pt = cell_of_pt // V

    s1 = rng.uniform(-0.45, 0.45, size=npts)
    s2 = rng.uniform(-0.45, 0.45, size=npts)
    nz = rng.normal(0, noise, size=npts)
    world = origin[vox_of_pt] + s1[:, None] * b1[vox_of_pt] + s2[:, None] * b2[vox_of_pt] + nz[:, None] * normals[vox_of_pt]
    # body frame x = R_gt^T (w - p_gt)
    d = world - ps[frm_of_pt]
    points_body = np.einsum("nji,nj->ni", Rs[frm_of_pt], d)
    points_body = np.ascontiguousarray(points_body)

    if exact_clusters and npts:
        x, y, z = points_body[:, 0], points_body[:, 1], points_body[:, 2]
        feats = np.stack([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z, np.ones_like(x)], axis=1)
        nonempty = counts.reshape(-1) > 0
        cl = np.zeros((W * V, 10))
        cl[nonempty] = np.add.reduceat(feats, cell_ptr[:-1][nonempty], axis=0)
    else:
        cl = clusters_from_points(points_body, cell_ptr)
    clusters = np.ascontiguousarray(cl.reshape(W, V, 10).transpose(1, 0, 2))

    # optional world-frame fix clusters (marginalised scans, voxel_map.hpp:1256-1268)
    fix = np.zeros((V, 10))
    if fix_frac > 0:
        has = np.nonzero(rng.uniform(size=V) < fix_frac)[0]
        nfix = rng.integers(20, 101, size=has.size)
        for a, k in zip(has, nfix):
            q1 = rng.uniform(-0.45, 0.45, size=k); q2 = rng.uniform(-0.45, 0.45, size=k); qn = rng.normal(0, noise, size=k)
            w = origin[a] + q1[:, None] * b1[a] + q2[:, None] * b2[a] + qn[:, None] * normals[a]
            fix[a] = [np.sum(w[:, 0] ** 2), np.sum(w[:, 0] * w[:, 1]), np.sum(w[:, 0] * w[:, 2]), np.sum(w[:, 1] ** 2),
                      np.sum(w[:, 1] * w[:, 2]), np.sum(w[:, 2] ** 2), w[:, 0].sum(), w[:, 1].sum(), w[:, 2].sum(), k]

    return Scene(win_size=W, n_voxels=V, points_body=points_body, cell_ptr=cell_ptr, clusters=clusters, fix=fix,
                 coe=np.ones(V), poses_gt=pack_poses(Rs, ps), poses_init=pack_poses(Rs_init, ps_init), normals=normals)


def make_config(name: str, **overrides) -> Scene:
    idx = list(CONFIGS).index(name) + 1
    kw = dict(CONFIGS[name]); kw.setdefault("seed", MASTER_SEED + idx); kw.update(overrides)
    return make_scene(**kw)


def pose_errors(Rp_a: np.ndarray, Rp_b: np.ndarray):
    """(translation RMSE [m], rotation RMSE [rad]) over the window between two packed pose sets."""
    Ra, pa = unpack_poses(Rp_a)
    Rb, pb = unpack_poses(Rp_b)
    dt = np.linalg.norm(pa - pb, axis=1)
    dr = []
    for A, B in zip(Ra, Rb):
        c = np.clip((np.trace(A.T @ B) - 1) / 2, -1, 1)
        # for tiny angles use the skew part (acos loses precision near 1)
        S = A.T @ B
        s = 0.5 * np.linalg.norm([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]])
        dr.append(np.arctan2(s, c))
    return float(np.sqrt(np.mean(dt ** 2))), float(np.sqrt(np.mean(np.square(dr))))


# ------------------------------------------------------------------------------------------------------------
# Inertial side of a window: a smooth trajectory through the scene's ground-truth poses, an IMU sample stream
# measured along it, and the 15-dimensional window states (R, p, v, bg, ba | g) the LiDAR-inertial BA optimises.
# ------------------------------------------------------------------------------------------------------------
GRAVITY = np.array([0.0, 0.0, -9.8])          # G_m_s2 of the reference (tools.hpp), world frame
STATE_LEN = 24


def so3_log(R: np.ndarray) -> np.ndarray:
    """Rotation vector of R (angle < pi); atan2 form, accurate for tiny angles too."""
    K = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.linalg.norm(K)
    th = np.arctan2(sn, 0.5 * (np.trace(R) - 1))
    return K if sn < 1e-12 else (th / sn) * K


def pack_states(Rs, ps, vs, bg, ba, g=GRAVITY) -> np.ndarray:
    W = len(Rs)
    out = np.zeros((W, STATE_LEN))
    for i in range(W):
        out[i, :9] = np.asarray(Rs[i]).T.reshape(9)
        out[i, 9:12] = ps[i]; out[i, 12:15] = vs[i]; out[i, 15:18] = bg; out[i, 18:21] = ba; out[i, 21:24] = g
    return out


@dataclasses.dataclass
class ImuWindow:
    states_gt: np.ndarray      # (W, 24)
    states_init: np.ndarray    # (W, 24): scene.poses_init + perturbed velocities + the bias estimate
    samples: list              # W-1 entries of (gyr (K,3), acc (K,3), dt (K,)): mid-point, bias-estimate-corrected samples
    noise_meas: np.ndarray     # (6,6)
    noise_walk: np.ndarray     # (6,6)
    dt_frame: float


def make_imu(scene: Scene, rate_hz=200.0, frame_dt=0.1, gyr_sigma=1e-3, acc_sigma=1e-2, bias_g=(0.002, -0.001, 0.0015),
             bias_a=(0.02, 0.01, -0.015), bias_est_err=0.3, vel_sigma=0.02, cov_gyr=0.01, cov_acc=1.0, rdw_gyr=1e-4, rdw_acc=1e-4,
             seed=MASTER_SEED + 77) -> ImuWindow:
    """IMU stream consistent with ``scene.poses_gt``: between frames the body turns with a constant body rate and moves
    with a constant world acceleration (so frame poses are hit exactly); the accelerometer reads R^T (a - g) + ba + noise,
    the gyro w + bg + noise.  The bias *estimate* used for preintegration is off by ``bias_est_err`` (relative), which is
    what the BA's bias states have to absorb.  Noise densities default to the reference's LocalBA settings
    (config/avia.yaml:39-42)."""
    rng = np.random.Generator(np.random.PCG64([seed, 4242]))
    W = scene.win_size
    Rs, ps = unpack_poses(scene.poses_gt)
    K = int(round(rate_hz * frame_dt))
    h = frame_dt / K
    bg_true = np.asarray(bias_g, dtype=np.float64); ba_true = np.asarray(bias_a, dtype=np.float64)
    bg_est = bg_true * (1 - bias_est_err); ba_est = ba_true * (1 - bias_est_err)
    # velocities at the frames: v_{i+1} = 2 (p_{i+1} - p_i) / T - v_i  (constant acceleration per interval)
    vs = np.zeros((W, 3))
    vs[0] = (ps[1] - ps[0]) / frame_dt if W > 1 else 0.0
    samples = []
    for i in range(W - 1):
        a_w = 2 * (ps[i + 1] - ps[i] - vs[i] * frame_dt) / frame_dt ** 2
        vs[i + 1] = vs[i] + a_w * frame_dt
        w_b = so3_log(Rs[i].T @ Rs[i + 1]) / frame_dt
        t = np.arange(K + 1) * h
        gyr_raw = np.zeros((K + 1, 3)); acc_raw = np.zeros((K + 1, 3))
        for k in range(K + 1):
            Rt = Rs[i] @ rodrigues(w_b * t[k])
            gyr_raw[k] = w_b + bg_true + rng.normal(0, gyr_sigma, 3)
            acc_raw[k] = Rt.T @ (a_w - GRAVITY) + ba_true + rng.normal(0, acc_sigma, 3)
        gyr = 0.5 * (gyr_raw[:-1] + gyr_raw[1:]) - bg_est        # push_imu: mid-point, minus the factor's bias (preintegration.hpp:58-69)
        acc = 0.5 * (acc_raw[:-1] + acc_raw[1:]) - ba_est
        samples.append((gyr, acc, np.full(K, h)))
    Ri, pi = unpack_poses(scene.poses_init)
    vi = vs + rng.normal(0, vel_sigma, size=vs.shape)
    vi[0] = vs[0]
    noise_meas = np.diag([cov_gyr] * 3 + [cov_acc] * 3).astype(np.float64)
    noise_walk = np.diag([rdw_gyr] * 3 + [rdw_acc] * 3).astype(np.float64)
    return ImuWindow(states_gt=pack_states(Rs, ps, vs, bg_true, ba_true), states_init=pack_states(Ri, pi, vi, bg_est, ba_est),
                     samples=samples, noise_meas=noise_meas, noise_walk=noise_walk, dt_frame=frame_dt)


# ------------------------------------------------------------------------------------------------------------
# Raw scans for the batch factor construction (voxel hash -> octree -> plane test): a few large planar walls / floors
# plus clutter, sampled by every frame, NOT aligned with the voxel grid -- so root voxels contain one plane, two planes
# (edges: subdivided), or clutter (rejected), like a real scene.
# ------------------------------------------------------------------------------------------------------------
def make_scans(win_size=5, pts_per_scan=20_000, extent=20.0, noise=0.01, clutter_frac=0.1, seed=MASTER_SEED + 555, rot_sigma_deg=0.0,
               trans_sigma=0.0):
    """Returns (xyz_local (N,3) frame-major, frame_ptr (W+1,), poses (W,12)).  Points are expressed in their frame's body
    coordinates with the returned poses (optionally perturbed away from the poses the scans were taken at)."""
    rng = np.random.Generator(np.random.PCG64([seed, 99]))
    W = win_size
    axis = np.array([0.2, 0.1, 1.0]); axis /= np.linalg.norm(axis)
    Rs = np.stack([rodrigues(0.03 * i * axis) for i in range(W)])
    ps = np.stack([np.array([0.4 * i, 0.1 * np.sin(i), 0.02 * i]) for i in range(W)])
    # planes: point + two in-plane unit vectors + size
    planes = []
    for k in range(8):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        if k < 3:
            n = np.eye(3)[k] + 0.05 * rng.normal(size=3); n /= np.linalg.norm(n)
        a = np.cross(n, [0.3, 0.5, 0.8]); a /= np.linalg.norm(a)
        b = np.cross(n, a)
        c = rng.uniform(-extent / 2, extent / 2, size=3)
        planes.append((c, a, b, n, rng.uniform(extent / 4, extent / 2)))
    clouds = []
    for i in range(W):
        n_cl = int(pts_per_scan * clutter_frac)
        n_pl = pts_per_scan - n_cl
        which = rng.integers(0, len(planes), size=n_pl)
        w = np.zeros((n_pl, 3))
        for k, (c, a, b, n, sz) in enumerate(planes):
            sel = np.nonzero(which == k)[0]
            # a fixed lattice of surface samples per plane, so every frame revisits the same surface patches
            u = rng.uniform(-sz, sz, size=sel.size); v = rng.uniform(-sz, sz, size=sel.size)
            w[sel] = c + u[:, None] * a + v[:, None] * b + rng.normal(0, noise, size=sel.size)[:, None] * n
        cl = rng.uniform(-extent / 2, extent / 2, size=(n_cl, 3))
        world = np.concatenate([w, cl])[rng.permutation(pts_per_scan)]
        clouds.append(np.einsum("ji,nj->ni", Rs[i], world - ps[i]))
    xyz = np.ascontiguousarray(np.concatenate(clouds))
    frame_ptr = np.arange(W + 1, dtype=np.int64) * pts_per_scan
    Rs2, ps2 = Rs.copy(), ps.copy()
    for i in range(1, W):
        if rot_sigma_deg > 0:
            Rs2[i] = Rs[i] @ rodrigues(rng.normal(0, np.deg2rad(rot_sigma_deg), size=3))
        if trans_sigma > 0:
            ps2[i] = ps[i] + rng.normal(0, trans_sigma, size=3)
    return xyz, frame_ptr, pack_poses(Rs2, ps2), pack_poses(Rs, ps)


# ------------------------------------------------------------------------------------------------------------
# Initialisation: raw scans taken DURING the motion + the raw IMU messages of their intervals + propagated states off the truth.
# ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class InitSession:
    win_size: int
    scans: list                # W entries of (xyz (n,3) float32 in the LiDAR frame, toff (n,) float32 seconds after beg_times[i], ascending)
    beg_times: np.ndarray      # (W,)
    imus: list                 # W entries of (stamps (K,), gyr (K,3), acc (K,3)): the raw messages of scan i's interval
    states_gt: np.ndarray      # (W, 24) at the END of every scan
    states_init: np.ndarray    # (W, 24): off the truth, gravity guess tilted
    covs: np.ndarray           # (W, 15, 15) of the propagated states
    ext: np.ndarray            # (12,) LiDAR -> IMU, [R column-major | p]
    noise_meas: np.ndarray
    noise_walk: np.ndarray
    imupre_scale_gravity: float
    planes: list               # (point, normal) of the scene's planes


def make_init_session(win_size=6, pts_per_scan=1500, extent=6.6, noise=0.003, clutter_frac=0.05, frame_dt=0.1, imu_per_scan=10, rot_err_deg=0.2, trans_err=0.02,
                      vel_err=0.02, gravity_tilt_deg=3.0, bias_g=(0.002, -0.001, 0.0015), bias_a=(0.02, 0.01, -0.015), bias_est_err=0.3, scale_gravity=1.0,
                      gravity_norm=9.8, scene="room", cov_gyr=0.01, cov_acc=1.0, rdw_gyr=1e-4, rdw_acc=1e-4, seed=MASTER_SEED + 1500) -> InitSession:
    """A session for ``Initialization::motion_init``.  The trajectory has a constant body rate and a constant world acceleration per scan interval (as
    ``make_imu``), so mid-point integration of the noise-free messages reproduces it to O(h^2).  Every point is sampled at the pose of ITS OWN time offset
    and expressed in the LiDAR frame through a non-trivial extrinsic.  ``scene``: "room" = six slightly tilted walls off the voxel grid plus clutter;
    "parallel" = only floor and ceiling (a degenerate scatter of normals); "sparse" = clutter only (no plane voxels).  Initial states are off the truth by
    ``rot_err_deg`` / ``trans_err`` / ``vel_err`` (state 0 keeps its pose), the bias estimate by ``bias_est_err`` (relative), and the gravity guess is the
    true one tilted by ``gravity_tilt_deg``; ``gravity_norm`` is the magnitude the IMU actually senses."""
    rng = np.random.Generator(np.random.PCG64([seed, 1501]))
    W = win_size
    g_true = np.array([0.0, 0.0, -float(gravity_norm)])
    bg = np.asarray(bias_g, dtype=np.float64); ba = np.asarray(bias_a, dtype=np.float64)
    eR = rodrigues(np.array([0.02, -0.03, 0.5])); ep = np.array([0.1, 0.05, -0.02])
    # the scene
    h = extent / 2
    planes = []
    faces = [(np.array([0, 0, 1.0]), -h + 0.37), (np.array([0, 0, -1.0]), -h + 0.41)]
    if scene == "room":
        faces += [(np.array([1.0, 0, 0]), -h + 0.33), (np.array([-1.0, 0, 0]), -h + 0.29), (np.array([0, 1.0, 0]), -h + 0.43), (np.array([0, -1.0, 0]), -h + 0.35)]
    for k, (n0, off) in enumerate(faces if scene != "sparse" else []):
        n = n0 + (0.0 if scene == "parallel" else 0.03) * rng.normal(size=3); n /= np.linalg.norm(n)
        a = np.cross(n, [0.3, 0.5, 0.8]); a /= np.linalg.norm(a)
        planes.append((n0 * off, n, a, np.cross(n, a)))
    # the trajectory: state -1 (begin of scan 0) .. state W-1
    R = rodrigues(np.array([0.05, -0.02, 0.1])); p = np.array([0.2, -0.1, 0.05]); v = np.array([0.5, 0.2, -0.05])
    t0 = 100.0
    scans, imus, beg, Rs, ps, vs = [], [], [], [], [], []
    for i in range(W):
        w_b = np.array([0.25, -0.2, 0.35]) + 0.1 * rng.normal(size=3)
        a_w = np.array([0.6, -0.4, 0.2]) + 0.3 * rng.normal(size=3)

        def pose(t, R=R, p=p, v=v, w_b=w_b, a_w=a_w):
            return R @ rodrigues(w_b * t), p + v * t + 0.5 * a_w * t * t
        K = imu_per_scan + 1
        ts = np.linspace(0.0, frame_dt, K)
        gyr = np.tile(w_b + bg, (K, 1))
        acc = np.stack([(pose(t)[0].T @ (a_w - g_true) + ba) / scale_gravity for t in ts])     # upstream: acc_avr * scale - ba
        imus.append((t0 + i * frame_dt + ts, gyr, acc))
        beg.append(t0 + i * frame_dt)
        n_cl = int(pts_per_scan * clutter_frac) if planes else pts_per_scan
        n_pl = pts_per_scan - n_cl
        world = [rng.uniform(-h, h, size=(n_cl, 3))]
        if planes:
            which = rng.integers(0, len(planes), size=n_pl)
            for k, (c, n, a, b) in enumerate(planes):
                m = int((which == k).sum())
                world.append(c + rng.uniform(-h, h, m)[:, None] * a + rng.uniform(-h, h, m)[:, None] * b + rng.normal(0, noise, m)[:, None] * n)
        world = np.concatenate(world)[rng.permutation(pts_per_scan)]
        toff = np.sort(rng.uniform(0.02 * frame_dt, frame_dt, pts_per_scan)).astype(np.float32)
        xyz = np.zeros((pts_per_scan, 3))
        for q in range(pts_per_scan):
            Rt, pt = pose(float(toff[q]))
            xyz[q] = eR.T @ (Rt.T @ (world[q] - pt) - ep)
        scans.append((xyz.astype(np.float32), toff))
        R, p, v = pose(frame_dt)[0], pose(frame_dt)[1], v + a_w * frame_dt
        Rs.append(R); ps.append(p); vs.append(v)
    states_gt = pack_states(Rs, ps, vs, bg, ba, g_true)
    Ri = [Rs[0]] + [Rs[i] @ rodrigues(rng.normal(0, np.deg2rad(rot_err_deg), 3)) for i in range(1, W)]
    pi = [ps[0]] + [ps[i] + rng.normal(0, trans_err, 3) for i in range(1, W)]
    vi = [vs[i] + rng.normal(0, vel_err, 3) for i in range(W)]
    tilt = rodrigues(np.deg2rad(gravity_tilt_deg) * np.array([0.6, -0.8, 0.0]))
    states_init = pack_states(Ri, pi, vi, bg * (1 - bias_est_err), ba * (1 - bias_est_err), tilt @ np.array([0.0, 0.0, -9.8]))
    covs = np.tile(np.diag([1e-5] * 3 + [1e-4] * 3 + [1e-3] * 3 + [1e-6] * 6), (W, 1, 1))
    return InitSession(win_size=W, scans=scans, beg_times=np.array(beg), imus=imus, states_gt=states_gt, states_init=states_init, covs=covs,
                       ext=np.concatenate([eR.T.reshape(9), ep]), noise_meas=np.diag([cov_gyr] * 3 + [cov_acc] * 3).astype(np.float64),
                       noise_walk=np.diag([rdw_gyr] * 3 + [rdw_acc] * 3).astype(np.float64), imupre_scale_gravity=float(scale_gravity),
                       planes=[(c, n) for c, n, _, _ in planes])


# ------------------------------------------------------------------------------------------------------------
# Odometry: a voxel plane map as the reference's `surf_map` would hold it after some scans -- root voxels that
# are one plane, or are subdivided once / twice with planes, plane-less leaves and missing children below -- flattened to its
# leaves, and one scan that sees those planes from a pose near the true one.
# ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PlaneMapData:
    voxel_size: float
    max_layer: int
    loc: np.ndarray        # (n,3) int64  root voxel
    layer: np.ndarray      # (n,)  int32
    path: np.ndarray       # (n,)  int32  leafnum per level, 3 bits each, first level lowest
    is_plane: np.ndarray   # (n,)  int32
    center: np.ndarray     # (n,3)
    normal: np.ndarray     # (n,3)
    plane_var: np.ndarray  # (n,6,6)
    radius: np.ndarray     # (n,)  float32-representable
    box_center: np.ndarray  # (n,3) centre of the leaf's cell
    box_half: np.ndarray   # (n,)

    def args(self):
        return self.loc, self.layer, self.path, self.center, self.normal, self.plane_var, self.radius, self.is_plane


def make_plane_map(n_roots=2000, extent=12, voxel_size=1.0, max_layer=2, seed=MASTER_SEED + 900) -> PlaneMapData:
    rng = np.random.Generator(np.random.PCG64([seed, 31]))
    side = 2 * extent
    flat = rng.choice(side ** 3, size=n_roots, replace=False)
    roots = np.stack([flat // (side * side), (flat // side) % side, flat % side], axis=1).astype(np.int64) - extent
    rows = []

    def leaf(loc, layer, path, c_box, half, plane):
        if plane:
            fam = np.eye(3)[rng.integers(0, 3)] * rng.choice([-1.0, 1.0])
            n = fam + 0.15 * rng.normal(size=3); n /= np.linalg.norm(n)
            c = c_box + rng.uniform(-0.3, 0.3, size=3) * half
            B = rng.normal(size=(6, 6)) * 3e-3
            rows.append((loc, layer, path, 1, c, n, B @ B.T, np.float32((2 * half) ** 2 / 12 * rng.uniform(0.6, 1.2)), c_box, half))
        else:
            rows.append((loc, layer, path, 0, c_box, np.array([0.0, 0.0, 1.0]), np.zeros((6, 6)), np.float32(0.0), c_box, half))

    def grow(loc, layer, path, c_box, half):
        # a node at `layer`: leaf (plane or not) or subdivided
        p_split = 0.0 if layer >= max_layer else (0.4 if layer == 0 else 0.3)
        if rng.random() < p_split:
            for leafnum in range(8):
                if rng.random() < 0.65:
                    sgn = np.array([(leafnum >> 2) & 1, (leafnum >> 1) & 1, leafnum & 1]) * 2 - 1
                    grow(loc, layer + 1, path | (leafnum << (3 * layer)), c_box + sgn * half / 2, half / 2)
        else:
            leaf(loc, layer, path, c_box, half, rng.random() < 0.9)

    for loc in roots:
        grow(loc, 0, 0, (loc + 0.5) * voxel_size, voxel_size / 2)
    cols = list(zip(*rows))
    return PlaneMapData(voxel_size, max_layer, np.array(cols[0], dtype=np.int64), np.array(cols[1], dtype=np.int32), np.array(cols[2], dtype=np.int32),
                        np.array(cols[3], dtype=np.int32), np.array(cols[4]), np.array(cols[5]), np.array(cols[6]), np.array(cols[7], dtype=np.float64),
                        np.array(cols[8]), np.array(cols[9]))


@dataclasses.dataclass
class LioScan:
    xyz: np.ndarray        # (n,3) float32, sensor (= IMU) frame
    state_gt: np.ndarray   # VXBA state vector of the pose the scan was taken at
    state_init: np.ndarray  # the propagated guess lio_state_estimation starts from
    cov: np.ndarray        # 15x15


def make_lio_scan(pm: PlaneMapData, n_points=20_000, noise=0.02, clutter_frac=0.05, rot_sigma_deg=0.3, trans_sigma=0.03, seed=MASTER_SEED + 901,
                  coherent=False, planes_hit=None) -> LioScan:
    """coherent: points ordered along the voxel grid (a spinning LiDAR's neighbouring returns fall on neighbouring surfaces) instead of
    shuffled; planes_hit: restrict the scan to that many of the map's planes (a real scan sees a small part of the map, many points each)."""
    rng = np.random.Generator(np.random.PCG64([seed, 32]))
    R_gt = rodrigues(np.array([0.02, -0.03, 0.4])); p_gt = np.array([0.3, -0.2, 0.1])
    planes = np.nonzero(pm.is_plane == 1)[0]
    if planes_hit is not None and planes_hit < planes.size:
        planes = planes[rng.choice(planes.size, size=planes_hit, replace=False)]
    n_cl = int(n_points * clutter_frac); n_pl = n_points - n_cl
    k = planes[rng.integers(0, planes.size, size=n_pl)]
    n = pm.normal[k]
    a = np.cross(n, np.array([0.31, 0.52, 0.79])); a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(n, a)
    h = pm.box_half[k][:, None]
    w = pm.center[k] + rng.uniform(-1, 1, size=(n_pl, 1)) * h * a + rng.uniform(-1, 1, size=(n_pl, 1)) * h * b + rng.normal(0, noise, size=(n_pl, 1)) * n
    lo = pm.loc.min(axis=0) * pm.voxel_size; hi = (pm.loc.max(axis=0) + 1) * pm.voxel_size
    cl = rng.uniform(lo, hi, size=(n_cl, 3))
    world = np.concatenate([w, cl])[rng.permutation(n_points)]
    if coherent:
        cell = np.floor(world / pm.voxel_size).astype(np.int64)
        world = world[np.lexsort((cell[:, 2], cell[:, 1], cell[:, 0]))]
    xyz = np.ascontiguousarray(((world - p_gt) @ R_gt).astype(np.float32))
    R0 = R_gt @ rodrigues(rng.normal(0, np.deg2rad(rot_sigma_deg), size=3)); p0 = p_gt + rng.normal(0, trans_sigma, size=3)
    v = np.array([0.5, 0.1, 0.0]); g = np.array([0.0, 0.0, -9.8])
    st = lambda R, p: np.concatenate([R.T.reshape(9), p, v, np.zeros(3), np.zeros(3), g])
    cov = np.eye(15) * 1e-4
    cov[9:, 9:] = np.eye(6) * 1e-5
    M = rng.normal(size=(15, 15)) * 1e-3       # a propagated covariance is not diagonal
    cov = cov + 0.02 * (M @ M.T)
    return LioScan(xyz, st(R_gt, p_gt), st(R0, p0), cov)


# ------------------------------------------------------------------------------------------------------------
# Raw scan + raw IMU in front of the odometry (vxba_imuekf_*, front.OdometryFront): one scan interval of a motion that is EXACTLY the
# model IMUEKF::motion_blur integrates -- between two IMU stamps a constant body rate and a constant world acceleration R_k s_k + g with
# the rotation at the step's start -- so that the filter's propagation and de-skew reproduce it to rounding.
# ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class RawOdometryStep:
    scan: tuple            # (xyz (n,3) float32 in the LiDAR frame AS MEASURED, each point at its own time; toff (n,) float32 seconds after beg_time, ascending)
    imus: tuple            # (stamps (K,), gyr (K,3), acc (K,3)): the raw messages of the interval
    beg_time: float
    end_time: float
    state_prev: np.ndarray  # (24,) what the filter starts from: the truth at the previous scan end plus a pose error
    cov: np.ndarray        # (15,15)
    truth_prev: np.ndarray  # (24,)
    truth_end: np.ndarray  # (24,) at end_time
    last_imu: tuple        # (stamp, gyr, acc) of the interval's last message: the next step's `last_imu`
    scan_end: np.ndarray   # (n,3) float64: the points in the LiDAR frame at end_time -- what a perfect de-skew returns
    ext: np.ndarray        # (12,)


def make_raw_motion(truth_prev, last_imu, last_end, K, span, scale_gravity=1.0, end_after=0.3, rate=(0.25, -0.2, 0.35), accel=(0.6, -0.4, 0.2), jitter=0.1, seed=MASTER_SEED + 950):
    """K messages at last_end + span k / K and a scan end `end_after` steps behind the last one; per step a body rate and a world acceleration drawn around
    `rate` / `accel`.  The messages are chosen so that the mid-point samples the filter forms (last_imu in front) are those values exactly.
    Returns (imus, end_time, pose(t) -> (R, p, v) for last_end <= t <= end_time, truth_end (24))."""
    rng = np.random.Generator(np.random.PCG64([seed, 33]))
    x = np.asarray(truth_prev, dtype=np.float64)
    R, p, v, bg, ba, g = x[:9].reshape(3, 3).T.copy(), x[9:12].copy(), x[12:15].copy(), x[15:18], x[18:21], x[21:24]
    step = span / K
    stamps = last_end + step * np.arange(1, K + 1)
    end_time = float(stamps[-1] + end_after * step)
    nodes = np.concatenate([[last_end], stamps])
    gyr, acc, seg = np.zeros((K, 3)), np.zeros((K, 3)), []
    g_prev, a_prev = np.asarray(last_imu[1], dtype=np.float64), np.asarray(last_imu[2], dtype=np.float64)
    for k in range(K):
        w = np.asarray(rate) + jitter * rng.normal(size=3)
        a_w = np.asarray(accel) + 3 * jitter * rng.normal(size=3)
        s = R.T @ (a_w - g)                                        # the specific force in the body frame at the step's start
        gyr[k] = 2.0 * (w + bg) - g_prev
        acc[k] = 2.0 * (s + ba) / scale_gravity - a_prev
        g_prev, a_prev = gyr[k], acc[k]
        seg.append((nodes[k], R.copy(), p.copy(), v.copy(), w, a_w))
        dt = nodes[k + 1] - nodes[k]
        p = p + v * dt + 0.5 * a_w * dt * dt
        v = v + a_w * dt
        R = R @ rodrigues(w * dt)
    seg.append((nodes[K], R.copy(), p.copy(), v.copy(), seg[-1][4], seg[-1][5]))      # the tail keeps the last step's rate and acceleration

    def pose(t):
        k = min(max(int(np.searchsorted(nodes, t, side="right")) - 1, 0), K)
        t0, Rk, pk, vk, w, a_w = seg[k]
        d = t - t0
        return Rk @ rodrigues(w * d), pk + vk * d + 0.5 * a_w * d * d, vk + a_w * d

    Re, pe, ve = pose(end_time)
    truth_end = np.concatenate([Re.T.reshape(9), pe, ve, bg, ba, g])
    return (stamps, gyr, acc), end_time, pose, truth_end


def make_raw_odometry_step(pm: PlaneMapData, last_imu, last_end, g, scale_gravity=1.0, truth_prev=None, n_points=3000, K=20, span=0.1, end_after=0.3, ext=None,
                           noise=0.02, clutter_frac=0.05, rot_sigma_deg=0.3, trans_sigma=0.03, bias_g=(0.002, -0.001, 0.0015), bias_a=(0.02, 0.01, -0.015),
                           seed=MASTER_SEED + 951) -> RawOdometryStep:
    """One raw odometry step on top of make_plane_map / make_lio_scan: the scan's world points are make_lio_scan's; the sensor moves by make_raw_motion over
    the interval and sees every point at the pose of the point's own time (the inverse of the de-skew, in f64, stored as float32).  last_imu / last_end / g /
    scale_gravity: the filter's history (its last message, last scan end, gravity and accelerometer scale).  truth_prev: the true state at last_end
    (None: make_lio_scan's pose); the filter is handed that state off by rot_sigma_deg / trans_sigma."""
    rng = np.random.Generator(np.random.PCG64([seed, 34]))
    ls = make_lio_scan(pm, n_points=n_points, noise=noise, clutter_frac=clutter_frac, seed=seed + 1)
    R0, p0 = ls.state_gt[:9].reshape(3, 3).T, ls.state_gt[9:12]
    world = ls.xyz.astype(np.float64) @ R0.T + p0
    if truth_prev is None:
        truth_prev = np.concatenate([ls.state_gt[:15], np.asarray(bias_g, dtype=np.float64), np.asarray(bias_a, dtype=np.float64), np.asarray(g, dtype=np.float64)])
    truth_prev = np.asarray(truth_prev, dtype=np.float64).copy()
    ext = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]) if ext is None else np.asarray(ext, dtype=np.float64).reshape(12)
    L, l = ext[:9].reshape(3, 3).T, ext[9:12]
    imus, end_time, pose, truth_end = make_raw_motion(truth_prev, last_imu, last_end, K, span, scale_gravity, end_after, seed=seed + 2)
    toff = np.sort(rng.uniform(1e-4, end_time - last_end, n_points)).astype(np.float32)
    Re, pe, _ = pose(end_time)
    scan_end = ((world - pe) @ Re - l) @ L                                   # L^T (R_e^T (w - p_e) - l)
    xyz = np.zeros((n_points, 3))
    for q in range(n_points):
        Rt, pt, _ = pose(last_end + float(toff[q]))
        xyz[q] = L.T @ (Rt.T @ (world[q] - pt) - l)
    Rp = truth_prev[:9].reshape(3, 3).T @ rodrigues(rng.normal(0, np.deg2rad(rot_sigma_deg), size=3))
    state_prev = truth_prev.copy()
    state_prev[:9] = Rp.T.reshape(9); state_prev[9:12] += rng.normal(0, trans_sigma, size=3)
    return RawOdometryStep((xyz.astype(np.float32), toff), imus, float(last_end), end_time, state_prev, ls.cov.copy(), truth_prev, truth_end,
                           (float(imus[0][-1]), imus[1][-1].copy(), imus[2][-1].copy()), scan_end, ext)


# ------------------------------------------------------------------------------------------------------------
# Loop-edge registration (vxba_loopreg_*, hba.loop_registration): two keyframes of one scene, each a few consecutive
# make_scans scans merged in the frame of its first scan, far enough apart that their views differ.
# ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LoopPair:
    cloud_tar: np.ndarray     # (n, 3) the earlier keyframe (the loop's target), in its own frame
    cloud_cur: np.ndarray     # (n, 3) the current keyframe (the source), in its own frame
    pose_tar: np.ndarray      # (12,) world pose of the target keyframe
    pose_cur: np.ndarray      # (12,) world pose of the current keyframe
    pose_true: np.ndarray     # (12,) current-frame -> target-frame: the measurement a perfect registration returns
    pose_guess: np.ndarray    # (12,) pose_true perturbed: R_true Exp(guess_rot), t_true + guess_tr


def merge_keyframe(xyz, fp, poses, ids):
    """Scans ``ids`` in the frame of scan ids[0]."""
    R, p = unpack_poses(poses)
    R0, p0 = R[ids[0]], p[ids[0]]
    out = []
    for k in ids:
        w = xyz[fp[k]:fp[k + 1]] @ R[k].T + p[k]
        out.append((w - p0) @ R0)
    return np.ascontiguousarray(np.concatenate(out))


def relative_pose(pose_tar, pose_cur):
    """The pose record that maps the current keyframe's coordinates into the target's: (R_t^T R_c, R_t^T (p_c - p_t))."""
    R, p = unpack_poses(np.stack([pose_tar, pose_cur]))
    return pack_poses((R[0].T @ R[1])[None], (R[0].T @ (p[1] - p[0]))[None])[0]


def loop_pair(win_size=12, pts_per_scan=60_000, extent=20.0, noise=0.01, seed=MASTER_SEED + 555, tar_ids=(0, 1, 2, 3), cur_ids=(8, 9, 10, 11),
              guess_rot_deg=(1.5, -1.0, 2.0), guess_tr=(0.25, -0.2, 0.15)) -> LoopPair:
    xyz, fp, _, gt = make_scans(win_size=win_size, pts_per_scan=pts_per_scan, extent=extent, noise=noise, seed=seed)
    cloud_tar, cloud_cur = merge_keyframe(xyz, fp, gt, list(tar_ids)), merge_keyframe(xyz, fp, gt, list(cur_ids))
    pose_tar, pose_cur = gt[tar_ids[0]].copy(), gt[cur_ids[0]].copy()
    true = relative_pose(pose_tar, pose_cur)
    R, t = unpack_poses(true[None])
    guess = pack_poses((R[0] @ rodrigues(np.deg2rad(np.asarray(guess_rot_deg, dtype=np.float64))))[None], (t[0] + np.asarray(guess_tr, dtype=np.float64))[None])[0]
    return LoopPair(cloud_tar, cloud_cur, pose_tar, pose_cur, true, guess)


def drifted_odometry(gt, rot_bias=(2e-4, -1e-4, 6e-4), tr_bias=(4e-3, 3e-3, -1e-3)):
    """Dead reckoning with a constant bias per step: pose k = pose k-1 o (true relative pose o (Exp(rot_bias), tr_bias)); pose 0 is the truth.  What
    a session looks like before a loop closure: locally right, the end off by the accumulated drift."""
    R, p = unpack_poses(gt)
    dR = rodrigues(np.asarray(rot_bias, dtype=np.float64)); dp = np.asarray(tr_bias, dtype=np.float64)
    Ro, po = [R[0]], [p[0]]
    for k in range(1, R.shape[0]):
        Rrel = R[k - 1].T @ R[k]; prel = R[k - 1].T @ (p[k] - p[k - 1])
        po.append(Ro[-1] @ (prel + dp) + po[-1])
        Ro.append(Ro[-1] @ Rrel @ dR)
    return pack_poses(np.stack(Ro), np.stack(po))


# BASELINE configs[4]: a long session for the hierarchical global BA (scripts/run_cfg5.py, bench.py --config cfg5)
def corridor_session(K, pts, seed):
    """A long hall (floor, ceiling, two side walls, all slightly tilted against the voxel grid) with partial cross walls every 10 m,
    seen by a sensor moving along it with a 30 m range: every keyframe samples only the surfaces around it."""
    rng = np.random.Generator(np.random.PCG64([seed, 7]))
    axis = np.array([0.2, 0.1, 1.0]); axis /= np.linalg.norm(axis)
    Rs = np.stack([rodrigues(0.004 * i * axis) for i in range(K)])
    ps = np.stack([np.array([0.4 * i, 0.6 * np.sin(0.05 * i), 0.1 * np.sin(0.03 * i)]) for i in range(K)])
    tilt = rodrigues(np.array([0.013, -0.021, 0.017]))
    clouds = []
    for i in range(K):
        x0 = ps[i, 0]
        n_each = pts // 5
        u = rng.uniform(x0 - 30, x0 + 30, size=(5, n_each)); v = rng.uniform(0, 1, size=(5, n_each))
        floor = np.stack([u[0], -8 + 16 * v[0], np.full(n_each, -2.0)], 1)
        ceil_ = np.stack([u[1], -8 + 16 * v[1], np.full(n_each, 4.0)], 1)
        wall1 = np.stack([u[2], np.full(n_each, -8.0), -2 + 6 * v[2]], 1)
        wall2 = np.stack([u[3], np.full(n_each, 8.0), -2 + 6 * v[3]], 1)
        kx = np.round(u[4] / 10.0) * 10.0                                   # cross walls at x = 10 k, alternating sides, 4 m wide
        side = np.where((kx / 10.0) % 2 == 0, 1.0, -1.0)
        cross = np.stack([kx, side * (4 + 4 * v[4]), -2 + 6 * rng.uniform(0, 1, n_each)], 1)
        w = np.concatenate([floor, ceil_, wall1, wall2, cross]) @ tilt.T
        w += rng.normal(0, 0.01, size=w.shape)
        clouds.append(((w - ps[i]) @ Rs[i]).astype(np.float32))
    gt = pack_poses(Rs, ps)
    Ri, pi = Rs.copy(), ps.copy()
    for i in range(1, K):
        Ri[i] = Rs[i] @ rodrigues(rng.normal(0, np.deg2rad(0.05), size=3)); pi[i] = ps[i] + rng.normal(0, 0.02, size=3)
    return clouds, pack_poses(Ri, pi), gt


# ------------------------------------------------------------------------------------------------------------
# Pose graphs (vxba_pgo_*, vxba.PoseGraph): a drifting odometry chain around a loop, closed either by a few loop
# edges (the graph build_graph makes after a loop closure) or by the edges of a hierarchical-BA pass (topDownProcess).
# Edge records are vxba_hba_pass's: (n, 2) int32 indices and (n, 18) [R_i^T R_j row-major | R_i^T (p_j - p_i) | v6].
# ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PoseGraphData:
    gt: np.ndarray            # (K, 12) ground truth
    poses: np.ndarray         # (K, 12) dead-reckoned odometry: the initial guess
    edge_ij: np.ndarray       # (E, 2) int32
    edge_data: np.ndarray     # (E, 18)
    prior_node: np.ndarray    # (P,) int32
    prior_pose: np.ndarray    # (P, 12)
    prior_v6: np.ndarray      # (P, 6)
    n_chain: int              # the first n_chain edges are the odometry chain


def _edge_record(Ri, pi, Rj, pj, v6, noise_R=None, noise_p=None):
    Z = Ri.T @ Rj
    if noise_R is not None:
        Z = Z @ noise_R
    z = Ri.T @ (pj - pi)
    if noise_p is not None:
        z = z + noise_p
    return np.concatenate([Z.reshape(9), z, v6])


def pose_graph(K, loops=(), hba=False, wdsize=10, mgsize=5, drift_rot=2e-3, drift_tr=2e-2, seed=MASTER_SEED + 7000) -> PoseGraphData:
    """K keyframes around 98 % of a 30 m circle; odometry with ``drift_rot`` rad / ``drift_tr`` m of noise per step, dead-reckoned from the true
    first pose; chain variances (1e-6 rad^2, 1e-4 m^2) x U(0.3, 3) per entry; ``loops``: (i, j) pairs measured exactly at the chain's nominal
    variances; ``hba``: every keyframe pair inside each ``wdsize`` window at stride ``mgsize`` and every pair of window anchors, measured to
    1e-4 rad / 1e-3 m with variances spread over four decades (what edges_from_hessian produces); one prior on keyframe 0 at 1e-9."""
    rng = np.random.default_rng(seed)
    R, p = [], []
    for k in range(K):
        a = 2 * np.pi * k / max(K - 1, 1) * 0.98
        R.append(rodrigues(np.array([0.02 * np.sin(3 * a), 0.03 * np.cos(2 * a), a])))
        p.append(np.array([30 * np.cos(a), 30 * np.sin(a), 0.5 * np.sin(4 * a)]))
    XR, Xp = [R[0]], [p[0]]
    for k in range(1, K):
        dR = R[k - 1].T @ R[k] @ rodrigues(rng.normal(size=3) * drift_rot)
        dp = R[k - 1].T @ (p[k] - p[k - 1]) + rng.normal(size=3) * drift_tr
        XR.append(XR[-1] @ dR); Xp.append(Xp[-1] + XR[-2] @ dp)
    v_ch = np.array([1e-6] * 3 + [1e-4] * 3)
    ij, data = [], []
    for k in range(1, K):
        ij.append((k - 1, k)); data.append(_edge_record(XR[k - 1], Xp[k - 1], XR[k], Xp[k], v_ch * rng.uniform(0.3, 3, 6)))
    for i, j in loops:
        ij.append((i, j)); data.append(_edge_record(R[i], p[i], R[j], p[j], v_ch))
    if hba:
        S = (K - wdsize) // mgsize + 1
        for w in range(S):
            for a in range(w * mgsize, w * mgsize + wdsize):
                for b in range(a + 1, w * mgsize + wdsize):
                    v6 = 1.0 / 10 ** rng.uniform(2, 6, 6)
                    ij.append((a, b)); data.append(_edge_record(R[a], p[a], R[b], p[b], v6, rodrigues(rng.normal(size=3) * 1e-4), rng.normal(size=3) * 1e-3))
        anchors = [w * mgsize for w in range(S)]
        for x in range(S):
            for y in range(x + 1, S):
                a, b = anchors[x], anchors[y]
                v6 = 1.0 / 10 ** rng.uniform(1, 5, 6)
                ij.append((a, b)); data.append(_edge_record(R[a], p[a], R[b], p[b], v6, rodrigues(rng.normal(size=3) * 1e-4), rng.normal(size=3) * 1e-3))
    gt = pack_poses(np.array(R), np.array(p))
    return PoseGraphData(gt=gt, poses=pack_poses(np.array(XR), np.array(Xp)), edge_ij=np.asarray(ij, dtype=np.int32).reshape(-1, 2), edge_data=np.asarray(data).reshape(-1, 18),
                         prior_node=np.zeros(1, dtype=np.int32), prior_pose=gt[:1].copy(), prior_v6=np.full((1, 6), 1e-9), n_chain=K - 1)


def random_pose_graph(K=20, extra_edges=30, seed=MASTER_SEED + 7100, noise_rot=5e-3, noise_tr=5e-2, init_rot=0.05, init_tr=0.3, sigma_rot=5e-3, sigma_tr=5e-2) -> PoseGraphData:
    """A connected graph over K random poses: a spanning chain in a random node order (both orientations, i > j included) plus ``extra_edges``
    random pairs, measurements with ``noise_rot`` rad / ``noise_tr`` m of noise (0: consistent measurements) under variances sigma^2 x U(0.3, 3), a
    prior on a random node, an initial guess ``init_rot`` rad / ``init_tr`` m off."""
    rng = np.random.default_rng(seed)
    R = np.array([rodrigues(rng.normal(size=3) * 0.8) for _ in range(K)])
    p = rng.normal(size=(K, 3)) * 5
    order = rng.permutation(K)
    pairs = [(int(order[k - 1]), int(order[k])) for k in range(1, K)]
    while len(pairs) < K - 1 + extra_edges:
        a, b = rng.integers(0, K, 2)
        if a != b:
            pairs.append((int(a), int(b)))
    data = []
    for a, b in pairs:
        v6 = np.concatenate([sigma_rot ** 2 * rng.uniform(0.3, 3, 3), sigma_tr ** 2 * rng.uniform(0.3, 3, 3)])
        data.append(_edge_record(R[a], p[a], R[b], p[b], v6, rodrigues(rng.normal(size=3) * noise_rot), rng.normal(size=3) * noise_tr))
    gt = pack_poses(R, p)
    Ri = np.array([R[k] @ rodrigues(rng.normal(size=3) * init_rot) for k in range(K)])
    node = int(rng.integers(0, K))
    return PoseGraphData(gt=gt, poses=pack_poses(Ri, p + rng.normal(size=(K, 3)) * init_tr), edge_ij=np.asarray(pairs, dtype=np.int32), edge_data=np.asarray(data),
                         prior_node=np.array([node], dtype=np.int32), prior_pose=gt[node:node + 1].copy(), prior_v6=np.full((1, 6), 1e-6), n_chain=K - 1)


# ScanPose hand-over of local mapping (voxelslam.cpp:1898-1911): what vxba.KeyframeBuilder takes, scan by scan
@dataclasses.dataclass
class ScanPoseStream:
    win_size: int
    poses: np.ndarray          # (n_scans, 12) world poses
    v6: np.ndarray             # (n_scans, 6) pose variances
    points: list               # per scan (n_i, 3) float64, body frame
    variances: list            # per scan (n_i, 9) float64, column-major 3 x 3 per point
    stationary: tuple          # (first scan, count) of the stretch that shares one pose; (0, 0) if the stream is too short for one
    empty: int                 # index of the scan without points; -1 if none

    def __len__(self):
        return self.poses.shape[0]

    def __iter__(self):
        for k in range(len(self)):
            yield self.poses[k], self.v6[k], self.points[k], self.variances[k]


def make_scanpose_stream(n_scans, pts_per_scan, win_size, room=(3.0, 3.0, 2.0), step=0.06, yaw_step_deg=0.8, noise=0.005, stationary=True, empty_scan=1,
                         seed=MASTER_SEED + 8100) -> ScanPoseStream:
    """A sensor creeping through a box-shaped room centred on the origin (so coordinates of both signs occur): ``step`` metres and ``yaw_step_deg``
    per scan -- a keyframe every ``win_size`` scans under the reference's 0.1 m rule -- except for a stationary stretch of ``win_size + 2`` scans
    from scan ``win_size + 1`` on (longer than a window: the drop rule runs) and one scan without points (``empty_scan``; < 0 or beyond the stream:
    none).  Deterministic in its arguments."""
    rng = np.random.default_rng(seed)
    first, count = (win_size + 1, win_size + 2) if stationary and 2 * win_size + 3 <= n_scans else (0, 0)
    Rs, ps = [], []
    R, p = rodrigues(np.array([0.01, -0.02, 0.3])), np.array([-0.4, 0.3, 0.1])
    for k in range(n_scans):
        if k > 0 and not (first < k < first + count):
            R = R @ rodrigues(np.deg2rad(np.array([0.1, -0.05, yaw_step_deg])))
            p = p + R @ np.array([step, 0.01, 0.002])
        Rs.append(R); ps.append(p)
    half = np.asarray(room, dtype=np.float64) / 2
    area = np.array([half[1] * half[2], half[1] * half[2], half[0] * half[2], half[0] * half[2], half[0] * half[1], half[0] * half[1]])
    points, variances = [], []
    empty = empty_scan if 0 <= empty_scan < n_scans else -1
    for k in range(n_scans):
        n = 0 if k == empty else int(pts_per_scan)
        face = rng.choice(6, size=n, p=area / area.sum())
        w = rng.uniform(-1.0, 1.0, size=(n, 3)) * half
        axis, sign = face // 2, np.where(face % 2 == 0, -1.0, 1.0)
        w[np.arange(n), axis] = sign * half[axis]
        w += noise * rng.normal(size=(n, 3))
        points.append(np.ascontiguousarray((w - ps[k]) @ Rs[k]))
        A = 0.01 * rng.normal(size=(n, 3, 3))
        variances.append(np.ascontiguousarray((A @ np.transpose(A, (0, 2, 1)) + 1e-6 * np.eye(3)).reshape(n, 9)))
    v6 = 1e-4 * (1.0 + 0.1 * np.arange(n_scans))[:, None] * np.ones((n_scans, 6))
    return ScanPoseStream(int(win_size), pack_poses(np.stack(Rs), np.stack(ps)), v6, points, variances, (first, count), empty)


def make_corner_scene(seed=MASTER_SEED + 9100, extent=12.0, n_walls=3, n_poles=8, n_boxes=3, density=30.0, noise=0.01, floor_z=-0.37, pole_radius=0.18,
                      motion=None):
    """A scene the corner extraction (``vxba.CornerExtractor``) finds corners in: a floor of ``extent`` x ``extent`` metres at ``floor_z`` (kept off the
    faces of 1 m and 2 m voxels), ``n_walls`` (two or three; none for a bare floor) walls 3 m high standing on it, and ``n_poles`` poles and ``n_boxes`` boxes of 1-4 m standing on the
    floor.  Points sit at continuous random positions (``density`` per square metre of surface, Gaussian ``noise`` along the surface normal), never on a
    lattice.  ``motion`` = (R (3, 3), t (3,)): the cloud is moved by x -> R x + t.  Returns (xyz (n, 3) float64, dict(poles, boxes, walls)).
    Deterministic in its arguments."""
    rng = np.random.default_rng(seed)
    half = extent / 2
    parts = []

    def sheet(origin, u, v, lu, lv, nrm):      # a rectangle origin + a u + b v, a in [0, lu), b in [0, lv)
        n = max(int(density * lu * lv), 12)
        a, b = rng.uniform(0, lu, n), rng.uniform(0, lv, n)
        parts.append(np.asarray(origin)[None, :] + a[:, None] * np.asarray(u)[None, :] + b[:, None] * np.asarray(v)[None, :] + noise * rng.normal(size=n)[:, None] * np.asarray(nrm)[None, :])

    ex, ey, ez = np.eye(3)
    sheet([-half + 0.13, -half + 0.21, floor_z], ex, ey, extent, extent, ez)
    walls = [([half + 0.13 - 0.31, -half + 0.21, floor_z], ey, ez, ex), ([-half + 0.13, half + 0.21 - 0.27, floor_z], ex, ez, ey), ([-half + 0.13 + 0.29, -half + 0.21, floor_z], ey, ez, ex)]
    for o, u, v, nrm in walls[:max(0, min(int(n_walls), 3))]:
        sheet(o, u, v, extent, 3.0, nrm)
    poles, boxes = [], []
    for _ in range(int(n_poles)):
        c = rng.uniform(-half + 1.5, half - 1.5, 2); h = rng.uniform(1.0, 4.0)
        n = max(int(density * 4 * h * 2 * np.pi * pole_radius), 60)
        ang, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, h, n)
        r = pole_radius + noise * rng.normal(size=n)
        parts.append(np.stack([c[0] + r * np.cos(ang), c[1] + r * np.sin(ang), floor_z + z], axis=1))
        poles.append((c[0], c[1], h))
    for _ in range(int(n_boxes)):
        c = rng.uniform(-half + 2.0, half - 2.0, 2); h = rng.uniform(1.0, 4.0); w = rng.uniform(0.6, 1.4, 2)
        o = np.array([c[0] - w[0] / 2, c[1] - w[1] / 2, floor_z])
        sheet(o, ex, ez, w[0], h, ey); sheet(o + w[1] * ey, ex, ez, w[0], h, ey)
        sheet(o, ey, ez, w[1], h, ex); sheet(o + w[0] * ex, ey, ez, w[1], h, ex)
        sheet(o + h * ez, ex, ey, w[0], w[1], ez)
        boxes.append((c[0], c[1], w[0], w[1], h))
    xyz = np.concatenate(parts)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    if motion is not None:
        R, t = np.asarray(motion[0], dtype=np.float64), np.asarray(motion[1], dtype=np.float64)
        xyz = xyz @ R.T + t[None, :]
    return np.ascontiguousarray(xyz), dict(poles=poles, boxes=boxes, walls=int(max(0, min(int(n_walls), 3))))


def make_corner_revisit_stream(n_visits=2, win_size=3, step=0.15, yaw_step_deg=0.5, seed=MASTER_SEED + 9155, extent=12.0, n_poles=10, revisit_noise=0.002, **scene_kw):
    """``n_visits * win_size`` ScanPoses of one ``make_corner_scene`` seen from a slowly moving sensor: every scan holds one ``win_size``-th of the scene in
    its body frame, so every keyframe (one per ``win_size`` scans under the reference's 0.1 m rule) is the whole scene -- a revisit of the keyframe
    before it; the later visits' points carry fresh noise.  Returns a list of (pose, v6, body points, None)."""
    world = make_corner_scene(seed=seed, extent=extent, n_poles=n_poles, **scene_kw)[0]
    rng = np.random.default_rng(seed + 1)
    scans = []
    for k in range(int(n_visits) * int(win_size)):
        R = rodrigues(np.deg2rad(np.array([0.0, 0.0, yaw_step_deg * k])))
        p = np.array([step * k, 0.02 * k, 0.0])
        pts = world[(k % win_size)::win_size]
        if k >= win_size:
            pts = pts + revisit_noise * rng.normal(size=pts.shape)
        scans.append((pack_poses(R[None], p[None])[0], 1e-4 * np.ones(6), np.ascontiguousarray((pts - p) @ R), None))
    return scans


# ------------------------------------------------------------------------------------------------------------
# Driver messages (vxba_intake_*, front.ScanIntake): arrays packed into the point bytes of a message of any layout.
# ------------------------------------------------------------------------------------------------------------
_TIME_DTYPES = {0: None, 1: "<f4", 2: "<u4", 3: "<f8"}          # vxba_scan_layout.time_type


def raw_times(toff, layout, time_head=0.0):
    """Seconds after the scan's begin -> the values a driver writes into the time field of ``layout``: float32 seconds (as is), uint32 nanoseconds
    (rounded), float64 ``time_head + toff`` (minus head), None (no time field)."""
    dt = _TIME_DTYPES[int(layout.time_type)]
    if dt is None:
        return None
    t = np.asarray(toff, dtype=np.float64)
    if dt == "<f4":
        return t.astype(np.float32)
    if dt == "<u4":
        return np.rint(t * 1e9).astype(np.uint32)
    return float(time_head) + t


def make_driver_message(xyz, times, layout, seed=MASTER_SEED + 990):
    """The point bytes of a driver message: n points of ``layout.point_step`` bytes, x y z (float32) and ``times`` -- the RAW values of the time field in
    its own type (raw_times; None without one) -- little-endian at the layout's offsets, every other byte filled with noise."""
    xyz = np.ascontiguousarray(xyz, dtype="<f4").reshape(-1, 3)
    n, step = xyz.shape[0], int(layout.point_step)
    rng = np.random.Generator(np.random.PCG64([seed, 35]))
    msg = rng.integers(0, 256, size=(n, step), dtype=np.uint8)
    for col, off in enumerate((int(layout.off_x), int(layout.off_y), int(layout.off_z))):
        msg[:, off:off + 4] = xyz[:, col:col + 1].copy().view(np.uint8).reshape(n, 4)
    dt = _TIME_DTYPES[int(layout.time_type)]
    if dt is not None:
        t = np.ascontiguousarray(times, dtype=dt).reshape(n, 1)
        w = t.dtype.itemsize
        msg[:, int(layout.off_time):int(layout.off_time) + w] = t.view(np.uint8).reshape(n, w)
    return msg.tobytes()
