"""The inputs of tests/test_gpu_loopreg.py, built in one place so that tests/test_loopreg_cpu.py can hold every one of them against the conditions
that keep the GPU tests honest (no exact float32 distance ties, decisive gate verdicts and step norms, no eigenvalue on the plane threshold)."""
import functools

import numpy as np

from tests import _loopreg_ref as R
from voxel_slam_amd import synth

KEYFRAMES = ((0, 1, 2, 3), (4, 5, 6, 7), (8, 9, 10, 11), (2, 3, 4, 5))      # scans of synth.make_scans(win_size=12, ...) merged per keyframe
SCORE_THRESHOLDS = (0.2, 0.5)                                               # normal_threshold_, dis_threshold_ (BTC.cpp:33-34)


def perturbed(pose, rot_deg, tr):
    Rm, t = synth.unpack_poses(np.asarray(pose)[None])
    return synth.pack_poses((Rm[0] @ synth.rodrigues(np.deg2rad(np.asarray(rot_deg, dtype=np.float64))))[None], (t[0] + np.asarray(tr, dtype=np.float64))[None])[0]


@functools.lru_cache(maxsize=None)
def keyframes():
    """Four keyframe clouds of one scene with their world poses: dict(clouds, poses, planes: the checker's plane clouds)."""
    xyz, fp, _, gt = synth.make_scans(win_size=12, pts_per_scan=60_000, extent=20.0, noise=0.01)
    clouds = [synth.merge_keyframe(xyz, fp, gt, list(ids)) for ids in KEYFRAMES]
    poses = [gt[ids[0]] for ids in KEYFRAMES]
    return dict(clouds=clouds, poses=poses, planes=[R.plane_cloud(c) for c in clouds])


@functools.lru_cache(maxsize=None)
def boundary_cloud():
    """A slightly rough plane sampled on a lattice of eighths across the origin: many points lie exactly on cell boundaries, on both sides of zero
    (an exact negative integer belongs to the cell BELOW it: BTC.cpp:290-292 subtracts 1.0 before truncating)."""
    g = np.arange(-3.0, 3.0 + 1e-9, 0.125)
    x, y = np.meshgrid(g, g, indexing="ij")
    rng = np.random.default_rng(41)
    z = -0.3 + 0.05 * x - 0.03 * y + rng.normal(0, 0.005, x.shape)
    pts = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return np.ascontiguousarray(pts[rng.permutation(pts.shape[0])])


@functools.lru_cache(maxsize=None)
def big_pair():
    """50 000 x 50 000 random planes in a 40 m box: many LDS tiles, a last tile and a last workgroup that are not full."""
    rng = np.random.default_rng(78)
    def cloud(n):
        p = rng.uniform(-20, 20, (n, 3)); nv = rng.normal(size=(n, 3)); nv /= np.linalg.norm(nv, axis=1)[:, None]
        return np.concatenate([p, nv], axis=1).astype(np.float32)
    pose = R.pose_of(synth.rodrigues(np.array([0.02, -0.01, 0.03])), [0.1, -0.2, 0.05])
    return cloud(50_000), cloud(50_000), pose


def duplicated_target(tar):
    """Every target row twice: the copy has the higher index, so the lowest-index rule must return the original."""
    return np.ascontiguousarray(np.concatenate([tar, tar]))


def pair_truth(kf, s, t):
    return synth.relative_pose(kf["poses"][t], kf["poses"][s])


@functools.lru_cache(maxsize=None)
def score_batch():
    """64 hypotheses over the four plane clouds: (src_tar (64, 2), poses (64, 12))."""
    kf = keyframes()
    rng = np.random.default_rng(11)
    st, poses = [], []
    for b in range(64):
        s, t = b % 4, (b // 4) % 4
        st.append((s, t)); poses.append(perturbed(pair_truth(kf, s, t), rng.uniform(-3, 3, 3), rng.uniform(-0.4, 0.4, 3)))
    return np.array(st, dtype=np.int32), np.stack(poses)


ICP_SUBSETS = (None, None, None, None, 1500, 1000, 700, 300)     # clouds 4-7: the first rows of clouds 0-3


@functools.lru_cache(maxsize=None)
def icp_clouds():
    kf = keyframes()
    return [kf["planes"][k % 4]["rows"] if n is None else np.ascontiguousarray(kf["planes"][k % 4]["rows"][:n]) for k, n in enumerate(ICP_SUBSETS)]


@functools.lru_cache(maxsize=None)
def icp_batch():
    """32 pairs of different sizes and guesses over eight clouds: (src_tar (32, 2), poses (32, 12))."""
    kf = keyframes()
    rng = np.random.default_rng(24)
    st, poses = [], []
    for b in range(32):
        s, t = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        scale = (0.3, 1.0, 2.0, 4.0)[b % 4]
        st.append((s, t)); poses.append(perturbed(pair_truth(kf, s % 4, t % 4), scale * rng.uniform(-1.5, 1.5, 3), scale * rng.uniform(-0.2, 0.2, 3)))
    return np.array(st, dtype=np.int32), np.stack(poses)


# ---- end to end: a corridor session whose end sees its beginning again ---------------------------------------------------------------
E2E = dict(K=40, pts=100_000, seed=synth.MASTER_SEED + 8100, candidates=(0, 2, 4), v6=(1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4))


@functools.lru_cache(maxsize=None)
def revisit():
    """dict(cloud_cur, candidates [(index, cloud)], guesses (from the drifted odometry), cur_index, poses (drifted), gt)."""
    clouds, _, gt = synth.corridor_session(E2E["K"], E2E["pts"], E2E["seed"])
    poses = synth.drifted_odometry(gt)
    cur = E2E["K"] - 1
    cands = [(i, np.asarray(clouds[i], dtype=np.float64)) for i in E2E["candidates"]]
    guesses = np.stack([synth.relative_pose(poses[i], poses[cur]) for i in E2E["candidates"]])
    return dict(cloud_cur=np.asarray(clouds[cur], dtype=np.float64), candidates=cands, guesses=guesses, cur_index=cur, poses=poses, gt=gt)


class CheckerRegistration:
    """tests/_loopreg_ref.py behind the methods of vxba.LoopRegistration that hba.loop_registration calls."""

    def __init__(self):
        self.clouds = []

    def close(self):
        pass

    def add_keyframe(self, xyz, params=None):
        kw = {} if params is None else dict(voxel_size=params.voxel_size, voxel_init_num=params.voxel_init_num, plane_detection_thre=params.plane_detection_thre)
        self.clouds.append(R.plane_cloud(xyz, **kw)["rows"])
        return len(self.clouds) - 1

    def add_cloud(self, rows):
        self.clouds.append(np.asarray(rows, dtype=np.float32).reshape(-1, 6))
        return len(self.clouds) - 1

    def score(self, src_tar, poses, normal_threshold, dis_threshold):
        r = [R.score(self.clouds[s], self.clouds[t], P, normal_threshold, dis_threshold) for (s, t), P in zip(src_tar, poses)]
        self.last_score = r
        return np.array([x["score"] for x in r]), np.array([x["useful"] for x in r], dtype=np.int64)

    def icp(self, src_tar, poses, options=None):
        kw = {} if options is None else dict(max_iter=options.max_iter, gates0=tuple(options.gates0), gates1=tuple(options.gates1), step_tol=options.step_tol, icp_eigval=options.icp_eigval)
        r = [R.icp(self.clouds[s], self.clouds[t], P, **kw) for (s, t), P in zip(src_tar, poses)]
        self.last_icp = r
        return dict(poses=np.stack([x["pose"] for x in r]), report=np.stack([report_row(x) for x in r]))


def report_row(r):
    return np.array([float(r["accept"]), r["is_converge"], r["iterations"], r["match_num"], *r["eig"], r["resi"]], dtype=np.float64)
