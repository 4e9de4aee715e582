"""Shared inputs of tests/test_session_cpu.py and tests/test_gpu_session.py: small saved sessions (body-frame float32 scans + scan poses) that reach
every path of the saved-session unit.  Deterministic; nothing here computes an expected value."""
import numpy as np

from voxel_slam_amd import synth

VOXEL_SIZE = 1.0          # the filter runs at a tenth of it


def poses_for(n, seed=0, step=0.15):
    rng = np.random.default_rng(1000 + seed)
    Rs = np.stack([synth.rodrigues(np.deg2rad(np.array([0.3 * rng.normal(), 0.3 * rng.normal(), 0.7 * k]))) for k in range(n)]) if n else np.zeros((0, 3, 3))
    ps = np.stack([np.array([step * k, 0.02 * k, 0.01 * rng.normal()]) for k in range(n)]) if n else np.zeros((0, 3))
    return synth.pack_poses(Rs, ps) if n else np.zeros((0, 12))


def cloud(n, rng, cells=3):
    """n points in (2 cells)^3 voxels of 0.1 m around the origin (negative coordinates included): several points per voxel."""
    return (rng.integers(-cells, cells, size=(n, 3)) * 0.1 + rng.uniform(0.0, 0.1, size=(n, 3))).astype(np.float32)


def make_session(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [cloud(int(n), rng) for n in sizes], poses_for(len(sizes), seed)


def main_case():
    """7 scans at win_size 3: two keyframes, one scan dropped; sizes 300, 0 (an empty scan inside a group), 1, ...; in the LAST scan of the second group
    (whose relative pose is the identity up to rounding) points on and next to voxel borders, and two identical points."""
    scans, poses = make_session([300, 0, 1, 257, 300, 64, 50], seed=11)
    eps = np.float32(1e-6)
    b = np.array([-0.3, -0.2, -0.1, 0.0, 0.1, 0.2], dtype=np.float32)
    edge = np.concatenate([np.stack([b, b, b], 1), np.stack([b + eps, b - eps, b], 1), np.stack([b - eps, b, b + eps], 1)]).astype(np.float32)
    twin = np.tile(np.array([[0.123, -0.234, 0.045]], dtype=np.float32), (2, 1))
    scans[5] = np.concatenate([scans[5], edge, twin]).astype(np.float32)
    return dict(scans=scans, poses=poses, win_size=3, voxel_size=VOXEL_SIZE)


def window_case(K=5, win_size=3, seed=21):
    scans, poses = make_session([40 + 7 * (k % 5) for k in range(K * win_size)], seed=seed)
    return dict(scans=scans, poses=poses, win_size=win_size, voxel_size=VOXEL_SIZE)


def many_case(K=12, win_size=3, seed=31):
    scans, poses = make_session([20 + (k % 4) for k in range(K * win_size)], seed=seed)
    return dict(scans=scans, poses=poses, win_size=win_size, voxel_size=VOXEL_SIZE)


def moved_poses(poses, seed=5):
    """What an optimisation might return: every pose moved by one rigid motion plus a little of its own."""
    rng = np.random.default_rng(seed)
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    dR = synth.rodrigues(np.deg2rad(np.array([1.0, -2.0, 15.0])))
    out = []
    for k in range(P.shape[0]):
        R = P[k, :9].reshape(3, 3).T
        Rk = dR @ synth.rodrigues(np.deg2rad(0.2 * rng.normal(size=3))) @ R
        out.append((Rk, dR @ P[k, 9:] + np.array([2.0, -1.0, 0.3]) + 0.01 * rng.normal(size=3)))
    return synth.pack_poses(np.stack([r for r, _ in out]), np.stack([p for _, p in out]))
