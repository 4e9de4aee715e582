"""Inputs shared by tests/test_keyframe_cpu.py (which asserts that every case contains what it claims) and tests/test_gpu_keyframe.py (which runs them
on the device against tests/_keyframe_ref.py).  A case is one keyframe: ``win_size`` scans whose last push emits (the first window of a session
always does).  The edge cases use identity poses and voxel_size 2.5, so the filter's edge vs = 0.25 and every lattice coordinate are exact in
binary and the merged point equals the body point bit for bit."""
import numpy as np

IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
MOVED = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0, 0, 0], dtype=np.float64)      # one metre on: a push with this pose completes a window AND emits
V6 = np.full(6, 1e-4)
VOXEL_SIZE = 2.5
VS = VOXEL_SIZE / 10
TOP = (1 << 20) - 1          # the largest voxel index in magnitude
KEY_BLOCK = 256              # lanes per workgroup of the assembly (key) kernel


def _var(rng, n):
    A = 0.02 * rng.normal(size=(n, 3, 3))
    return np.ascontiguousarray((A @ np.transpose(A, (0, 2, 1))).reshape(n, 9))


def _case(name, scans, win=3, voxel_size=VOXEL_SIZE, poses=None, seed=0):
    rng = np.random.default_rng(1000 + seed)
    poses = [IDENT] * win if poses is None else poses
    return dict(name=name, win=win, voxel_size=voxel_size,
                scans=[(np.asarray(poses[k], dtype=np.float64), V6, np.ascontiguousarray(s, dtype=np.float64).reshape(-1, 3), _var(rng, np.asarray(s).reshape(-1, 3).shape[0]))
                       for k, s in enumerate(scans)])


def lattice(n, first=0, jitter=None):
    """n points in n distinct voxels: voxel (i, -i // 7, i % 5 - 2) for i = first ..., at the voxel's centre (plus jitter inside +-0.4 of a voxel)."""
    i = np.arange(first, first + n)
    idx = np.stack([i, -(i // 7), i % 5 - 2], axis=1).astype(np.float64)
    off = 0.5 if jitter is None else 0.5 + 0.4 * jitter.uniform(-1, 1, size=(n, 3))
    return (idx + off) * VS


def ragged():
    """win_size 3 with scans of 257, 0 and 64 points under moving poses: a scan one past a workgroup, an empty one, a short one."""
    from voxel_slam_amd import synth
    st = synth.make_scanpose_stream(3, 257, 3, stationary=False, empty_scan=1, seed=77)
    pts = [st.points[0], st.points[1], st.points[2][:64]]
    return _case("ragged", pts, voxel_size=1.0, poses=list(st.poses), seed=1)


def heavy_voxel():
    """One voxel of 300 points -- rows 100 .. 399 of the first scan, so its run crosses the workgroup boundary at row 256 -- among single-point voxels."""
    rng = np.random.default_rng(5)
    heavy = (np.array([3.0, -2.0, 1.0]) + rng.uniform(0.02, 0.98, size=(300, 3))) * VS
    s0 = np.concatenate([lattice(100, 1000), heavy, lattice(100, 2000)])
    return _case("heavy_voxel", [s0, lattice(10, 3000), lattice(10, 4000)], seed=2)


def distinct():
    rng = np.random.default_rng(6)
    return _case("distinct", [lattice(70, 0, rng), lattice(70, 70, rng), lattice(70, 140, rng)], seed=3)


def single_point():
    return _case("single_point", [np.zeros((0, 3)), np.zeros((0, 3)), np.array([[0.3, -0.7, 1.1]])], seed=4)


def voxels(n_vox):
    """n_vox occupied voxels with two or three points each, spread over the three scans."""
    rng = np.random.default_rng(7 + n_vox)
    base = lattice(n_vox, 50) - 0.5 * VS
    scans = [base + rng.uniform(0.05, 0.95, size=base.shape) * VS for _ in range(3)]
    scans[2] = scans[2][: max(1, n_vox // 2)]
    return _case(f"voxels_{n_vox}", scans, seed=5)


def edges():
    """Coordinates at -vs, -0.0, just below 0, and the two outermost voxel indices.  +TOP vs is an exact multiple and lands in voxel +TOP; a NEGATIVE exact
    multiple -k vs lands in voxel -k - 1 (upstream subtracts 1.0 from every negative quotient), so voxel -TOP is reached from -(TOP - 0.5) vs."""
    tiny = -np.nextafter(0.0, 1.0)
    col = np.array([-VS, -0.0, tiny, -1e-30, TOP * VS, -(TOP - 0.5) * VS, -2 * VS, 0.0, VS, -3 * VS + 1e-9])
    rng = np.random.default_rng(8)
    s = [np.stack([col, rng.permutation(col), rng.permutation(col)], axis=1) for _ in range(3)]
    s[1] = np.stack([col, col, col], axis=1)
    return _case("edges", s, seed=6)


def all_cases():
    return [ragged(), heavy_voxel(), distinct(), single_point(), voxels(1), voxels(65), edges()]


def bad_cases():
    """(name, the scan that must be refused when it completes a window under the pose MOVED -- the newest scan's merged points are its body points): a NaN
    point; voxel index 2^20; voxel index -2^20 (the exact multiple -TOP vs)."""
    ok = lattice(5)
    nan = ok.copy(); nan[2, 1] = np.nan
    far = ok.copy(); far[3, 0] = (TOP + 1) * VS
    neg = ok.copy(); neg[1, 2] = -TOP * VS
    return [("nan", nan), ("index_2^20", far), ("index_-2^20", neg)]


# ---- the keyframe rule: a stream with a hand-written expectation (voxelslam.cpp:1928-1942) ----
def rule_stream():
    """14 pushes, win_size 3: (x position, yaw in degrees); a few points per scan so that a keyframe's size says which scans it holds."""
    from voxel_slam_amd import synth
    xs = [0.0, 0.05, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.5, 0.5, 0.5]
    yaw = [0, 0, 0, 0, 0, 0, 0, 6, 6, 6, 6, 6, 6, 6]
    poses = synth.pack_poses(np.stack([synth.rodrigues(np.deg2rad([0.0, 0.0, y])) for y in yaw]), np.stack([[x, 0.0, 0.0] for x in xs]))
    rng = np.random.default_rng(9)
    return [(poses[k], np.full(6, 1e-4 * (k + 1)), rng.uniform(-1, 1, size=(k + 1, 3)), None) for k in range(14)]


RULE_EMITTED = [0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0]
RULE_ACTION = ["buffer", "buffer", "emit", "buffer", "buffer", "drop", "drop", "emit", "buffer", "buffer", "drop", "emit", "buffer", "buffer"]
RULE_BUFFERED = [1, 2, 0, 1, 2, 2, 2, 0, 1, 2, 2, 0, 1, 2]
RULE_IDS = {2: 2, 7: 7, 11: 11}
RULE_SCANS = {2: (0, 1, 2), 7: (5, 6, 7), 11: (9, 10, 11)}         # the scans each keyframe holds: the drops at pushes 5, 6 and 10 removed scans 3, 4 and 8
RULE_JOUR = {2: 0.2, 7: 0.2 + 0.0, 11: 0.2 + 0.0 + (0.5 - 0.2)}
