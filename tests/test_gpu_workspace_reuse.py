"""One grow-only device workspace per handle (csrc/vxba_dev.hpp: vxu::Arena), carved anew by every call: what fresh allocations cannot get wrong and a
shared workspace can -- stale contents of a larger earlier call, a regrow in the middle of a handle's life, a refused call that leaves its work behind.
Every entry point that carves one runs the point counts COUNTS in that order on ONE handle: 3000 -> 20000 crosses the growth, 20000 -> 65 and 3000 -> 1
reuse the block at a smaller size; after the largest call one call is refused and the next must be right again.  Each result is held to the checker its
neighbouring test uses, in the same way."""
import numpy as np
import pytest

from tests import _init_ref as IR
from tests import _keyframe_ref as KR
from tests import _loopreg_ref as LR
from tests import _oracle as O
from tests.test_gpu_keyframe import same_keyframe
from tests.test_gpu_loopreg import NORMAL_BOUND

pytestmark = pytest.mark.gpu

COUNTS = (3000, 1, 65, 20000, 65)
REFUSE_AFTER = 3          # ... the 20000-point call: the refused call and the 65-point one after it find the most left behind


def _cloud32(rng, n):
    """Gaussian points of a few voxels' spread, a tenth of them on voxel faces (tests/test_gpu_lio.py::test_down_sampling_voxel_is_bit_identical)."""
    xyz = (rng.normal(size=(n, 3)) * 2).astype(np.float32)
    xyz[: n // 10] = np.round(xyz[: n // 10] / 0.5) * 0.5
    if n > 10:
        xyz[5] = xyz[9]
    return xyz


def test_down_sampling_on_the_per_device_scratch():
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(8300)
    for k, n in enumerate(COUNTS):
        xyz = _cloud32(rng, n)
        assert np.array_equal(vxba.down_sampling_voxel(xyz, 0.5), O.down_sampling_voxel(xyz, 0.5)), (k, n)
        pts, sel = vxba.down_sampling_close(xyz, 0.5)
        want_p, want_s = IR.down_sampling_close(xyz, 0.5)
        assert np.array_equal(sel, want_s) and np.array_equal(pts, want_p), (k, n)
        if k == REFUSE_AFTER:
            bad = _cloud32(rng, 3000); bad[7] = (3e6, 0, 0)
            with pytest.raises(vxba.VxbaError):
                vxba.down_sampling_voxel(bad, 0.5)
            with pytest.raises(vxba.VxbaError):
                vxba.down_sampling_close(bad, 0.5)


def _planes(rng, n):
    """n points on a slightly rough plane, about fifty to a 1 m voxel (65 and fewer: inside one voxel), in random order."""
    half = max(1, int(round(np.sqrt(n / 50.0) / 2)))
    xy = rng.uniform(-half, half, size=(n, 2)) if n > 100 else rng.uniform(0.05, 0.95, size=(n, 2))
    z = 0.3 + 0.05 * xy[:, 0] - 0.03 * xy[:, 1] + rng.normal(0, 0.005, n)
    return np.ascontiguousarray(np.concatenate([xy, z[:, None]], axis=1))


def test_loopreg_add_keyframe_on_one_handle():
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(8301)
    with vxba.LoopRegistration() as r:
        for k, n in enumerate(COUNTS):
            c = _planes(rng, n)
            got = r.read_cloud(r.add_keyframe(c))
            want = LR.plane_cloud(c)
            rows, lam = want["rows"], want["lam"]
            assert got.shape == rows.shape and (got.shape[0] > 0) == (n >= 65), (k, n, got.shape, rows.shape)
            assert np.array_equal(LR.voxel_coords(got[:, :3].astype(np.float64), 1.0), want["coords"]), (k, n)
            assert np.all(np.abs(got[:, :3] - rows[:, :3]) <= np.spacing(np.abs(rows[:, :3]))), (k, n)
            well = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
            assert np.all(np.abs(got[well, 3:].astype(np.float64) - rows[well, 3:].astype(np.float64)) <= NORMAL_BOUND), (k, n)
            if k == REFUSE_AFTER:
                bad = _planes(rng, 3000); bad[7, 0] = 2.0 ** 20 + 0.5
                before = r.num_clouds()
                with pytest.raises(vxba.VxbaError, match="beyond 2\\^20 voxels"):
                    r.add_keyframe(bad)
                assert r.num_clouds() == before


def test_keyframe_builder_on_one_handle():
    """win_size 2 and a metre between pushes: every push that completes a window emits, a keyframe of two scans of the count's size."""
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(8302)
    b, r = vxba.KeyframeBuilder(2, 1.0), KR.KeyframeRef(2, 1.0)
    v6 = np.full(6, 1e-4)
    step = 0

    def pose():
        nonlocal step
        step += 1
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, float(step), 0.25, 0], dtype=np.float64)

    for k, n in enumerate(COUNTS):
        first, second = rng.uniform(-1, 1, size=(n, 3)), rng.uniform(-1, 1, size=(n, 3))
        P = pose()
        assert not b.push_scan(P, v6, first) and not r.push_scan(P, v6, first)
        if k == REFUSE_AFTER:
            bad = second.copy(); bad[n // 2, 1] = np.inf
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
                b.push_scan(pose(), v6, bad)
            assert b.num_buffered() == 1 and b.num_scans() == 2 * k + 1
        P = pose()
        assert b.push_scan(P, v6, second) and r.push_scan(P, v6, second), (k, n)
        same_keyframe(b, r.keyframe)
        assert b.info()["n_full"] == 2 * n and 0 < b.info()["n_down"] <= 2 * n
    b.close()
