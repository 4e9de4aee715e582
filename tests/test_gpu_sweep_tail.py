"""The reduction behind the Hessian sweep at chosen numbers of workgroup partials, and the sweep's tail at chosen shapes (run with ``-m gpu``).

k3_finalize_kernel requests up to four workgroup partials per thread before it knows what an element is, on clamped indices, works the
element out from immediates and leaves out of its sums what does not count (csrc/vxba_kernels.hip).  How many partials there are is the
launch rule's business (k3_blocks_for, csrc/vxba_kernels.h: one workgroup per PAIR of batches, at most one per CU; a fused launch gives one
CU to the solve): `_split` restates it, and every test asserts the shape it is named for against it.  The sweep itself (csrc/vxba_k3.hpp)
and the residual sweep's eigen-solver are unchanged; their cases here are regression tests at shapes no other test pins down: a workgroup
with a given number of full steps and ragged batches, whole and partly filled batches, and one wave of the residual sweep whose cached
eigenvectors are exact, near and far off.

Bounds: the literals tests/test_gpu_parity.py uses for the same quantities (it keeps them inside its tests, so they are restated here, each
with the test it comes from; that file's helpers are imported)."""
import numpy as np
import pytest

from tests import _oracle as O
from tests.test_gpu_parity import relerr, seeded_pair, vx  # noqa: F401 -- vx: that module's library fixture
from voxel_slam_amd import synth

pytestmark = pytest.mark.gpu

def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nv(W):
    """K3Cfg<W>::NV (csrc/vxba_k3.hpp): voxels per wave and batch."""
    nt = (6 * W + 15) // 16
    cap = 12 if nt <= 2 else (8 if nt == 3 else 6)
    return min(64 // W, cap)


def _split(W, head, end, cus):
    """The launch rule restated: (number of workgroups = partials, {(full steps, ragged batches) of a workgroup}) of a sweep over [head, end)
    on `cus` CUs -- k3_blocks_for (csrc/vxba_kernels.h) and the contiguous, evenly sized runs of k3_sweep_body."""
    nv = _nv(W)
    nb = (end - 1) // nv - head // nv + 1
    nwg = max(1, min((nb + 1) // 2, cus))
    q, rem = divmod(nb, nwg)
    return nwg, {(c // 8, c % 8) for c in ([q + 1] if rem else []) + ([q] if rem < nwg else [])}


def _scene(W, V, seed):
    return synth.make_scene(win_size=W, pts_per_scan=8 * V if V >= 256 else 4000, n_voxels=V, p_obs=0.8, fix_frac=0.2, seed=seed, rot_sigma_deg=0.1, trans_sigma=0.03)


def _check_system(fo, fg, poses, head=0, end=None):
    """acc_evaluate2 (packed Hess | JacT | residual) against the oracle; twice: identical bits."""
    H_ref, J_ref, r_ref = fo.acc_evaluate2(poses, head, end)
    H, J, r = fg.acc_evaluate2(poses, head, end)
    print(f"  [{head}, {end}): relerr H {relerr(H, H_ref):.2e}  J {relerr(J, J_ref):.2e}  r {abs(r - r_ref) / abs(r_ref):.2e}")
    # test_gpu_parity.py::test_hessian_sweep_and_lm_loop_with_full_steps_every_window_size: 1e-10, 1e-10, 1e-12; H == H.T
    assert relerr(H, H_ref) < 1e-10 and relerr(J, J_ref) < 1e-10 and abs(r - r_ref) <= 1e-12 * abs(r_ref)
    assert np.array_equal(H, H.T)
    # test_gpu_parity.py::test_shard_invariance_and_determinism: run-to-run bitwise
    H2, J2, r2 = fg.acc_evaluate2(poses, head, end)
    assert np.array_equal(H, H2) and np.array_equal(J, J2) and r == r2


def _check_loop_forms(vx, sc):  # noqa: F811
    """lm_steps with the fused residual + Hessian launch and as three launches: the same steps, the same poses and residual to round-off."""
    res = []
    for fused in (1, 0):
        f = vx.LidarFactor(sc.win_size)
        f.push_voxels(sc.clusters, sc.fix, sc.coe)
        f.evaluate_only_residual(sc.poses_init)
        f.set_option("fused_sweeps", fused)
        f.snapshot_cache()
        res.append(f.lm_steps(sc.poses_init, 6, 3))
        f.close()
    print(f"  fused vs three launches: poses {np.abs(res[0][0] - res[1][0]).max():.2e}  residual {abs(res[0][1][1] / res[1][1][1] - 1):.2e}")
    assert res[0][2] == res[1][2] and res[0][2]["iters"] == 6, (res[0][2], res[1][2])
    # test_gpu_parity.py::test_fused_launch_is_the_three_launch_iteration_to_round_off, bench-driver leg: atol 1e-11, rtol 1e-10
    assert np.allclose(res[0][0], res[1][0], rtol=0, atol=1e-11) and np.isclose(res[0][1][1], res[1][1][1], rtol=1e-10)


# (full steps, ragged batches) of EVERY workgroup of the stand-alone sweep at W = 10 on 256 CUs: 256 x (8 nfull + nrag) batches of six voxels.
# One batch per workgroup on all 256 CUs cannot be reached: the launch rule gives a workgroup per pair of batches, so (0, 1) occurs as the
# one short workgroup of an odd batch count -- 511 batches: 255 workgroups at (0, 2), the last at (0, 1) -- and as the only workgroup of a
# sweep over one batch (test_reduction_at_every_count_of_partials[1]).
TAIL_CASES = [(0, 1, 6 * 511), (0, 2, 6 * 512), (0, 7, 10_752), (1, 1, 13_824), (1, 7, 23_040), (2, 3, 29_184)]


def _assert_shape(W, head, end, nfull, nrag, only=False):
    cus = _cus()
    assert cus == 256, f"the shapes are laid out for the 256 CUs of an MI355X, this device has {cus}"
    nwg, shapes = _split(W, head, end, cus)
    assert nwg == 256 and (nfull, nrag) in shapes and (not only or shapes == {(nfull, nrag)}), (nwg, shapes)


@pytest.mark.parametrize("nfull,nrag,V", TAIL_CASES)
def test_ragged_step_at_every_tail_shape(vx, nfull, nrag, V):  # noqa: F811
    _assert_shape(10, 0, V, nfull, nrag, only=(nfull, nrag) != (0, 1))
    sc = _scene(10, V, 2100 + 8 * nfull + nrag)
    fo, fg = seeded_pair(vx, sc)
    _check_system(fo, fg, sc.poses_init)
    _check_loop_forms(vx, sc)
    fg.close()


@pytest.mark.parametrize("nfull,nrag,V", TAIL_CASES)
def test_ragged_step_with_both_kinds_of_workgroup(vx, nfull, nrag, V):  # noqa: F811
    """A voxel count that is no multiple of 6 x 256: the first workgroups own one batch more than the others, the last batch is partly
    filled; then a sub-range whose head and end sit inside a batch."""
    V2 = V + 6 * 100 + 3
    nwg, shapes = _split(10, 0, V2, _cus())
    assert nwg == 256 and len(shapes) == 2, (nwg, shapes)
    sc = _scene(10, V2, 2200 + 8 * nfull + nrag)
    fo, fg = seeded_pair(vx, sc)
    _check_system(fo, fg, sc.poses_init)
    _check_system(fo, fg, sc.poses_init, 7, V2 - 4)
    _check_loop_forms(vx, sc)
    fg.close()


def test_fewer_batches_than_workgroups(vx):  # noqa: F811
    sc = _scene(10, 100, 2301)
    fo, fg = seeded_pair(vx, sc)
    _check_system(fo, fg, sc.poses_init)
    _check_system(fo, fg, sc.poses_init, 3, 95)
    _check_loop_forms(vx, sc)
    fg.close()


@pytest.mark.parametrize("W", [3, 7])
def test_one_full_step_and_one_ragged_batch_at_other_window_sizes(vx, W):  # noqa: F811
    """(1, 1) at an odd window size (two padding columns in the tile; twelve and eight voxels per batch)."""
    V = _nv(W) * 256 * 9
    _assert_shape(W, 0, V, 1, 1, only=True)
    sc = _scene(W, V, 2400 + W)
    fo, fg = seeded_pair(vx, sc)
    _check_system(fo, fg, sc.poses_init)
    _check_system(fo, fg, sc.poses_init, 5, V - 7)
    _check_loop_forms(vx, sc)
    fg.close()


@pytest.mark.parametrize("nparts", [1, 63, 64, 65, 255, 256])
def test_reduction_at_every_count_of_partials(vx, nparts):  # noqa: F811
    """k3_finalize_kernel adds the workgroup partials 64 at a time (one slice of threads per partial), up to four per thread in its first
    round: with 1, 63, 64, 65, 255 and 256 partials slice 63 has a partial or none, slice 0 one or two, and every thread none to four.  A
    sweep over 2 p - 1 batches runs on p workgroups (511 batches: 256); the sub-range call moves head and end off a batch boundary and
    must leave the count where it is."""
    nb = 2 * nparts - 1 if nparts < 256 else 511
    V = 6 * nb
    cus = _cus()
    assert cus >= nparts, f"{nparts} partials need as many CUs, this device has {cus}"
    assert _split(10, 0, V, cus)[0] == nparts and _split(10, 1, V - 1, cus)[0] == nparts
    sc = _scene(10, V, 2500 + nparts)
    fo, fg = seeded_pair(vx, sc)
    _check_system(fo, fg, sc.poses_init)
    _check_system(fo, fg, sc.poses_init, 1, V - 1)
    fg.close()


def test_one_wave_with_warm_starts_exact_near_and_far_off(vx):  # noqa: F811
    """The cache goes up through push_voxels' record upload with eigenvectors that are exact for most voxels, 1e-5 rad off for every fifth,
    1e-3 for every third and far off for every seventh (the eigen-solver's generic fallback): every wave of the residual sweep holds all
    four kinds of warm start, whose three fixed sweeps and fallback must give the oracle's residual and cache."""
    from scipy.spatial.transform import Rotation
    W, V = 10, 1500
    sc = synth.make_scene(win_size=W, pts_per_scan=12 * V, n_voxels=V, p_obs=0.6, fix_frac=0.3, seed=2600, rot_sigma_deg=0.2, trans_sigma=0.03)
    coe = np.linspace(0.5, 2.0, V)
    fo = O.Oracle(W); fo.push_voxels(sc.clusters, sc.fix, coe)
    r_ref = fo.evaluate_only_residual(sc.poses_init)
    ev_ref, U_ref, m_ref = fo.read_cache()
    rng = np.random.default_rng(2601)
    Us = U_ref.reshape(V, 3, 3).transpose(0, 2, 1).copy()            # (n, 9) column-major -> matrices with the eigenvectors in their columns
    angle = np.zeros(V)
    angle[::5] = 1e-5; angle[::3] = 1e-3; angle[::7] = 0.7
    for a in np.nonzero(angle)[0]:
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        Us[a] = Us[a] @ Rotation.from_rotvec(axis * angle[a]).as_matrix()
    U_start = np.ascontiguousarray(Us.transpose(0, 2, 1).reshape(V, 9))
    fg = vx.LidarFactor(W); fg.push_voxels(sc.clusters, sc.fix, coe, ev_ref, U_start, m_ref)
    r = fg.evaluate_only_residual(sc.poses_init)
    ev, U, m = fg.read_cache()
    vb2 = np.sum((m_ref[:, 6:9] / m_ref[:, 9:10]) ** 2, axis=1, keepdims=True)
    d = np.abs(np.einsum("nck,nck->nc", U.reshape(V, 3, 3), U_ref.reshape(V, 3, 3)))
    Um = U.reshape(V, 3, 3)
    print(f"  residual {abs(r - r_ref) / abs(r_ref):.2e}  eigenvalues {np.max(np.abs(ev - ev_ref) / (vb2 + 1.0)):.2e}  normal {np.max(1 - d[:, 0]):.2e}")
    # test_gpu_parity.py::test_k2_residual_sweep_matches_oracle: every bound below
    assert abs(r - r_ref) <= 1e-10 * abs(r_ref)
    assert np.array_equal(m[:, 9], m_ref[:, 9]) and np.allclose(m, m_ref, rtol=1e-13, atol=1e-9)
    assert np.all(np.abs(ev - ev_ref) <= 1e-14 * (vb2 + 1.0))
    assert np.all(d[:, 0] > 1 - 1e-8)                                  # plane normal up to sign
    assert np.allclose(np.einsum("nck,ndk->ncd", Um, Um), np.eye(3)[None], atol=1e-13)
    fg.close()
