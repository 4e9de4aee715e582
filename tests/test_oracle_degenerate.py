"""The oracle on degenerate voxels and non-finite residuals (tests/_degenerate.py), pinned to the reference's own code.

Every GPU test of the degenerate windows (tests/test_gpu_degenerate.py) judges the kernels against the oracle; these tests make sure
that on these inputs the oracle behaves like oracle/_ref/libref.so (the reference's voxel_map.hpp compiled against the API shim):
same finite / non-finite pattern in the residuals, eigenvalues and Hessian, same accept / reject schedule, same poses.  The premise
of each case (equal eigenvalues bit for bit, residual exactly 0, ...) is checked through the oracle alone and runs everywhere."""
import numpy as np
import pytest

from tests import _degenerate as D
from tests import _oracle as O
from tests import _ref

R = _ref.backend()
needs_ref = pytest.mark.skipif(R is None, reason="oracle/_ref/libref.so not available (needs /root/reference or a prebuilt copy)")


@pytest.fixture(autouse=True)
def _quiet():
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        yield


def run(B, case, iters=4):
    f = B.Oracle(case.win_size)
    f.push_voxels(case.clusters, case.fix, case.coe)
    r0 = f.evaluate_only_residual(case.poses_init)
    ev, _, _ = f.read_cache()
    H, J, r = f.acc_evaluate2(case.poses_init)
    f.evaluate_only_residual(case.poses_init)
    lm = f.damping_iter(case.poses_init, max_iter=iters, thd_num=2)
    return dict(f=f, r0=r0, ev=ev, H=H, J=J, r=r, lm=lm)


# what the reference does on each case (recorded from libref.so; test_reference_behaves_as_recorded re-derives it where it is present)
EXPECT = {
    "gauge_only": dict(all_rejected=False, residual_finite=True),
    "collinear": dict(all_rejected=True, residual_finite=True),
    "single_point": dict(all_rejected=True, residual_finite=True),
    "nan_point": dict(all_rejected=True, residual_finite=False),
    "inf_point": dict(all_rejected=True, residual_finite=False),
    "subrange": dict(all_rejected=True, residual_finite=True),
    "zero_residual": dict(all_rejected=True, residual_finite=True),
}


@pytest.mark.parametrize("name", D.CASES)
def test_degenerate_premise_and_oracle_behaviour(name):
    case = D.make(name)
    D.check_exact(case, O)
    o = run(O, case)
    lm = o["lm"]
    assert D.all_rejected(lm) == EXPECT[name]["all_rejected"]
    assert np.isfinite(o["r0"]) == EXPECT[name]["residual_finite"]
    if EXPECT[name]["all_rejected"]:
        assert np.array_equal(lm["poses"], case.poses_init)                   # nothing moves, bit for bit
        assert lm["trace"].shape[0] == 4 and not lm["is_converge"]            # no early stop (zero_residual: 0 / 0 is not < eps)
    if name in ("collinear", "single_point", "subrange"):
        # the degenerate voxel poisons exactly the block of the frame that sees it
        assert D.nonfinite_blocks(o["H"], case.win_size) == {(j, j) for j in case.observers}
        assert np.isfinite(lm["resis"][0]) and not np.isfinite(lm["resis"][1])
    if name == "gauge_only":
        # its non-finite terms land in block (0, 0), which the gauge fix overwrites: the window converges like the one without the voxel
        assert D.nonfinite_blocks(o["H"], case.win_size) == {(0, 0)}
        keep = np.ones(case.n_voxels, dtype=bool); keep[case.deg] = False
        f2 = O.Oracle(case.win_size)
        f2.push_voxels(case.clusters[keep], case.fix[keep], case.coe[keep])
        f2.evaluate_only_residual(case.poses_init)
        lm2 = f2.damping_iter(case.poses_init, max_iter=4, thd_num=2)
        assert np.array_equal(lm["trace"][:, 6:], lm2["trace"][:, 6:])
        assert np.allclose(lm["trace"][:, :2], lm2["trace"][:, :2], rtol=1e-12)
        assert np.allclose(lm["poses"], lm2["poses"], rtol=0, atol=1e-12)
    if name == "zero_residual":
        assert o["r0"] == 0.0 and np.all(np.isfinite(o["H"])) and np.all(lm["trace"][:, :2] == 0.0)


@needs_ref
@pytest.mark.parametrize("name", D.CASES)
def test_oracle_matches_the_reference_on_degenerate_windows(name):
    case = D.make(name)
    o, r = run(O, case), run(R, case)
    assert D.close_where_finite(o["r0"], r["r0"], rtol=1e-12) and D.close_where_finite(o["r"], r["r"], rtol=1e-12)
    assert D.close_where_finite(o["ev"], r["ev"], rtol=1e-9, atol=1e-15)
    assert D.finite_mask_equal(o["H"], r["H"]) and D.finite_mask_equal(o["J"], r["J"])
    assert D.close_where_finite(o["H"], r["H"], rtol=1e-9, atol=1e-12 * np.abs(r["H"][np.isfinite(r["H"])]).max(initial=1.0))
    lo, lr = o["lm"], r["lm"]
    assert lo["trace"].shape == lr["trace"].shape and np.array_equal(lo["trace"][:, 6:8], lr["trace"][:, 6:8])
    assert D.close_where_finite(lo["trace"][:, :2], lr["trace"][:, :2], rtol=1e-12)
    assert D.close_where_finite(lo["resis"], lr["resis"], rtol=1e-12)
    assert lo["is_converge"] == lr["is_converge"]
    if D.all_rejected(lr):
        assert np.array_equal(lo["poses"], lr["poses"]) and np.array_equal(lr["poses"], case.poses_init)
    else:
        assert np.allclose(lo["poses"], lr["poses"], rtol=0, atol=1e-12)
    assert D.all_rejected(lr) == EXPECT[name]["all_rejected"] and bool(np.isfinite(r["r0"])) == EXPECT[name]["residual_finite"]


@needs_ref
def test_subranges_around_a_degenerate_voxel_match_the_reference():
    """divide_thread's sub-ranges: [0, a) in front of the collinear voxel is finite, [a, V) carries its non-finite block."""
    case = D.make("subrange")
    a, V = case.deg[0], case.n_voxels
    fo, fr = (B.Oracle(case.win_size) for B in (O, R))
    for f in (fo, fr):
        f.push_voxels(case.clusters, case.fix, case.coe)
    for head, end in ((0, a), (a, V), (a + 1, V), (0, a + 1)):
        ro, rr = fo.evaluate_only_residual(case.poses_init, head, end), fr.evaluate_only_residual(case.poses_init, head, end)
        assert ro == rr and np.isfinite(rr)
        (Ho, Jo, so), (Hr, Jr, sr) = fo.acc_evaluate2(case.poses_init, head, end), fr.acc_evaluate2(case.poses_init, head, end)
        assert so == sr
        assert D.nonfinite_blocks(Hr, case.win_size) == ({(j, j) for j in case.observers} if head <= a < end else set())
        assert D.close_where_finite(Ho, Hr, rtol=1e-9, atol=1e-12 * np.abs(Hr[np.isfinite(Hr)]).max())
        assert D.close_where_finite(Jo, Jr, rtol=1e-9, atol=1e-12 * np.abs(Jr[np.isfinite(Jr)]).max())
