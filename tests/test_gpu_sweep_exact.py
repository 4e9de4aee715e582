"""Every sweep on its own against exact arithmetic (run with ``-m gpu``): k2_residual_kernel, k3_hessian_kernel / k3_sweep_body, the
residual sweep with the in-launch solve, the Hessian half of k23_fused_kernel, k2_wide_kernel, k3w_blocks_kernel + k3w_combine_kernel.

The windows, the seeded cache, the criteria and where their constants come from: tests/_sweep_cases.py.  The reference: tests/_sweep_ref.py
(mpmath, 200 bits).  tests/test_sweep_cpu.py checks both without a GPU and shows that degraded sweeps fail these same checks.

  * evaluate_only_residual on every case: merged clusters, decompositions (backward errors on the row the sweep itself wrote) and the scalar;
    a second, warm-started call at other poses; a sub-range call, after which the cache rows outside [head, end) keep their bits.  Narrow
    store, and the wide store through push_voxels and through push_voxels_csr -- wide11's compressed rows carry one entry WITHOUT points
    (N == 0 beside stale moments; the push accepts it), which k2_wide_kernel and k3w_blocks_kernel must skip on N alone;
  * acc_evaluate2 from the seeded cache on every case and every sub-range; wide windows through both pushes, each in two appends with a sweep
    in between, so that the incidence index is built, invalidated and rebuilt;
  * acc_evaluate2 after the device's own residual sweep (V <= 33): the reference is evaluated from the cache read back, which covers the
    auxiliary scales the residual sweep writes where a push computes them;
  * the fused launch.  Read in csrc/vxba_capi_lm.hip (queue_lm_steps): a fused launch [solve | residual half | the NEXT step's Hessian half]
    is only queued where another step of the window follows, and the last step of every call is [solve | residual sweep] on its own.  So
    damping_iter(max_iter = 1) never runs the fused launch: the cache it leaves is the in-launch-solve residual sweep's at the accepted
    poses, and that is checked like any residual sweep.  damping_iter(max_iter = 2) from the same start returns the fused Hessian half at
    those poses in `hess` (the last Hessian adopted, vxba_capi_lm.hip:181), computed on the cache the fused residual half wrote, which the
    second step overwrites before the call returns and no public call exposes.  In the ONE-LANE form (VXBA_K23_PAIR=0, a child process)
    that cache is bit for bit the one read back after max_iter = 1, so the fused Hessian half's VALUES are asserted there, on (2, 33) and
    (10, 515), with the same criterion as every other Hessian.  In the lane-pair form the residual half sums a voxel's frames in another
    order: its cache differs in last bits from anything that can be read back, and only what does not depend on the cache is asserted --
    exact zeros and bitwise symmetry on (2, 33), (9, 197), (10, 197); the pair form's values stay with
    tests/test_gpu_parity.py::test_fused_launch_is_the_three_launch_iteration_to_round_off;
  * set_precision("mixed") / ("mixed_f32_clusters"): left out, tests/_sweep_cases.py says why.

Figures of a run on an MI355X: the largest |err| / (u M) -- for the decompositions / (u s) -- over the cases of a group, next to the
bound in brackets.  H: outside the rotation-rotation part of the diagonal blocks (bound 0.224), inside it (in units of u M_H, no bound
of its own), and the largest fraction of the criterion's right-hand side u (0.224 M_H + 20 M_RR + (n - 1) S_RR) reached by any element.
                                        narrow + far            wide (dense and csr)     after own residual sweep   one-lane fused half
  H   outside the rotation blocks       0.035 (0.224)           0.0581 (0.224)           0.0473 (0.224)             0.004 (0.224)
  H   rotation blocks, u M_H            0.762 (w10_v1)          0.232                    0.379                      0.004
  H   fraction of its bound             0.157                   0.26                     0.211                      0.0179
  J                                     0.823 (3.65)            1.02 (3.65)              0.76 (3.65)                --
  r of acc_evaluate2, units of u sum    1.3 (n + 1)             1.18 (n + 1)             1.43 (n + 1)               --
                                        narrow + far            wide (dense and csr)     in-launch-solve sweep
  merged                                2.98 (12.4)             3.5 (12.4)               2.86 (12.4)
  ||C u - lambda u||                    1.23 (5.86)             1.13 (5.86)              1.05 (5.86)
  |lambda - lambda*|                    1.25 (6.24)             1.1 (6.24)               1.23 (6.24)
  ||U^T U - I|| / s,  / 1               8.79 (44.2), 10.8 (54.7) 2.34, 8.77              3.76, 6.54
  r of the residual sweep               1.11 (n + 1)            1.92 (n + 1)             1.06 (n + 1)
No sweep failed a criterion: no kernel was changed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _sweep_cases as S
from tests import _sweep_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


def _csr(c):
    """The case's compressed rows; wide11's with one entry that has no points."""
    if c.name == "wide11":
        return S.csr_with_zero_entry(c.clusters, 700, 3)
    return S.dense_to_csr(c.clusters)


def _push(vx, c, store, cache=None, between=None):
    """A factor holding the case.  store: 'dense' (push_voxels) or 'csr' (push_voxels_csr).  between: called after the first of two appends
    (wide windows: a sweep there builds the incidence index, which the second append invalidates)."""
    f = vx.LidarFactor(c.W)
    cuts = (0, c.V) if between is None else (0, c.V // 3, c.V)
    rp, fr, ent = _csr(c) if store == "csr" else (None, None, None)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi == lo:
            continue
        extra = () if cache is None else tuple(x[lo:hi] for x in cache)
        if store == "csr":
            f.push_voxels_csr(rp[lo: hi + 1] - rp[lo], fr[rp[lo]: rp[hi]], ent[rp[lo]: rp[hi]], c.fix[lo:hi], c.coe[lo:hi], *extra)
        else:
            f.push_voxels(c.clusters[lo:hi], c.fix[lo:hi], c.coe[lo:hi], *extra)
        if between is not None and hi < c.V:
            between(f)
    assert f.size() == c.V
    return f


def _stores(name):
    return ("dense", "csr") if name in S.WIDE else ("dense",)


RESIDUAL = [(n, s) for n in S.CASES for s in _stores(n)]


def _check_cache(name, f, r, second, head=0, end=None, label=""):
    c = S.case(name)
    end = c.V if end is None else end
    ev, Uv, m = f.read_cache(head, end)
    S.check_merged(m, name, second=second, head=head, end=end, label=label)
    S.check_eig(m, ev, Uv, label=label)
    S.check_scalar(r, c.coe[head:end], ev[:, 0], label=label)


@pytest.mark.parametrize("name,store", RESIDUAL)
def test_residual_sweep(vx, name, store):
    c = S.case(name)
    f = _push(vx, c, store)
    assert np.array_equal(f.read_clusters()[:, :, 9], c.clusters[:, :, 9])
    r = f.evaluate_only_residual(c.poses)
    _check_cache(name, f, r, False, label=f"{name} {store} cold")
    r = f.evaluate_only_residual(c.poses2)                                   # warm-started from the decomposition just written
    _check_cache(name, f, r, True, label=f"{name} {store} warm")
    if c.V >= 7:
        head, end = c.ranges[1] if len(c.ranges) > 1 else (c.V // 3, c.V - c.V // 4)
        before = f.read_cache()
        r = f.evaluate_only_residual(c.poses, head, end)
        after = f.read_cache()
        for b, a in zip(before, after):
            assert np.array_equal(b[:head].view(np.uint64), a[:head].view(np.uint64)) and np.array_equal(b[end:].view(np.uint64), a[end:].view(np.uint64)), \
                "a residual sweep over [head, end) changed cache rows outside it"
        _check_cache(name, f, r, False, head, end, label=f"{name} {store} [{head}, {end})")
    f.close()


HESSIAN = [(n, s, k) for n in S.CASES for s in _stores(n) for k in range(1 + (n in S.WIDE) + (n == "wide11") + n.endswith("_v515"))]


@pytest.mark.parametrize("name,store,k", HESSIAN)
def test_hessian_sweep_from_the_seeded_cache(vx, name, store, k):
    c = S.case(name)
    head, end = c.ranges[k]
    cache = S.seeded_cache(name)
    # wide windows: two appends with a sweep in between (the index is built, invalidated by the second append and rebuilt)
    between = (lambda f: f.acc_evaluate2(c.poses)) if c.wide else None
    f = _push(vx, c, store, cache, between)
    H, J, r = f.acc_evaluate2(c.poses, head, end)
    S.check_hessian(H, J, r, S.reference(name, head, end), end - head, label=f"{name} {store} [{head}, {end})")
    H, J, r = f.acc_evaluate2(c.poses, 5 % c.V, 5 % c.V)
    assert not H.any() and not J.any() and r == 0.0
    f.close()


@pytest.mark.parametrize("name", S.SMALL)
def test_hessian_sweep_after_the_devices_own_residual_sweep(vx, name):
    c = S.case(name)
    f = _push(vx, c, "dense")
    f.evaluate_only_residual(c.poses)
    ev, Uv, m = f.read_cache()
    H, J, r = f.acc_evaluate2(c.poses)
    ref = R.hessian_exact(c.clusters, c.coe, c.poses, ev, Uv, m)
    S.check_hessian(H, J, r, ref, c.V, label=f"{name} after the residual sweep")
    f.close()


def _lm_start(vx, c):
    f = _push(vx, c, "dense")
    f.evaluate_only_residual(c.poses)
    f.set_option("fused_sweeps", 2)
    return f


def _one_step(vx, c, label):
    """damping_iter(max_iter = 1): the poses after one accepted step and the cache the [solve | residual sweep] launch left there, checked like
    any residual sweep's (merged_exact at those poses, live)."""
    f = _lm_start(vx, c)
    one = vx.Lidar_BA_Optimizer().damping_iter(c.poses, f, max_iter=1)
    assert one["trace"].shape[0] == 1 and one["trace"][0, 6] == 1, "the first step was not accepted"
    ev, Uv, m = f.read_cache()
    f.close()
    ex, M = R.merged_exact(c.clusters, c.fix, one["poses"])
    hi, lo = R.split_hi_lo(ex)
    assert np.array_equal(m[:, 9], hi[:, 9])
    km = R.err_units(m[:, :9], hi[:, :9], lo[:, :9], M[:, :9]).max()
    print(f"  {label}: merged {km:.3g} (bound {S.C_M:.3g})")
    assert km <= S.C_M
    S.check_eig(m, ev, Uv, label=label)
    S.check_scalar(one["resis"][1], c.coe, ev[:, 0], label=label)
    return one, (ev, Uv, m)


def _two_steps(vx, c, one):
    f = _lm_start(vx, c)
    two = vx.Lidar_BA_Optimizer().damping_iter(c.poses, f, max_iter=2)
    f.close()
    # same first step: same decision; its trial residual comes from the fused launch's residual half here
    assert two["trace"].shape[0] == 2 and np.array_equal(two["trace"][0, 6:], one["trace"][0, 6:]) and two["trace"][0, 0] == one["trace"][0, 0]
    return np.ascontiguousarray(two["hess"])


@pytest.mark.parametrize("W,V", S.FUSED)
def test_lm_step_residual_sweep_and_the_structure_of_the_fused_hessian(vx, W, V):
    """The lane-pair form (what a fused launch takes at these sizes): the in-launch-solve residual sweep's cache, and of the fused Hessian half
    what does not depend on the cache it read -- exact zeros where no term reaches, bitwise symmetry.  Its values: the one-lane test below."""
    c = S.case(f"w{W}_v{V}")
    one, cache = _one_step(vx, c, f"w{W}_v{V} in-launch-solve residual sweep")
    H = _two_steps(vx, c, one)
    M_H = R.hessian_magnitude(c.clusters, c.coe, one["poses"], *cache)[0]
    S.check_structure(H, np.zeros(6 * W), dict(M_H=M_H, M_J=np.ones(6 * W)))


ONE_LANE = ((2, 33), (10, 515))


def test_fused_hessian_half_in_the_one_lane_form():
    """VXBA_K23_PAIR=0 (read once per process: a child, started like tests/test_gpu_sweep_valu_identity.py::test_one_lane_form_of_the_fused_launch
    starts its own).  In the one-lane form the residual half of the fused launch is the stand-alone residual sweep's arithmetic statement
    for statement (csrc/vxba_k23.hpp), so the cache read back after damping_iter(max_iter = 1) is, bit for bit, the cache the fused
    launch of damping_iter(max_iter = 2) wrote and its Hessian half then read: same start, same warm start, same trial poses.  `hess` of
    the second call is checked against hessian_exact of that cache with the Hessian criterion as it stands."""
    env = dict(os.environ, VXBA_K23_PAIR="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_sweep_exact", "--check-one-lane"], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def _main(argv):
    if "--check-one-lane" not in argv:
        return 2
    assert os.environ.get("VXBA_K23_PAIR") == "0"
    from voxel_slam_amd import vxba
    vxba.load_library()
    for W, V in ONE_LANE:
        c = S.case(f"w{W}_v{V}")
        one, cache = _one_step(vxba, c, f"w{W}_v{V} one-lane, in-launch-solve residual sweep")
        H = _two_steps(vxba, c, one)
        ref = R.hessian_exact(c.clusters, c.coe, one["poses"], *cache)
        S.check_hessian(H, None, None, ref, V, label=f"w{W}_v{V} one-lane fused Hessian half")
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
