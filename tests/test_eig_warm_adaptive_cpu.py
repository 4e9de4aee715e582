"""The warm-started eigen-solver (vxm::eig_sym3_warm, voxel-slam_amd/csrc/vxba_math.hpp) through the host build of the lane arithmetic,
over the whole range of starts: three fixed branch-free sweeps, then the generic loop for whoever is not converged.  Starts that would be
done after one sweep (an exact basis), two (the later LM steps of a window) or three (a pose update of 1e-3), starts that need the
fallback, equal eigenvalues and bases the orthonormality test rejects must all meet the bounds tests/test_device_math_on_host.py sets for
the warm start (test_warm_start_fixed_sweeps_and_fallback).  An exit from the sweep loop as soon as the off-diagonals are negligible was
measured and not kept; these are the cases such a change has to pass."""
import numpy as np
import pytest

from tests.test_device_math_on_host import hm  # noqa: F401 -- the two host builds (exact / emulated hardware estimates), as a fixture


def _c6(M):
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def _solve(hm, M, Up):
    lam = np.zeros(3); U = np.zeros(9)
    hm.vxmh_eig_sym3_warm(_c6(M), np.ascontiguousarray(Up, dtype=np.float64).reshape(9), lam, U)
    return lam, U.reshape(3, 3)


def _check(M, lam, U, tag):
    """The bounds of test_warm_start_fixed_sweeps_and_fallback: eigenvalues against numpy.linalg.eigh, orthogonality, ||M U - U L||."""
    ref, _ = np.linalg.eigh(M)
    nrm = np.abs(M).max()
    assert np.all(np.diff(lam) >= 0), tag
    assert np.allclose(lam, ref, rtol=0, atol=2e-15 * nrm), (tag, lam - ref)
    assert np.allclose(U.T @ U, np.eye(3), atol=1e-13), tag
    assert np.allclose(M @ U, U * lam, atol=1e-13 * nrm), (tag, np.abs(M @ U - U * lam).max() / nrm)


def _planar(rng, gap=None):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    l1 = 0.07 * rng.uniform(0.5, 1.5)
    lam = np.sort(np.array([4e-4 * rng.uniform(0.2, 3), l1, l1 * (1 + gap) if gap is not None else 0.07 * rng.uniform(0.5, 1.5)]))
    M = Q @ np.diag(lam) @ Q.T
    return 0.5 * (M + M.T), Q


@pytest.mark.parametrize("exponent", list(range(1, 15)))
def test_warm_start_rotated_from_the_exact_basis(hm, exponent):  # noqa: F811
    """Starts 1e-1 .. 1e-14 rad from the exact basis."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(4100 + exponent)
    angle = 10.0 ** -exponent
    for trial in range(40):
        M, Q = _planar(rng)
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        Up = Q @ Rotation.from_rotvec(axis * angle).as_matrix()
        if trial % 2:
            Up = Up[:, rng.permutation(3)] * rng.choice([-1.0, 1.0], size=3)   # the cache keeps no order or sign
        lam, U = _solve(hm, M, Up)
        _check(M, lam, U, (angle, trial))
        assert abs(abs(U[:, 0] @ Q[:, 0]) - 1.0) < 1e-12, (angle, trial)          # the plane normal, up to sign


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-5, 1e-3, 0.3])
def test_warm_start_with_equal_eigenvalues(hm, angle):  # noqa: F811
    """Two equal eigenvalues (in-plane pair, or the smallest pair) and three: the fixed sweeps and the fallback's flush rule must neither
    stop on a matrix that is not diagonal nor loop on one that is."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(4200)
    for trial in range(60):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        kind = trial % 4
        lam_true = {0: [4e-4, 0.07, 0.07], 1: [0.02, 0.02, 0.5], 2: [0.3, 0.3, 0.3], 3: [4e-4, 0.07, 0.07 * (1 + 1e-12)]}[kind]
        M = Q @ np.diag(lam_true) @ Q.T; M = 0.5 * (M + M.T)
        Up = Q @ Rotation.from_rotvec(rng.normal(size=3) * angle).as_matrix()
        lam, U = _solve(hm, M, Up)
        _check(M, lam, U, (angle, kind))
        if kind in (0, 3):
            assert abs(abs(U[:, 0] @ Q[:, 0]) - 1.0) < 1e-12, (angle, kind)
        if kind == 1:
            assert abs(abs(U[:, 2] @ Q[:, 2]) - 1.0) < 1e-12, (angle, kind)
    lam, U = _solve(hm, np.diag([2.0, 2.0, 2.0]), np.eye(3))                      # exactly diagonal, exactly equal
    assert np.array_equal(lam, [2.0, 2.0, 2.0]) and np.allclose(U.T @ U, np.eye(3), atol=1e-15)


def test_warm_start_from_a_basis_that_is_not_orthonormal(hm):  # noqa: F811
    """A cache that was never written (zeros), a scaled basis, a sheared one, junk, NaN: the solver's orthonormality test rejects them and
    the cold start takes over (same bounds); the exact basis beside them as the control."""
    rng = np.random.default_rng(4300)
    for trial in range(60):
        M, Q = _planar(rng)
        starts = [np.zeros((3, 3)), 1.01 * Q, Q + 1e-3 * np.outer(Q[:, 0], Q[:, 1]), rng.normal(size=(3, 3)), np.full((3, 3), np.nan), Q]
        for k, Up in enumerate(starts):
            lam, U = _solve(hm, M, Up)
            _check(M, lam, U, (trial, k))
            assert abs(abs(U[:, 0] @ Q[:, 0]) - 1.0) < 1e-12, (trial, k)
