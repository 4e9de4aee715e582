"""The damped solves against exact arithmetic, CPU half: the host's pivoted LDL^T (vxba_debug_host_damped_step), the numpy model of the
four-wave device solve, the honesty of the generated systems, and the proof that the acceptance criteria the device tests use
(tests/_solve_cases.py: check_dxi) reject deliberately degraded solvers.  No GPU."""
import numpy as np
import pytest
import scipy.linalg as sl

from . import _solve_cases as SC
from . import _solve_ref as R
from . import test_solve4_model as M4


@pytest.fixture(scope="module")
def vx():
    import __graft_entry__ as g
    import os
    if not os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-slam_amd", "csrc", "libvxba.so")):
        g.build()
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


def _ids(W):
    return [c["name"] for c in SC.host_cases(W)]


def _host_case_params():
    return [pytest.param(W, i, id=f"W{W}-{name}") for W in SC.HOST_WINDOWS for i, name in enumerate(_ids(W))]


# Rodrigues + the 3 x 3 product in float64: two roundings in theta^2's sum and one in the root, two per axis component, four per entry of
# K K, four in 1 + s K + c1 K K (sin and 1 - cos to an ulp), five in a row of R E whose terms sum to at most sqrt(3) in magnitude -- about
# 16 roundings of 2^-53 on numbers up to sqrt(3): 32 x 2^-53.  The ill-conditioned cases turn by thousands of radians, and the float64 angle
# theta itself carries ~2.5 roundings: the argument of sin / cos is off by 2.5 x 2^-53 theta, an entry of Exp by no more, a row of R E by
# sqrt(3) times that -- 5 theta x 2^-53 on top.
def host_rot_bound(dxi):
    theta = np.linalg.norm(np.asarray(dxi).reshape(-1, 6)[:, :3], axis=1).max()
    return (32 + 5 * theta) * R.U53


def growth_diagonal_pivoting(A):
    """|| |L| |D| |L^T| ||_2 / ||A||_2 of the elimination that pivots on the largest remaining diagonal entry (>= 1, and 1 up to rounding for a
    positive definite A).  The componentwise backward error of an LDL^T solve is bounded by a small multiple of n u |L| |D| |L^T| (Higham,
    Accuracy and Stability, 10.3 / 11.1); the multipliers of a diagonal pivot may exceed 1, so this, not the entry growth, is the factor."""
    S = np.array(A, dtype=np.float64)
    n = S.shape[0]
    left = np.arange(n)
    G = np.zeros((n, n))
    while left.size:
        k = int(np.argmax(np.abs(np.diag(S))))
        v = S[:, k].copy()
        G[np.ix_(left, left)] += np.outer(np.abs(v), np.abs(v)) / abs(S[k, k])
        keep = np.arange(left.size) != k
        S = S[np.ix_(keep, keep)] - np.outer(v[keep], v[keep]) / S[k, k]
        left = left[keep]
    return max(1.0, float(np.linalg.norm(G, 2) / np.linalg.norm(np.asarray(A, dtype=np.float64), 2)))


@pytest.mark.parametrize("W,i", _host_case_params())
def test_host_damped_step_against_exact(vx, W, i):
    """vxh::lm_damped_step on every case family.  The caller's system is NOT gauge-fixed (frame 0's rows and columns are filled in): the step
    fixes it itself.  Bound: eta <= n 2^-53, dimension x unit round-off, times the growth rho of the elimination's factors.  On a positive
    definite matrix rho = 1; picking the largest remaining DIAGONAL entry (Eigen's LDLT, the reference's solver) does not bound it on an
    indefinite one, so there rho is taken from the same elimination carried out in longdouble (growth_diagonal_pivoting)."""
    c = SC.host_cases(W)[i]
    n = 6 * W
    Hr, Jr = SC.raw_from_fixed(c["H"], c["J"], np.random.default_rng(W * 100 + i))
    got = vx.debug_host_damped_step(W, Hr, Jr, c["u"], c["Rp"])
    dxi = got["dxi"]
    assert np.all(np.isfinite(dxi)) and np.all(dxi[:6] == 0.0)
    for f in c["dead"]:
        assert np.all(dxi[6 * f:6 * f + 6] == 0.0), f"empty frame {f} moved"
    eta = SC.case_eta(c, dxi)
    rho = growth_diagonal_pivoting(SC.R.system(c["H"], c["J"], c["u"])[0]) if c["kind"] == "indef" else 1.0
    assert eta <= n * R.U53 * rho, f"eta {eta:.3e} = {eta / (n * R.U53):.3g} x n 2^-53, growth {rho:.3g}"
    if n <= 60 and c["cond"] is not None:
        xm, idx = SC._exact(W, c["name"])
        ferr, xnorm = R.forward_error(dxi[idx], xm)
        assert ferr <= c["cond"] * n * R.U53 * xnorm, f"forward error {ferr:.3e} on |x| = {xnorm:.3e}"
    # q1 at the solver's own dxi: n terms of three products and a sum -- (n + 3) roundings on the sum of magnitudes
    q1, mag = R.exact_q1(c["H"], c["J"], c["u"], dxi)
    assert abs(got["q1"] - q1) <= (n + 3) * R.U53 * mag, (got["q1"], q1)
    if n <= 60:
        rots, trans = R.exact_trial_poses(c["Rp"], dxi)
        assert np.array_equal(got["xt"][:, 9:], trans)
        assert R.rotation_error(got["xt"], rots) <= host_rot_bound(dxi)
        for f in (0,) + c["dead"]:
            assert got["xt"][f].tobytes() == c["Rp"][f].tobytes(), f"frame {f} has dxi = 0 and must keep its pose bit for bit"


def _narrow_all():
    out = []
    for W in SC.NARROW_WINDOWS:
        out += [(W, c["name"]) for c in SC.narrow_cases(W)]
        if W in SC.LI_WINDOWS:
            out.append((W, "li"))
    return out


def _get(W, name):
    return SC.li_case(W) if name == "li" else next(c for c in SC.narrow_cases(W) if c["name"] == name)


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS)
def test_model_against_exact(W):
    """The numpy model the device is compared with meets the device's own acceptance criteria on every case, LI form included, and stays
    below 0.1 of the cap on the positive definite ones (the issue's figure: 0.03 for LAPACK and the model alike)."""
    names = [nm for w, nm in _narrow_all() if w == W]
    for nm in names:
        c = _get(W, nm)
        fig = SC.check_dxi(c, SC.model_dxi(c))
        if c["kind"] != "indef":
            assert fig["eta"] <= 0.1 * fig["cap"], (nm, fig)


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS[1:])
def test_inputs_are_what_they_claim(W):
    for c in list(SC.narrow_cases(W)) + ([SC.li_case(W)] if W in SC.LI_WINDOWS else []):
        A, b, idx = R.system(c["H"], c["J"], c["u"], c.get("E"), c.get("e"), c["dead"])
        Af = A.astype(np.float64)
        assert np.array_equal(Af, Af.T)
        if idx.size == 0:
            continue
        ev = np.linalg.eigvalsh(Af)
        if c["cond"] is not None:
            # float64 eigenvalues carry n eps lambda_max: a percent of the smallest one at cond 1e13
            cond = np.abs(ev).max() / np.abs(ev).min()
            assert abs(cond / c["cond"] - 1) <= (1e-2 if c["cond"] >= 1e12 else 1e-5), (c["name"], cond)
        if c["kind"] == "indef":
            assert ev[0] < -1e-3 * ev[-1] and ev[-1] > 0
            assert np.sum(ev < 0) == max(1, idx.size // 4)
        else:
            assert ev[0] > 0, c["name"]
        if c["name"].startswith("u_"):
            assert np.linalg.cond(c["H"][6:, 6:]) == pytest.approx(1e6, rel=1e-5)
        # unpivoted elimination of the live part: no pivot anywhere near the null-pivot rule, which therefore only fires on empty frames
        S = A.copy()
        for k in range(S.shape[0]):
            assert abs(S[k, k]) > 1e-290, (c["name"], k, float(S[k, k]))
            S[k + 1:, k + 1:] -= np.outer(S[k + 1:, k], S[k + 1:, k]) / S[k, k]
        for f in c["dead"]:
            sl_ = slice(6 * f, 6 * f + 6)
            assert not c["H"][sl_, :].any() and not c["H"][:, sl_].any() and not c["J"][sl_].any()


def test_recorded_rounding_ratio():
    """K of the indefinite criterion is measured, not chosen: twice the largest ratio of eta between the rounding variants of the model.  The
    figure in the header of _solve_cases.py is the one measured when it was written."""
    ratio, where = SC.measured_rounding_ratio()
    assert 1.0 < ratio < 100.0, (ratio, where)
    assert abs(ratio / SC.RECORDED_RATIO - 1) < 0.05, (ratio, where)


def test_emulated_reciprocal_is_the_kernels():
    """rcp_device: from an estimate good to 2^-23 the cubic step lands within 2 ulp of 1 / d (the kernel's claim: 2^-69 before the final rounding)."""
    d = np.concatenate([np.random.default_rng(5).standard_normal(2000) * 10.0 ** np.random.default_rng(6).integers(-150, 150, 2000), [1e-301, 0.0, -1e-300]])
    q = SC.rcp_device(d)
    assert np.all(q[-3:] == 0.0)
    assert np.abs(q[:-3] * d[:-3].astype(np.longdouble) - 1).max() <= 2 * 2.0 ** -52


# ---- the criteria have teeth -----------------------------------------------------------------------------------------------------------
class _RcpF32(M4.Ops):
    def rcp(self, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.abs(d) > 1e-300, SC.round_rel(1.0 / d, 24), 0.0)


class _Rcp46(M4.Ops):
    def rcp(self, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.abs(d) > 1e-300, SC.round_rel(1.0 / d, 46), 0.0)


class _NoNullRule(M4.Ops):
    def rcp(self, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            return 1.0 / d


class _RhsLate(M4.Ops):
    rhs_late = True


def _skip_last(W):
    o = M4.Ops()
    o.skip_apply = (0, W - 2)      # panel 0 never taken out of the last block column
    return o


def _rejected(c, ops):
    try:
        with np.errstate(all="ignore"):      # the broken variants divide by zero on purpose
            dxi = SC.model_dxi(c, ops)
        SC.check_dxi(c, dxi)
    except AssertionError:
        return True
    return False


def _spd_like(W):
    return [c for c in SC.narrow_cases(W) if c["kind"] in ("spd", "scaled") and c["name"] != "diagonal"]


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS[1:])
def test_criteria_reject_float32_reciprocals(W):
    for c in list(SC.narrow_cases(W)) + ([SC.li_case(W)] if W in SC.LI_WINDOWS else []):
        if c["kind"] == "null" and len(c["dead"]) == W - 1:
            continue                    # nothing left to solve
        assert _rejected(c, _RcpF32()), c["name"]


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS[2:])
def test_criteria_reject_a_skipped_panel_update(W):
    for c in _spd_like(W) + [k for k in SC.narrow_cases(W) if k["kind"] == "indef"]:
        assert _rejected(c, _skip_last(W)), c["name"]


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS[2:])
def test_criteria_reject_a_late_rhs_chain(W):
    for c in _spd_like(W) + [k for k in SC.narrow_cases(W) if k["kind"] == "indef"]:
        assert _rejected(c, _RhsLate()), c["name"]


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS[1:])
def test_criteria_reject_a_division_by_a_null_pivot(W):
    nulls = [c for c in SC.narrow_cases(W) if c["kind"] == "null"]
    assert nulls
    for c in nulls:
        assert _rejected(c, _NoNullRule()), c["name"]


def test_criteria_reject_reciprocals_rounded_to_46_bits():
    """Reciprocals rounded to 46 significand bits (relative error up to 2^-47).  The criteria as a whole reject this solver, but NOT through the
    positive definite cap: measured on the CPU, its eta lies between 0.006 and 0.89 of n 2^-53 over the positive definite and scaled cases
    (the model: 0.002 to 0.034) -- the rank-one terms that carry a reciprocal's error are small against ||A|| on a log-spaced spectrum, and
    even a one-sided error of 2^-46 stays below the cap on all but a few cases.  What catches it is the model-relative criterion of the
    indefinite cases: eta 0.127 of the cap against the model's 0.018 at W = 2, 0.278 against 0.039 at W = 5 (K = 6.25).  A reciprocal error of
    this size that only showed on positive definite systems would pass the device tests; a float32 reciprocal (1e4 to 1e6 of the cap) cannot."""
    hit = [(W, c["name"]) for W in SC.NARROW_WINDOWS[1:] for c in SC.narrow_cases(W) if _rejected(c, _Rcp46())]
    assert hit, "no case rejects reciprocals rounded to 2^-46"
    assert any(nm == "indef" for _, nm in hit), hit


# ---- wide Cholesky: the reference solver is inside the cap on the same matrices ---------------------------------------------------------
@pytest.mark.parametrize("n", SC.WIDE_SIZES)
def test_lapack_cholesky_is_inside_the_wide_cap(n):
    for cond in SC.WIDE_CONDS:
        c = SC.wide_case(n, cond)
        A, b, idx = R.system(c["H"], c["J"], c["u"])
        Af = A.astype(np.float64)
        sv = np.linalg.svd(Af, compute_uv=False)
        assert abs(sv[0] / sv[-1] / cond - 1) < 1e-4
        x = sl.cho_solve(sl.cho_factor(Af, lower=True), b.astype(np.float64))
        eta = R.eta(A, b, x)
        assert eta <= n * R.U53, (n, cond, eta / (n * R.U53))
        # the raw input is the same system once frame 0 is fixed
        assert np.array_equal(c["packed_raw"].reshape(-1)[: n * n].reshape(n, n)[6:, 6:], c["packed"][: n * n].reshape(n, n)[6:, 6:])
    neg = SC.wide_negative_case()
    k = neg["k"]
    assert np.linalg.eigvalsh(neg["H"][6:k, 6:k] * 1.01).min() > 0 and neg["H"][k, k] < 0
