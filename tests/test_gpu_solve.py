"""The damped solves on the device, one system at a time, against exact arithmetic (tests/_solve_ref.py) on the matrices of
tests/_solve_cases.py: the four-wave blocked LDL^T of vxba_solve4.hpp at every window size it is instantiated for (LiDAR-only through the
production stand-alone kernel, the LiDAR-inertial form through a kernel that only calls the body), and the persistent blocked Cholesky of
the wide windows.  Every case is one workgroup on a matrix of at most 54 x 54, or one wide solve of at most 768 x 768: no scenes, no LM loops.
The acceptance criteria are SC.check_dxi; tests/test_solve_cpu.py shows on the CPU that they reject degraded solvers."""
import numpy as np
import pytest

from . import _solve_cases as SC
from . import _solve_ref as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8DEB65017E000


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    assert vxba.DEBUG_NAN_BITS == NAN_BITS
    return vxba


_runs = {}


def run(vx, c):
    """The device's answer for a case, computed once per module."""
    key = (c["W"], c["name"])
    if key not in _runs:
        if c["kind"] == "li":
            _runs[key] = vx.debug_lm_solve(c["W"], c["H"], c["J"], np.nan, None, li_rec=c["li_rec"], li_seq=4711)
        else:
            _runs[key] = vx.debug_lm_solve(c["W"], c["H"], c["J"], c["u"], c["Rp"])
    return _runs[key]


def bits(o):
    return o["dxi"].tobytes() + o["xt"].tobytes() + np.float64(o["q1"]).tobytes() + (o["li_out"].tobytes() if "li_out" in o else b"")


def check_poses(vx, c, got):
    """Trial poses at the device's own dxi: translations are one float64 addition, rotations within twice what the host-compiled
    right_multiply_exp (through vxba_debug_host_damped_step on the system I x = dxi) shows against the mpmath exponential, floor 4 x 2^-52;
    frames that do not move keep their pose bit for bit."""
    W, dxi = c["W"], got["dxi"]
    rots, trans = R.exact_trial_poses(c["Rp"], dxi)
    assert np.array_equal(got["xt"][:, 9:], trans)
    host = vx.debug_host_damped_step(W, np.eye(6 * W), -dxi, 0.0, c["Rp"])
    assert np.array_equal(host["dxi"], dxi)
    e_host, e_dev = R.rotation_error(host["xt"], rots), R.rotation_error(got["xt"], rots)
    assert e_dev <= max(2 * e_host, 4 * 2.0 ** -52), f"rotation error {e_dev:.3e}, host {e_host:.3e}"
    for f in range(W):
        if not dxi[6 * f:6 * f + 6].any():
            assert got["xt"][f].tobytes() == c["Rp"][f].tobytes(), f"frame {f} did not move and must keep its pose bit for bit"


def check_q1(c, got):
    """q1 against the exact 0.5 dxi . (u D dxi - J) at the device's dxi: n terms of three products, summed in any order -- at most n + 3
    roundings on the sum of the terms' magnitudes."""
    q1, mag = R.exact_q1(c["H"], c["J"], c["u"], got["dxi"])
    assert abs(got["q1"] - q1) <= (6 * c["W"] + 3) * R.U53 * mag, (got["q1"], q1, mag)


def _narrow_params():
    return [pytest.param(W, c["name"], id=f"W{W}-{c['name']}") for W in SC.NARROW_WINDOWS for c in SC.narrow_cases(W)]


def _case(W, name):
    return next(c for c in SC.narrow_cases(W) if c["name"] == name)


@pytest.mark.parametrize("W,name", _narrow_params())
def test_narrow_solve_against_exact(vx, W, name):
    """Positive definite, scaled and empty-frame cases: eta <= n 2^-53 on the live system, forward error within cond n 2^-53 |x|; indefinite:
    eta <= K eta_model + n 2^-53 1e-3 with K measured on the CPU (SC.indefinite_K); empty frames: dxi exactly 0, pose untouched."""
    c = _case(W, name)
    got = run(vx, c)
    assert np.all(np.isfinite(got["dxi"])) and np.all(np.isfinite(got["xt"])) and np.isfinite(got["q1"])
    SC.check_dxi(c, got["dxi"])
    check_q1(c, got)
    check_poses(vx, c, got)
    if W == 1:
        assert not got["dxi"].any() and got["xt"].tobytes() == c["Rp"].tobytes() and got["q1"] == 0.0


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS[1:])
def test_scaled_systems_give_the_same_step(vx, W):
    """H, J x 1e-140 and x 1e+140 are the same system: both answers lie within the forward bound of the exact one, hence within twice that
    of each other."""
    lo, hi = _case(W, "scaled_lo"), _case(W, "scaled_hi")
    a, b = run(vx, lo)["dxi"], run(vx, hi)["dxi"]
    assert np.linalg.norm(a - b) <= 2 * lo["cond"] * 6 * W * R.U53 * np.linalg.norm(a)


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS)
def test_narrow_solve_reads_only_its_own_fields(vx, W):
    """NaN where the solve has no business: frame 0's rows and columns of Hwork and Jwork[0:6] (the gauge rows are excluded, not solved), the
    strict upper triangle of Hwork (lanes load it, nothing consumes it), and -- in every call of this module -- every field of the LM state
    but Hwork, Jwork, ctl[c].{u, x, done}: identical bits each time."""
    c = SC.narrow_cases(W)[min(1, len(SC.narrow_cases(W)) - 1)]
    n = 6 * W
    base = bits(run(vx, c))
    H, J = c["H"].copy(), c["J"].copy()
    H[:6, :] = np.nan
    H[:, :6] = np.nan
    J[:6] = np.nan
    assert bits(vx.debug_lm_solve(W, H, J, c["u"], c["Rp"])) == base, "the gauge rows / columns are read"
    # Hwork is column-major: entry (row r, column k) at k n + r; the wrapper takes the matrix and stores it that way
    H = c["H"].copy()
    H[np.triu_indices(n, 1)] = np.nan
    assert bits(vx.debug_lm_solve(W, H, c["J"], c["u"], c["Rp"])) == base, "the strict upper triangle is consumed"


@pytest.mark.parametrize("W", SC.NARROW_WINDOWS)
def test_narrow_solve_is_deterministic_in_both_slots(vx, W):
    c = SC.narrow_cases(W)[min(1, len(SC.narrow_cases(W)) - 1)]
    base = bits(run(vx, c))
    for slot in (0, 1):
        for _ in range(3):
            assert bits(vx.debug_lm_solve(W, c["H"], c["J"], c["u"], c["Rp"], c=slot)) == base


@pytest.mark.parametrize("W", (1, 2, 5, 10))
def test_a_finished_loop_is_left_alone(vx, W):
    """done = 1: the solve returns before it writes; dxi, the trial poses and q1 still hold the sentinel they were filled with."""
    c = SC.narrow_cases(W)[0]
    for slot in (0, 1):
        got = vx.debug_lm_solve(W, c["H"], c["J"], c["u"], c["Rp"], c=slot, done=1)
        for a in (got["dxi"], got["xt"].reshape(-1), np.array([got["q1"]])):
            assert np.all(np.ascontiguousarray(a).view(np.uint64) == NAN_BITS)


@pytest.mark.parametrize("W", SC.LI_WINDOWS)
def test_li_form_against_exact(vx, W):
    """The reduced pose system of the LiDAR-inertial shells: (H + u diag(H) + E) dx = e - J with u and the poses from li_rec (ctl.u and ctl.x
    hold NaN); li_out = [dx | trial poses | seq] bit for bit what the LM state got; the rows of E above each block column are never read."""
    c = SC.li_case(W)
    n = 6 * W
    got = run(vx, c)
    SC.check_dxi(c, got["dxi"])
    lo = got["li_out"]
    assert lo[:n].tobytes() == got["dxi"].tobytes() and lo[n:n + 12 * W].tobytes() == got["xt"].tobytes() and lo[18 * W] == 4711.0
    check_poses(vx, c, got)
    E = c["E"].copy()
    for b in range(W - 1):
        E[:6 + 6 * b, 6 + 6 * b:12 + 6 * b] = np.nan       # rows above block column b
    E[:, :6] = np.nan                                       # and frame 0's columns
    rec = np.concatenate([[c["u"]], c["Rp"].reshape(-1), c["e"], E.T.reshape(-1)])
    again = vx.debug_lm_solve(W, c["H"], c["J"], np.nan, None, li_rec=rec, li_seq=4711)
    assert bits(again) == bits(got)
    for _ in range(2):
        assert bits(vx.debug_lm_solve(W, c["H"], c["J"], np.nan, None, li_rec=c["li_rec"], li_seq=4711, c=1)) == bits(got)


# ---- wide Cholesky ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.WIDE_SIZES)
@pytest.mark.parametrize("cond", SC.WIDE_CONDS)
def test_wide_cholesky_against_exact_residual(vx, n, cond):
    c = SC.wide_case(n, cond)
    got = vx.debug_wide_solve(c["packed"], n, c["u"])
    assert got["info"] == 0 and np.all(np.isfinite(got["dxi"])) and not got["dxi"][:6].any()
    A, b, idx = R.system(c["H"], c["J"], c["u"])
    eta = R.eta(A, b, got["dxi"][idx])
    assert eta <= n * R.U53, f"eta {eta:.3e} = {eta / (n * R.U53):.3g} x n 2^-53"
    q1, mag = R.exact_q1(c["H"], c["J"], c["u"], got["dxi"])
    assert abs(got["q1"] - q1) <= (n + 3) * R.U53 * mag, (got["q1"], q1)
    assert got["residual1"] == c["residual"]
    again = vx.debug_wide_solve(c["packed"], n, c["u"])
    raw = vx.debug_wide_solve(c["packed_raw"], n, c["u"])           # frame 0 not fixed by the caller: the kernel fixes it
    for o in (again, raw):
        assert o["info"] == 0 and o["dxi"].tobytes() == got["dxi"].tobytes() and o["q1"] == got["q1"] and o["residual1"] == got["residual1"]


def test_wide_cholesky_reports_a_negative_pivot(vx):
    c = SC.wide_negative_case()
    got = vx.debug_wide_solve(c["packed"], c["n"], c["u"])
    assert got["info"] > 0
    assert np.all(np.isnan(got["dxi"])) and np.isnan(got["q1"]) and np.isnan(got["residual1"]), "no output may be consumed after a failed factorisation"


def test_wide_cholesky_gives_up_and_recovers(vx):
    c = SC.wide_case(96, 1e2)
    gave_up = vx.debug_wide_solve(c["packed"], 96, c["u"], give_up=True)
    assert gave_up["info"] == -1 and np.all(np.isnan(gave_up["dxi"]))
    ok = vx.debug_wide_solve(c["packed"], 96, c["u"])
    assert ok["info"] == 0
    A, b, idx = R.system(c["H"], c["J"], c["u"])
    assert R.eta(A, b, ok["dxi"][idx]) <= 96 * R.U53
