"""The odometry update on the GPU (csrc/vxba_lio.hip: lio_sweep_kernel, lio_ekf_kernel<0>, lio_var_init_kernel, lio_pvec_update_kernel) against
exact arithmetic: every case of tests/_lio_cases.py through vxba.LioEstimator, judged element by element with the criteria and the constants
recorded there (measured on CPU reference code by `python -m tests._lio_cases --calibrate`; tests/test_lio_cpu.py holds the oracle and a
list of degraded variants to the same criteria).  The mpmath work is the 4097 exact rows of the ladder, built once per module."""
import numpy as np
import pytest

from tests import _lio_cases as Cs
from tests import _lio_ref as R
from tests.test_gpu_lio import check_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


@pytest.fixture(scope="module")
def L():
    return Cs.ladder()


def device(vx, pm, pnt, var):
    g = vx.LioEstimator(pm.voxel_size, pm.max_layer); g.map_update(*pm.args()); g.set_points(pnt, var)
    return g


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("HTH", "HTz", "nnt")) and a["match_num"] == b["match_num"]


def judge(res, sw, n, label):
    assert np.array_equal(res["HTH"], res["HTH"].T)
    Cs.check_points(res, sw, n, label=label)
    Cs.check_sums(R.unpack34(res), sw, n, Cs.d_of(n), label=label)


@pytest.mark.parametrize("n", Cs.LADDER_N)
def test_sweep_ladder(vx, L, n):
    """Reset at pose A, cached at pose B, reset at pose B; each sweep with the per-point outputs and again without them, bit for bit."""
    g = device(vx, L.pm, L.pnt[:n], L.var[:n])
    assert g.scan_size() == n
    r0 = g.sweep(L.state_a, L.cov, reset_cache=True, want_points=True)
    judge(r0, L.sweep[0], n, "reset at A")
    r1 = g.sweep(L.state_b, L.cov, reset_cache=False, want_points=True)
    judge(r1, L.sweep[1], n, "cached at B")
    r2 = g.sweep(L.state_b, L.cov, reset_cache=True, want_points=True)
    judge(r2, L.sweep[2], n, "reset at B")
    # the same three again, without the per-point outputs, from the same cache states
    assert same_bits(g.sweep(L.state_a, L.cov, reset_cache=True), r0)
    assert same_bits(g.sweep(L.state_b, L.cov, reset_cache=False), r1)
    assert same_bits(g.sweep(L.state_b, L.cov, reset_cache=True), r2)


@pytest.mark.parametrize("shift", range(len(Cs.EDGE_NAMES)))
def test_gate_edges(vx, shift):
    """Rows exactly on a gate's boundary or one step from it, at lanes 0, 63, 64, 511 and 512: `<=` on the range gate, strict `<` on 3 sigma."""
    pnt, var, verdict, names = Cs.edge_scan(shift)
    g = device(vx, Cs.edge_map(), pnt, var)
    res = g.sweep(Cs.EDGE_STATE, Cs.edge_cov(), want_points=True)
    wrong = [(lane, names[lane]) for lane in Cs.EDGE_LANES if (res["plane_of_point"][lane] >= 0) != verdict[lane]]
    assert not wrong, wrong
    judge(res, Cs.edge_sweep(shift), 513, f"edges, shift {shift}")
    assert same_bits(g.sweep(Cs.EDGE_STATE, Cs.edge_cov()), res)


@pytest.mark.parametrize("shift", range(len(Cs.NOTHING)))
def test_rows_that_must_contribute_nothing(vx, L, shift):
    """NaN, +-Inf, 3e6, 1e30 in a coordinate, NaN in the variance: unmatched, as on the oracle, and the sums equal bit for bit those of the
    scan with a finite far point in that row (the lanes stay where they are); -0.0 against +0.0 likewise.  The estimation stays finite."""
    pnt, var, ps, vs, kinds = Cs.nothing_scan(shift)
    g, g2 = device(vx, L.pm, pnt, var), device(vx, L.pm, ps, vs)
    o, _ = Cs.make_pair(None, L.pm, pnt, var, gpu=False)
    for st, reset in ((L.state_a, True), (L.state_b, False)):
        a, b = g.sweep(st, L.cov, reset_cache=reset, want_points=True), g2.sweep(st, L.cov, reset_cache=reset, want_points=True)
        ro = o.sweep(st, L.cov, reset_cache=reset, want_points=True)
        assert np.array_equal(a["plane_of_point"] >= 0, ro["plane_of_point"] >= 0), kinds
        for row, kind in kinds.items():
            if kind != "-0.0":
                assert a["plane_of_point"][row] == -1 and a["sigma_of_point"][row] == 0.0, (row, kind)
        # (record indices are handed out by atomics per handle: the mask and the variances are what two handles share)
        assert same_bits(a, b) and np.array_equal(a["plane_of_point"] >= 0, b["plane_of_point"] >= 0) and np.array_equal(a["sigma_of_point"], b["sigma_of_point"]), kinds
        assert all(np.isfinite(a[k]).all() for k in ("HTH", "HTz", "nnt"))
    for ekf in (1, 0):
        g.set_option("device_ekf", ekf)
        res = g.lio_state_estimation(L.state_a, L.cov)
        assert np.isfinite(res["state"]).all() and np.isfinite(res["cov"]).all() and np.isfinite(res["min_eig"]), (ekf, kinds)


def test_node_cache_on_a_shared_face(vx):
    """A point that failed under the cache keeps its cached leaf (the reference writes `oc` on a match only): on a shared face, where
    OctoTree::inside is closed and a fresh lookup lands in the other voxel, the difference decides the verdict."""
    pm, pnt, var, st, cov, verdicts = Cs.face_case()
    g = device(vx, pm, pnt, var)
    got = tuple(bool(g.sweep(s, cov, reset_cache=(k == 0), want_points=True)["plane_of_point"][0] >= 0) for k, s in enumerate(st))
    assert got == verdicts


@pytest.mark.parametrize("device_ekf", [1, 0])
@pytest.mark.parametrize("case", Cs.EKF_CASES)
def test_state_estimation_against_the_exact_replay(vx, L, case, device_ekf):
    """The EKF replayed in mpmath from the sweeps the device itself returned: schedule equal, every state component and covariance entry
    within C_EKF_STATE / C_EKF_COV u kappa mag, min_eig as a backward error on nnt; the iteration-0 sweep against the exact sweep at the input state (the
    chain order of lio_ekf_kernel when device_ekf = 1); later sweeps against the oracle's as tests/test_gpu_lio.py compares them."""
    n, state, cov, sw = Cs.ekf_inputs(case)
    g = device(vx, L.pm, L.pnt[:n], L.var[:n])
    g.set_option("device_ekf", device_ekf)
    got = g.lio_state_estimation(state, cov)
    Cs.check_sums(R.unpack34(got["sweeps"][0]), sw, n, Cs.d_of(n, chain=bool(device_ekf)), label=f"iteration 0, {case}, device_ekf={device_ekf}")
    Cs.check_ekf(got, state, cov, label=f"{case}, device_ekf={device_ekf}")
    o, _ = Cs.make_pair(None, L.pm, L.pnt[:n], L.var[:n], gpu=False)
    ref = o.lio_state_estimation(state, cov)
    assert got["iterations"] == ref["iterations"] and got["ok"] == ref["ok"] and got["match_num"] == ref["match_num"]
    for a, b in zip(got["sweeps"][1:], ref["sweeps"][1:]):
        check_sweep(a, b, tol=1e-9)
    # bitwise repeat of the whole estimation
    again = g.lio_state_estimation(state, cov)
    assert np.array_equal(again["state"], got["state"]) and np.array_equal(again["cov"], got["cov"]) and all(same_bits(a, b) for a, b in zip(again["sweeps"], got["sweeps"]))


@pytest.mark.parametrize("n", Cs.VARINIT_N)
def test_var_init_and_pvec_update_against_mpmath(vx, n):
    """z = 0, a point on each axis, 1 cm and 200 m from the sensor, a non-trivial extrinsic; n across a wave boundary and a 256-lane block."""
    g = vx.LioEstimator()
    Cs.check_varinit(g, n, label="device")
    pnt, var = g.read_points()
    assert np.array_equal(var, np.transpose(var, (0, 2, 1))) and g.scan_size() == n
    # the raw path feeds the sweep: the points var_init left are what a sweep on an empty map walks over without a match
    assert g.sweep(*Cs.pvec_pose())["match_num"] == 0
