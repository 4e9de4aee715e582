"""The odometry update against exact arithmetic, without a GPU: the cases and criteria of tests/_lio_cases.py, checked on CPU code alone.

  - the float64 restatement of the per-point terms against mpmath (this is what measures K_T and K_SIG);
  - the CPU oracle (oracle/vxo_lio.hpp) against every criterion, with the recorded constants;
  - the honesty of every input: gate, face and box margins, the share of dropped rows, the exactness of the gate-edge rows, the margins of
    the EKF schedule;
  - the exact EKF against mathematics (the normal equations, a central difference of the cost it minimises, Log o Exp);
  - degraded variants as numpy models of the kernel's data flow, each rejected by the criterion meant for it, and the record of which of
    them the older max-norm comparisons of tests/test_gpu_lio.py accept."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _lio_cases as Cs
from tests import _lio_ref as R
from tests import _oracle as O

U = R.U64


@pytest.fixture(scope="module")
def L():
    return Cs.ladder()


def test_constants_are_four_times_the_measured_ones():
    assert Cs.MARGIN == 4.0
    for c, k in ((Cs.C_T, Cs.K_T), (Cs.C_SIG, Cs.K_SIG), (Cs.C_EKF_STATE, Cs.K_EKF_STATE), (Cs.C_EKF_COV, Cs.K_EKF_COV), (Cs.C_EIG, Cs.K_EIG), (Cs.C_VI_PNT, Cs.K_VI_PNT), (Cs.C_VI_VAR, Cs.K_VI_VAR),
                 (Cs.C_PV_PNT, Cs.K_PV_PNT), (Cs.C_PV_VAR, Cs.K_PV_VAR)):
        assert c == 4.0 * k and k > 0
    assert [Cs.grid_of(n) for n in (1, 512, 513, 4096, 4097, 131072, 131073, 262145)] == [8, 8, 8, 8, 16, 256, 256, 256]
    assert Cs.d_of(1) == 1 + 13 + 7 and Cs.d_of(131073) == 2 + 13 + 255 and Cs.d_of(262145) == 3 + 13 + 255 and Cs.d_of(131073, chain=True) == 2 + 13 + 42


def test_restatement_against_mpmath_measures_the_term_constants(L):
    kt, ks = L.k_constants()
    print(f"  ladder: K_T {kt:.4g} (recorded {Cs.K_T})  K_SIG {ks:.4g} (recorded {Cs.K_SIG})")
    for sh in range(len(Cs.EDGE_NAMES)):
        s = Cs.edge_sweep(sh)
        kt, ks = max(kt, s.k_term), max(ks, s.k_sigma)
    assert 0 < kt <= Cs.SELF_CHECK * Cs.K_T and 0 < ks <= Cs.SELF_CHECK * Cs.K_SIG
    # the four parts of sigma add up to it, exactly, on exact rows
    pm = L.pm
    e = np.nonzero(L.sweep[0].flag[:64])[0]
    l = L.leaf[0][e]
    Rm, p = R.pose_of(L.state_a)
    with R.mp.workprec(R.PREC):
        x = R.point_terms(R.to_mp(L.pnt[e]), R.to_mp(L.var[e]), R.to_mp(pm.center[l]), R.to_mp(pm.normal[l]), R.to_mp(pm.plane_var[l]), R.to_mp(Rm), R.to_mp(p),
                          R.to_mp(L.cov[:3, :3]), R.to_mp(L.cov[3:6, 3:6]))
        parts = x["parts"][0] + x["parts"][1] + x["parts"][2] + x["parts"][3]
        assert max(abs(a - b) for a, b in zip(parts, x["sigma"])) < R.mpf(2) ** -150


def test_ladder_is_honest(L):
    assert L.dropped <= 0.01, L.dropped
    assert L.pnt.shape[0] == Cs.N_MASTER == max(Cs.LADDER_N) and L.index.exact_grid()
    assert L.index.grid_margin(L.wa).min() >= R.GRID_MARGIN and L.index.grid_margin(L.wb).min() >= R.GRID_MARGIN
    for k, s in enumerate(L.sweep):
        assert s.margin.min() >= R.GATE_MARGIN, (k, s.margin.min())
        # the same margins from the exact values of the first 4097 rows
        rows = np.array(sorted(s.exact_resi))
        ex = lambda d: np.array([float(d[i]) for i in rows])
        ok1, ok, marg = R.gates(ex(s.exact_resi), ex(s.exact_d2), ex(s.exact_sigma), L.pm.radius[s.leaf[rows]])
        assert marg.min() >= R.GATE_MARGIN and np.array_equal(ok, s.flag[rows]) and rows.size > 3000
    # faces, descent centres and leaf boxes (all on the grid of step voxel_size / 4) once more from exact world coordinates of rows 0..4096
    with R.mp.workprec(R.PREC):
        for st in (L.state_a, L.state_b):
            Rm, p = R.pose_of(st)
            w = R._mv(R._mat(R.to_mp(Rm)), [R.to_mp(L.pnt[:Cs.N_EXACT, k]) for k in range(3)])
            for k in range(3):
                wk = w[k] + R.mpf(float(p[k]))
                m = min(abs(x * 4 - R.mp.nint(x * 4)) / 4 / max(abs(x), 1) for x in wk)
                assert m >= R.GRID_MARGIN, (k, float(m))
    # what the second pose has to exercise among the first 513 rows
    f0, f1 = L.sweep[0].flag[:513], L.sweep[1].flag[:513]
    assert ((L.kept[:513] >= 0) & ~L.still_inside[:513]).sum() >= 5, "no point leaves its cached leaf's box"
    assert (f0 & ~f1).sum() >= 5 and (~f0 & f1).sum() >= 5
    assert np.array_equal(L.var, np.transpose(L.var, (0, 2, 1)))


def _oracle_sweeps(L, n):
    o, _ = Cs.make_pair(None, L.pm, L.pnt[:n], L.var[:n], gpu=False)
    return (o.sweep(L.state_a, L.cov, want_points=True), o.sweep(L.state_b, L.cov, reset_cache=False, want_points=True),
            o.sweep(L.state_b, L.cov, reset_cache=True, want_points=True))


@pytest.mark.parametrize("n", Cs.LADDER_N)
def test_oracle_meets_the_sweep_criteria_on_the_ladder(L, n):
    for k, ro in enumerate(_oracle_sweeps(L, n)):
        sw = L.sweep[k]
        assert np.array_equal(ro["plane_of_point"][sw.flag[:n]], sw.leaf[:n][sw.flag[:n]]), "the leaf of a matched point is not the oracle's"
        Cs.check_points(ro, sw, n, label=f"oracle sweep {k}")
        Cs.check_sums(R.unpack34(ro), sw, n, d=max(int(sw.flag[:n].sum()) - 1, 0), label=f"oracle sweep {k}")


def test_gate_edges_sit_exactly_where_they_should():
    two = R.mpf(2)
    for sh in range(len(Cs.EDGE_NAMES)):
        pnt, var, verdict, names = Cs.edge_scan(sh)
        sw = Cs.edge_sweep(sh)
        assert np.array_equal(sw.flag, verdict)
        o, _ = Cs.make_pair(None, Cs.edge_map(), pnt, var, gpu=False)
        ro = o.sweep(Cs.EDGE_STATE, Cs.edge_cov(), want_points=True)
        assert np.array_equal(ro["plane_of_point"] >= 0, verdict), "the oracle decides an edge row differently"
        Cs.check_points(ro, sw, 513)
        Cs.check_sums(R.unpack34(ro), sw, 513, d=int(verdict.sum()) - 1)
        with R.mp.workprec(R.PREC):
            for lane in Cs.EDGE_LANES:
                resi, d2, sig = sw.exact_resi[lane], sw.exact_d2[lane], sw.exact_sigma[lane]
                q = d2 - resi * resi
                nm = names[lane]
                if nm == "range_on":
                    assert q == R.mpf(2.25) == 9 * R.mpf(0.25)
                elif nm == "range_up":
                    assert q == R.mpf(2.25) + two ** -22 and float(np.nextafter(np.float32(2.25), np.float32(3))) == 2.25 + 2.0 ** -22
                else:
                    assert sig == two ** -8 and 3 * R.mp.sqrt(sig) == R.mpf(0.1875)
                    step = {"sigma_on": 0, "sigma_in": two ** -30, "sigma_in_f32": two ** -26}[nm]
                    assert abs(resi) == R.mpf(0.1875) - step
                    assert float(np.float32(0.1875 - 2.0 ** -30)) == 0.1875 and float(np.float32(0.1875 - 2.0 ** -26)) == 0.1875 - 2.0 ** -26


def test_rows_that_must_contribute_nothing_on_the_oracle(L):
    for sh in range(len(Cs.NOTHING)):
        pnt, var, ps, vs, kinds = Cs.nothing_scan(sh)
        o, _ = Cs.make_pair(None, L.pm, pnt, var, gpu=False)
        o2, _ = Cs.make_pair(None, L.pm, ps, vs, gpu=False)
        for st, reset in ((L.state_a, True), (L.state_b, False)):
            a, b = o.sweep(st, L.cov, reset_cache=reset, want_points=True), o2.sweep(st, L.cov, reset_cache=reset, want_points=True)
            for row, kind in kinds.items():
                if kind != "-0.0":
                    assert a["plane_of_point"][row] == -1, (kind, row)
            assert np.array_equal(a["plane_of_point"], b["plane_of_point"])
            assert all(np.array_equal(a[k], b[k]) for k in ("HTH", "HTz", "nnt")) and np.isfinite(a["HTH"]).all()
            # and the reference's own verdicts
            w = R.world(pnt, st)
            leaf = L.index.lookup(w)
            if reset:
                sw = R.Sweep(L.pm, pnt, var, st, L.cov, leaf)
                assert np.array_equal(sw.flag, a["plane_of_point"] >= 0)
        assert np.isfinite(o.lio_state_estimation(L.state_a, L.cov)["state"]).all()


def test_node_cache_on_a_shared_face_follows_the_reference():
    pm, pnt, var, st, cov, verdicts = Cs.face_case()
    o, _ = Cs.make_pair(None, pm, pnt, var, gpu=False)
    got = [bool(o.sweep(s, cov, reset_cache=(k == 0), want_points=True)["plane_of_point"][0] >= 0) for k, s in enumerate(st)]
    assert tuple(got) == verdicts == tuple(bool(f[0]) for f in Cs.cache_model(pm, pnt, var, st, cov))


# ---- the kernel's own per-point arithmetic, built for the host -----------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "lio_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "liblio_hostcheck.so")
    hdrs = [os.path.join(HERE, "..", "voxel-slam_amd", "csrc", h) for h in ("vxba_lio_math.hpp", "vxba_lio_ctl.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    lib = C.CDLL(so)
    lib.lioh_points.argtypes = [C.c_longlong, f64p, f64p, i32p, f64p, C.c_double, i64p, i32p, i32p, f64p, f64p]
    lib.lioh_scatter.argtypes = [i32p, i32p]
    return lib


def _host_points(hm, pm, pnt, var, leaf, state, cov):
    """The header's voxel_index and plane_test over the points, each against the record of leaf[i] (laid out as lio_map_update_kernel does)."""
    n = pnt.shape[0]
    l = np.maximum(leaf, 0)
    rec = np.zeros((n, 32))
    rec[:, 0:3], rec[:, 3:6] = pm.center[l], pm.normal[l]
    rec[:, 6], rec[:, 7], rec[:, 8:11] = pm.radius[l].astype(np.float32), pm.box_half[l], pm.box_center[l]
    P = pm.plane_var[l]
    for k, (r, c) in enumerate(R.TRI6):
        rec[:, 11 + k] = 0.5 * (P[:, c, r] + P[:, r, c])
    pts = np.ascontiguousarray(np.concatenate([pnt, np.stack([var[:, r, c] for r, c in R.TRI3], axis=1)], axis=1))
    cov = np.asarray(cov)
    arg = np.ascontiguousarray(np.concatenate([state[:12], cov[:3, :3].T.reshape(9), cov[3:6, 3:6].T.reshape(9)]))
    loc = np.zeros((n, 3), dtype=np.int64); packed = np.zeros(n, dtype=np.int32); flag = np.zeros(n, dtype=np.int32)
    sigma, resi = np.zeros(n), np.zeros(n)
    hm.lioh_points(n, pts, np.ascontiguousarray(rec), np.ascontiguousarray((leaf >= 0).astype(np.int32)), arg, pm.voxel_size, loc, packed, flag, sigma, resi)
    return loc, packed.astype(bool), flag.astype(bool), sigma, resi


def test_kernel_arithmetic_on_the_host(L, hm):
    """csrc/vxba_lio_math.hpp through g++ -ffp-contract=off: the ladder's first 513 rows in its three sweeps and the gate-edge scans."""
    runs = [(L.pm, L.pnt[:513], L.var[:513], L.leaf[k][:513], st, L.cov, L.sweep[k]) for k, st in enumerate((L.state_a, L.state_b, L.state_b))]
    for sh in range(len(Cs.EDGE_NAMES)):
        pnt, var, verdict, names = Cs.edge_scan(sh)
        es = Cs.edge_sweep(sh)
        runs.append((Cs.edge_map(), pnt, var, es.leaf, Cs.EDGE_STATE, Cs.edge_cov(), es))
    for pm, pnt, var, leaf, st, cov, sw in runs:
        loc, packed, flag, sigma, resi = _host_points(hm, pm, pnt, var, leaf, st, cov)
        ref_loc, ok = R.MapIndex(pm).voxel_index(R.world(pnt, st))
        assert np.array_equal(packed, ok) and np.array_equal(loc[ok], ref_loc[ok])
        k = Cs.check_points(dict(plane_of_point=np.where(flag, leaf, -1), sigma_of_point=sigma), sw, 513, label="vxba_lio_math.hpp on the host")
        t = leaf >= 0
        assert np.all(np.abs(resi[t] - sw.resi[:513][t]) <= 8 * U * (np.abs(pnt[t]).sum(axis=1) + np.abs(st[9:12]).sum() + np.abs(pm.center[leaf[t]]).sum(axis=1)))
    # the special rows: every one rejected before or by the leaf test
    for sh in range(len(Cs.NOTHING)):
        pnt, var, ps, vs, kinds = Cs.nothing_scan(sh)
        with np.errstate(invalid="ignore", over="ignore"):
            leaf = np.where(np.isfinite(pnt).all(axis=1), L.index.lookup(R.world(np.nan_to_num(pnt, posinf=1e30, neginf=-1e30), L.state_a)), L.leaf[0][:513])
        loc, packed, flag, sigma, resi = _host_points(hm, L.pm, pnt, var, leaf, L.state_a, L.cov)
        for row, kind in kinds.items():
            if kind != "-0.0":
                assert not flag[row] and sigma[row] == 0.0, (row, kind)
            if kind in ("+inf", "-inf", "3e6", "1e30"):
                assert not packed[row], (row, kind)
    col, real = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32)
    hm.lioh_scatter(col, real)
    assert sorted(col[real >= 1].tolist()) == list(range(34)) and (real >= 1).sum() == 34


# ---- EKF ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ekf_runs():
    return {case: Cs.oracle_ekf(case) for case in Cs.EKF_CASES}


@pytest.mark.parametrize("case", Cs.EKF_CASES)
def test_oracle_and_host_algebra_meet_the_ekf_criterion(L, ekf_runs, case):
    got, state, cov = ekf_runs[case]
    self_check = tuple(Cs.SELF_CHECK * k for k in (Cs.K_EKF_STATE, Cs.K_EKF_COV, Cs.K_EIG))
    ks, kc, ke, ex = Cs.check_ekf(got, state, cov, *self_check, label=f"oracle {case}")
    assert float(ex["margin"]) >= Cs.SCHEDULE_MARGIN                       # every convergence / rematch decision and Log / Exp branch
    h = R.ekf_f64(state, cov, got["sweeps"])
    h.update(min_eig=got["min_eig"], ok=got["ok"], match_num=got["match_num"], sweeps=got["sweeps"])
    Cs.check_ekf(h, state, cov, *self_check, label=f"host algebra {case}")
    gj = R.ekf_f64(state, cov, got["sweeps"], inverse=R.gauss_jordan)
    gj.update(min_eig=got["min_eig"], ok=got["ok"], match_num=got["match_num"], sweeps=got["sweeps"])
    Cs.check_ekf(gj, state, cov, label=f"Gauss-Jordan order {case}")
    # the iteration-0 sweep of the oracle against the exact sweep at the input state
    n, _, _, sw = Cs.ekf_inputs(case)
    Cs.check_sums(R.unpack34(got["sweeps"][0]), sw, n, d=int(sw.flag[:n].sum()) - 1)


def test_exact_ekf_against_mathematics(ekf_runs):
    mp, mpf = R.mp, R.mpf
    got, state, cov = ekf_runs[(4097, "mixed")]
    with mp.workprec(R.PREC):
        ex = R.ekf_exact(state, cov, got["sweeps"])
        C = mp.matrix([[mpf(float(v)) for v in row] for row in cov])
        Cinv = C ** -1
        for it, sw in enumerate(got["sweeps"]):
            H = mp.zeros(15, 15); z = mp.zeros(15, 1)
            for r in range(6):
                z[r] = mpf(float(sw["HTz"][r]))
                for c in range(6):
                    H[r, c] = mpf(float(sw["HTH"][r, c]))
            sol, vec = ex["sol"][it], ex["vec"][it]
            # normal equations: (cov^-1 + HTH) sol = HTz + cov^-1 vec
            res = (Cinv + H) * sol - (z + Cinv * vec)
            assert max(abs(v) for v in res) <= mpf(2) ** -120 * max(abs(v) for v in z)
            # sol minimises  1/2 d^T HTH d - HTz^T d + 1/2 (d - vec)^T cov^-1 (d - vec): central differences of the cost vanish
            cost = lambda d: ((d.T * H * d)[0] / 2 - (z.T * d)[0] + ((d - vec).T * Cinv * (d - vec))[0] / 2)
            scale = abs(cost(sol)) + 1
            for i in range(15):
                h = mp.zeros(15, 1); h[i] = abs(sol[i]) * mpf(2) ** -60 + mpf(2) ** -90
                g = (cost(sol + h) - cost(sol - h)) / (2 * h[i])
                assert abs(g) * abs(h[i]) <= mpf(2) ** -100 * scale, (it, i)
        # (I - G) cov = K cov^-1 cov = K: the updated covariance is the last K itself
        K = ex["K"][-1]
        dev = max(abs(mpf(float(ex["cov"][r, c])) + mpf(float(ex["cov_lo"][r, c])) - K[r, c]) / mp.sqrt(K[r, r] * K[c, c]) for r in range(15) for c in range(15))
        assert dev <= mpf(2) ** -95
        # Log o Exp on the exact branches
        for w in ([0.3, -0.2, 0.1], [2e-3, 1e-3, -2e-3]):
            Rw = R._mp_exp([mpf(x) for x in w])
            back, _, _ = R._mp_log(Rw)
            assert max(abs(a - mpf(b)) for a, b in zip(back, w)) <= mpf(2) ** -150
    # the smallest eigenvalue: (nnt - lambda I) singular
    nn = np.array(got["sweeps"][-1]["nnt"])
    assert abs(np.linalg.det(nn - float(ex["min_eig"]) * np.eye(3))) <= 1e-9 * np.linalg.norm(nn) ** 3


@pytest.mark.parametrize("n", Cs.VARINIT_N)
def test_oracle_var_init_and_pvec_update_against_mpmath(n):
    xyz = Cs.varinit_scan(n)
    if n >= 6:
        assert (xyz[:, 2] == 0).sum() >= 3 and np.any(np.linalg.norm(xyz, axis=1) < 0.011) and np.any(np.linalg.norm(xyz, axis=1) > 199)
    Cs.check_varinit(O.LioOracle(), n, consts=tuple(Cs.SELF_CHECK * k for k in (Cs.K_VI_PNT, Cs.K_VI_VAR, Cs.K_PV_PNT, Cs.K_PV_VAR)), label="oracle")


# ---- degraded variants ------------------------------------------------------------------------------------------------------------------------
def _masked(sw, rows):
    """A copy of a reference sweep in which `rows` are unmatched."""
    m = copy.copy(sw)
    m.flag, m.terms, m.mags, m.terms_hi, m.terms_lo = (a.copy() for a in (sw.flag, sw.terms, sw.mags, sw.terms_hi, sw.terms_lo))
    m.flag[rows] = False
    for a in (m.terms, m.mags, m.terms_hi, m.terms_lo):
        a[rows] = 0.0
    m._sums = {}
    return m


def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()
    return True


def test_degraded_variants_are_rejected_and_the_old_tolerances_accept_some(L, ekf_runs):
    accepted_by_old = {}
    sw = L.sweep[0]
    n = 131073
    ref34 = lambda s, m: Cs.pack34(s.sums(m)[0])

    def sweep_variant(name, sums, ref_sw, m, chain=False):
        assert _rejected(lambda: Cs.check_sums(sums, ref_sw, m, Cs.d_of(m, chain))), name
        accepted_by_old[name] = Cs.old_check_sweep(Cs.pack34(sums), ref34(ref_sw, m))

    # the model itself, undegraded, meets the criterion on both summation paths and at every ladder size
    for m in Cs.LADDER_N:
        Cs.check_sums(Cs.device_sums(sw.terms, m), sw, m, Cs.d_of(m), label="model, host sum")
        Cs.check_sums(Cs.device_sums(sw.terms, m, chain=True), sw, m, Cs.d_of(m, True))
    # 1. workgroup 100 holds a single matched point of the 131 073 and its partial is dropped
    rows = np.arange(100 * 512, 101 * 512)
    one = rows[np.nonzero(sw.flag[rows])[0][0]]
    lone = _masked(sw, rows[rows != one])
    Cs.check_sums(Cs.device_sums(lone.terms, n), lone, n, Cs.d_of(n))
    sums = Cs.device_sums(lone.terms, n, variant=("drop_partial", 100))
    assert _rejected(lambda: Cs.check_sums(sums, lone, n, Cs.d_of(n)))
    s1 = sums.copy(); s1[33] += 1            # even with the count put right the other 33 sums give it away
    sweep_variant("dropped partial", s1, lone, n)
    # 2. a butterfly loses lane 63's share (workgroup 3, wave 5)
    r63 = 3 * 512 + 5 * 64 + 63
    assert sw.flag[r63]
    s2 = Cs.device_sums(sw.terms, n, variant=("lane63", 3, 5)); s2[33] = sw.sums(n)[0][33]
    sweep_variant("butterfly loses lane 63", s2, sw, n)
    # 3. the second pass of a lane is skipped
    m3 = 262145
    s3 = Cs.device_sums(sw.terms, m3, variant="skip_pass2")
    assert _rejected(lambda: Cs.check_sums(s3, sw, m3, Cs.d_of(m3)))
    # ... which tests/test_gpu_lio.py cannot see: at its largest scan, 100 000 points, no lane runs a second pass
    accepted_by_old["second pass skipped"] = Cs.old_check_sweep(Cs.pack34(Cs.device_sums(sw.terms, 100000, variant="skip_pass2")), ref34(sw, 100000))
    # 4. R_inv formed in float32
    t4 = sw.terms.copy()
    t4[:, :27] *= (sw.R_inv.astype(np.float32).astype(np.float64) / sw.R_inv)[:, None]
    sweep_variant("R_inv in float32", Cs.device_sums(t4, n), sw, n)
    # 5. sigma without the factor 2 on the off-diagonal of plane_var
    e = np.nonzero(sw.flag[:513])[0]
    l = sw.leaf[e]
    Rm, p = R.pose_of(L.state_a)
    d = L.pnt[e] @ Rm.T + p - L.pm.center[l]
    J = np.concatenate([d, -L.pm.normal[l]], axis=1)
    off = sum(L.pm.plane_var[l][:, r, c] * J[:, r] * J[:, c] for r in range(6) for c in range(r + 1, 6))
    res5 = dict(plane_of_point=np.where(sw.flag[:513], sw.leaf[:513], -1), sigma_of_point=sw.sigma[:513].copy())
    Cs.check_points(res5, sw, 513)
    res5["sigma_of_point"][e] -= off
    assert _rejected(lambda: Cs.check_points(res5, sw, 513))
    # 6. `<=` and `<` exchanged on either gate, at the edge rows
    es = Cs.edge_sweep(0)
    t = np.nonzero(es.leaf >= 0)[0]
    for which in ("range", "sigma"):
        _, ok, _ = R.gates(es.resi[t], es.d2[t], es.sigma_all[t], Cs.edge_map().radius[es.leaf[t]], swap=which)
        res6 = dict(plane_of_point=np.where(ok, 0, -1), sigma_of_point=np.where(ok, es.sigma_all[t], 0.0))
        assert _rejected(lambda: Cs.check_points(res6, es, 513)), which
        # ... while on a scan without edge rows (every scan of tests/test_gpu_lio.py) the exchanged comparison decides every row as before
        tt = np.nonzero(sw.leaf[:4097] >= 0)[0]
        _, ok, _ = R.gates(sw.resi[tt], sw.d2[tt], sw.sigma_all[tt], L.pm.radius[sw.leaf[tt]], swap=which)
        same = np.array_equal(ok, sw.flag[tt])
        accepted_by_old[f"{which} gate comparison exchanged"] = same and Cs.old_check_sweep(ref34(sw, 4097), ref34(sw, 4097))
    # 7. the cache overwritten with -1 for a point that failed under use_cache
    pm, pnt, var, st, cov, verdicts = Cs.face_case()
    assert tuple(bool(f[0]) for f in Cs.cache_model(pm, pnt, var, st, cov, overwrite=True)) != verdicts
    # ... while on a scan whose points keep off the faces a fresh lookup finds the leaf the cache held: nothing to see for the older test
    sts = [L.state_a, L.state_b, L.state_a]
    a, b = Cs.cache_model(L.pm, L.pnt[:4097], L.var[:4097], sts, L.cov), Cs.cache_model(L.pm, L.pnt[:4097], L.var[:4097], sts, L.cov, overwrite=True)
    accepted_by_old["cache overwritten with -1"] = all(np.array_equal(x, y) for x, y in zip(a, b))
    # 8. the chain sum stops at slot 252
    s8 = Cs.device_sums(sw.terms, n, chain=True, variant=("chain_stop", 252)); s8[33] = sw.sums(n)[0][33]
    sweep_variant("chain sum stops at slot 252", s8, sw, n, chain=True)
    # 9..11. the EKF algebra
    for case in Cs.EKF_CASES:
        got, state, cov = ekf_runs[case]
        ex = R.ekf_exact(state, cov, got["sweeps"])
        ref = dict(state=ex["state"], cov=ex["cov"])
        for variant in ("f32S", "gcols", "inplace"):
            h = R.ekf_f64(state, cov, got["sweeps"], variant=variant)
            h.update(min_eig=got["min_eig"], ok=got["ok"], match_num=got["match_num"], sweeps=got["sweeps"])
            assert _rejected(lambda: Cs.check_ekf(h, state, cov)), (case, variant)
            accepted_by_old[f"{variant} {case}"] = Cs.old_check_state(h, ref)
    took = sorted(k for k, v in accepted_by_old.items() if v)
    print("  accepted by check_sweep at 1e-10 / 1e-7 or by the state / covariance tolerances of test_state_estimation_matches_oracle:")
    for k in took:
        print(f"    {k}")
    print("  rejected by them too:", sorted(k for k, v in accepted_by_old.items() if not v))
    assert len(took) >= 2, took
    # what the record says: the older comparisons accept only the variants that need inputs they never had (an exchanged comparison without a row
    # on the boundary, the cache overwrite without a point on a face, the skipped pass below 131 073 points); every arithmetic variant -- also the
    # inverse on S rounded to float32 -- they reject on these cases as well
    assert not any(v for k, v in accepted_by_old.items() if k.split()[0] in ("f32S", "gcols", "inplace", "R_inv", "butterfly", "chain", "dropped"))
