"""IMUEKF on the GPU (vxba.ImuEkf, csrc/vxba_imuekf.hip) and the front of the chain (voxel_slam_amd.front) against the numpy checker
tests/_imuekf_ref.py.  Every input is one that tests/test_imuekf_cpu.py proves honest: the checker and the g++ build of the product's header meet the
conditions imposed here without a GPU."""
import numpy as np
import pytest

from tests import _imuekf_ref as E

pytestmark = pytest.mark.gpu

CASES = E.gpu_cases()


def _handle(kw):
    from voxel_slam_amd import vxba
    return vxba.ImuEkf(vxba.ImuEkfParams.make(**E.filter_options(kw)))


def _same_result(got, scan_got, ref, K, table_got=None, table_ref=None):
    assert got["ready"] == ref["ready"] and got["heads"] == ref["heads"] and got["compensated"] == ref["compensated"]
    assert got["point0_applications"] == ref["point0_applications"]
    for a, b in zip(got["imus"], ref["imus"]):
        assert np.array_equal(a, b)
    assert (np.abs(got["state"] - ref["state"]) <= E.tol(K + 1, ref["state"])).all()
    assert (np.abs(got["cov"] - ref["cov"]) <= E.tol(K + 1, ref["cov"])).all()
    if table_got is not None:
        assert table_got.shape == table_ref.shape and np.array_equal(table_got[:, 0], table_ref[:, 0]) and (np.abs(table_got - table_ref) <= E.tol(K + 1, table_ref)).all()
    ulp = E.ulp_diff32(scan_got, ref["scan"])
    differ = int((ulp > 0).sum())
    print(f"{differ} of {ulp.size} coordinates differ from the checker, max {int(ulp.max())} ulp")
    assert ulp.max() <= 1 and differ <= 0.001 * ulp.size


@pytest.mark.parametrize("name", sorted(CASES))
def test_process_equals_the_checker(name):
    kw = CASES[name]
    K = kw["K"]
    ref = E.ImuEkfRef(**E.filter_options(kw))
    c, state, cov, want = E.run_case(ref, kw)
    table_ref = ref.pose_table()
    with _handle(kw) as g:
        c2, _, _, got = E.run_case(g, kw)
        assert got["init_num"] == ref.init_num == 31 and got["scale_gravity"] == ref.scale_gravity and got["t"] == c["end"]
        scan = g.read_scan()
        _same_result(got, scan, want, K, g.pose_table(), table_ref)
        if kw.get("point_notime"):
            assert scan.tobytes() == c["scan"][0].tobytes()
        else:
            keep = c["scan"][1].astype(np.float64) <= table_ref[0, 0]
            assert keep.sum() == kw.get("prefix", 0) and scan[keep].tobytes() == c["scan"][0][keep].tobytes()
        assert g.stats()["n"] == kw["n"]
        # the next scan: last_imu (its ORIGINAL stamp) and last_pcl_end_time carry over
        nxt = E.make_case(kw["n"], K, seed=kw["seed"] + 1000, t_end=c["end"], ties=kw["n"] >= 8)
        want2 = ref.process(want["state"], want["cov"], nxt["scan"], nxt["imus"], nxt["beg"], nxt["end"])
        got2 = g.process(want["state"], want["cov"], nxt["scan"], nxt["imus"], nxt["beg"], nxt["end"])
        assert got2["imus"][0][0] == c["end"] and np.array_equal(got2["imus"][1][0], c["imus"][1][-1])
        _same_result(got2, g.read_scan(), want2, K, g.pose_table(), ref.pose_table())


def _ready_pair(kw, **case_kw):
    """A checker and a handle with the same history and one processed scan."""
    ref = E.ImuEkfRef(**E.filter_options(kw))
    c, state, cov, want = E.run_case(ref, kw)
    g = _handle(kw)
    _, _, _, got = E.run_case(g, kw)
    return ref, g, c, want, got


def test_filter_and_device_route_are_bit_identical():
    """The filter against the checker's filter applied to the DEVICE's de-skewed cloud, including the < 500 fallback (800 points that a 3 m grid brings
    below 500); then var_init from the device pointer against var_init of the read-back cloud."""
    from voxel_slam_amd import vxba
    ref, g, c, want, got = _ready_pair(E.FILTER_CASE)
    with g:
        scan = g.read_scan()
        for size, min_points, half in E.FILTER_PASSES:
            n_f, used_half = g.filter(size, min_points)
            flt = g.filtered()
            want_f, want_half = E.filter_scan(scan, size, min_points)
            assert used_half == want_half == half and n_f == want_f.shape[0] == g.stats()["n_filtered"] and flt.tobytes() == want_f.tobytes(), (size, min_points)
            d_xyz, n_d = g.filtered_device()
            assert n_d == n_f and d_xyz.value
            ext = E.ext_default()
            a = vxba.LioEstimator(); b = vxba.LioEstimator()
            a.var_init_device(d_xyz, n_d, ext, 0.02, 0.05)
            b.var_init(flt, ext[:9].reshape(3, 3).T, ext[9:12], 0.02, 0.05)
            pa, va = a.read_points(); pb, vb = b.read_points()
            assert pa.shape[0] == n_f and pa.tobytes() == pb.tobytes() and va.tobytes() == vb.tobytes()
            a.close(); b.close()


def test_every_refusal_leaves_the_handle_as_it_was():
    """Each refused call raises, launches nothing (the stats of the last good call stand) and leaves the handle untouched: the good call behind it gives
    the bytes a handle with the same history and no refused call gives."""
    from voxel_slam_amd import vxba
    kw = E.REFUSAL_CASE
    ref, g, c, want, got = _ready_pair(kw)
    ref2, g2, _, _, _ = _ready_pair(kw)
    nxt = E.make_case(t_end=c["end"], **E.REFUSAL_NEXT)
    with g, g2:
        clean = g2.process(want["state"], want["cov"], nxt["scan"], nxt["imus"], nxt["beg"], nxt["end"])
        clean_scan = g2.read_scan()
        before = g.stats()
        nan_state = want["state"].copy(); nan_state[10] = np.nan
        nan_cov = want["cov"].copy(); nan_cov[3, 4] = np.inf
        for name, (scan, imus, beg, end) in E.bad_calls(nxt, c["end"], 0.3 * 0.1 / 5).items():
            with pytest.raises(vxba.VxbaError) as ei:
                g.process(want["state"], want["cov"], scan, imus, beg, end)
            assert ("VXBA_ERR_UNSUPPORTED" if name == "more than 64 heads" else "VXBA_ERR_ARG") in str(ei.value), name
            with pytest.raises(E.Refused):
                E.ImuEkfRef.process(_copy_of(ref), want["state"], want["cov"], scan, imus, beg, end)
            assert g.stats() == before, name
        for bad_state, bad_cov in ((nan_state, want["cov"]), (want["state"], nan_cov)):
            with pytest.raises(vxba.VxbaError):
                g.process(bad_state, bad_cov, nxt["scan"], nxt["imus"], nxt["beg"], nxt["end"])
        after = g.process(want["state"], want["cov"], nxt["scan"], nxt["imus"], nxt["beg"], nxt["end"])
        assert after["state"].tobytes() == clean["state"].tobytes() and after["cov"].tobytes() == clean["cov"].tobytes() and g.read_scan().tobytes() == clean_scan.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(after["imus"], clean["imus"])) and after["heads"] == clean["heads"]


def _copy_of(ref):
    import copy
    return copy.deepcopy(ref)


def test_reinit_and_clear():
    kw = dict(n=65, K=5, seed=41, lag=E.LAG)
    ref, g, c, want, got = _ready_pair(kw)
    with g:
        rest = E.stationary_imus(c["end"], 12, 0.005, c["end"] + 0.06, acc=(0.3, -0.1, 9.7), seed=5)
        g_new = g.reinit(rest, 1.0)
        g_ref = ref.reinit(rest, 1.0)
        assert (np.abs(g_new - g_ref) <= E.tol(12, g_ref)).all() and ref.init_num == 13 and ref.init_flag
        # init_flag is left as it is: the next call propagates, from the re-initialisation's last message
        nxt = E.make_case(65, 5, seed=42, t_end=c["end"] + 0.06)
        state = want["state"].copy(); state[21:24] = g_ref
        want2 = ref.process(state, want["cov"], nxt["scan"], nxt["imus"], c["end"], nxt["end"])
        got2 = g.process(state, want["cov"], nxt["scan"], nxt["imus"], c["end"], nxt["end"])
        assert got2["init_num"] == 13
        _same_result(got2, g.read_scan(), want2, 5)
        # clear: a new handle's state -- the same history gives the same bytes again
        g.clear()
        assert g.stats() == {"launches": 0, "waits": 0, "n": 0, "n_filtered": 0}
        _, _, _, again = E.run_case(g, kw)
        assert again["state"].tobytes() == got["state"].tobytes() and again["cov"].tobytes() == got["cov"].tobytes() and again["init_num"] == 31


def test_launches_and_waits_do_not_depend_on_n():
    kw = dict(n=257, K=5, seed=51, lag=E.LAG)
    ref, g, c, want, got = _ready_pair(kw)
    seen = {}
    with g:
        t_end, state, cov = c["end"], want["state"], want["cov"]
        for n in (3000, 257, 3000, 257):                                                   # the first call at 3000 grows the buffers (one more wait)
            nxt = E.make_case(n, 5, seed=52 + n, t_end=t_end)
            r = g.process(state, cov, nxt["scan"], nxt["imus"], nxt["beg"], nxt["end"])
            assert g.stats()["launches"] == 1
            g.filter(0.5, 0)
            seen.setdefault(n, []).append(g.stats())
            t_end, state, cov = nxt["end"], r["state"], r["cov"]
    a, b = seen[257][-1], seen[3000][-1]
    print("stats", seen)
    assert (a["launches"], a["waits"]) == (b["launches"], b["waits"]) == (4, 1)


@pytest.fixture(scope="module")
def plane_map():
    from voxel_slam_amd import synth
    return synth.make_plane_map(n_roots=800, extent=6, seed=17)


def _pose_err(a, b):
    from tests._init_ref import so3_log
    Ra, Rb = a[:9].reshape(3, 3).T, b[:9].reshape(3, 3).T
    return float(np.linalg.norm(a[9:12] - b[9:12])), float(np.linalg.norm(so3_log(Ra.T @ Rb)))


def test_odometry_front_two_consecutive_steps(plane_map):
    """OdometryFront.step on make_raw_odometry_step (800-root map, 3000 points), twice in a row, against the chain checker -> LioOracle fed the device's
    filtered cloud: match_num, iterations and ok equal, pose within 1e-7 m / 1e-7 rad, and the estimate nearer the truth than the propagated state."""
    from tests import _oracle as O
    from voxel_slam_amd import synth, vxba
    from voxel_slam_amd.front import OdometryFront
    pm = plane_map
    kw = dict(lag=E.LAG)
    ext = E.ext_default()
    ref = E.ImuEkfRef(**E.filter_options(kw))
    st, _ = E.initialise(ref, t_end=100.0, lag=E.LAG)
    with _handle(kw) as ekf:
        st_g, res = E.initialise(ekf, t_end=100.0, lag=E.LAG)
        assert np.array_equal(st_g[21:24], st[21:24]) and not any(r["ready"] for r in res)
        est = vxba.LioEstimator(pm.voxel_size, pm.max_layer); est.map_update(*pm.args())
        orc = O.LioOracle(pm.voxel_size, pm.max_layer); orc.map_update(*pm.args())
        front = OdometryFront(ekf, est, ext, down_size=0.1)
        step = synth.make_raw_odometry_step(pm, ref.last_imu, 100.0, st[21:24], scale_gravity=ref.scale_gravity, n_points=3000, K=20, ext=ext)
        state, cov = step.state_prev, step.cov
        for k in range(2):
            got = front.step(state, cov, step.scan, step.imus, step.beg_time, step.end_time)
            want = ref.process(state, cov, step.scan, step.imus, step.beg_time, step.end_time)
            assert got["ready"] and (np.abs(got["state_prop"] - want["state"]) <= E.tol(21, want["state"])).all()
            assert all(np.array_equal(a, b) for a, b in zip(got["imus"], want["imus"]))
            flt = ekf.filtered()
            assert flt.shape[0] == got["n_filtered"] and not got["half_size"] and flt.shape[0] >= 500
            orc.var_init(flt, ext[:9].reshape(3, 3).T, ext[9:12], 0.02, 0.05)
            o = orc.lio_state_estimation(want["state"], want["cov"])
            e = got["estimation"]
            assert (e["match_num"], e["iterations"], e["ok"]) == (o["match_num"], o["iterations"], o["ok"]) and got["ok"] and got["degrade_cnt"] == 0
            dp, dr = _pose_err(got["state"], o["state"])
            ep, er = _pose_err(got["state"], step.truth_end); pp, pr = _pose_err(got["state_prop"], step.truth_end)
            print(f"step {k}: vs oracle {dp:.2e} m {dr:.2e} rad; estimate off the truth {ep:.4f} m {er:.5f} rad, propagated {pp:.4f} m {pr:.5f} rad")
            assert dp < 1e-7 and dr < 1e-7
            assert ep < pp and er < pr
            assert got["pwld"].shape == (flt.shape[0], 3)
            if k == 0:                                                                     # the second scan: the motion goes on from the first one's true end
                step = synth.make_raw_odometry_step(pm, step.last_imu, step.end_time, st[21:24], scale_gravity=ref.scale_gravity, truth_prev=step.truth_end, n_points=3000,
                                                    K=20, ext=ext, seed=synth.MASTER_SEED + 977)
                state, cov = step.state_prev, got["cov"]                                   # off the truth again, so that "nearer the truth" asks something
        est.close()


def test_feed_initializer_equals_push_scan_by_hand():
    """feed_initializer on an initialisation session, behind four stationary scans' worth of IMU that initialise the handle: return codes, states and
    report are those of Initializer.push_scan called by hand with the handle's outputs."""
    from tests import _init_ref as R
    from voxel_slam_amd import vxba
    from voxel_slam_amd.front import feed_initializer
    from voxel_slam_amd.init import Initializer
    s = R.motion_session("room")
    bg, ba = s.states_gt[0, 15:18], s.states_gt[0, 18:21]
    prm = vxba.ImuEkfParams.make(cov_acc=1.0, cov_gyr=0.01, cov_bias_gyr=1e-4, cov_bias_acc=1e-4, ext=s.ext, acc_in_g=True)
    mk = lambda: Initializer(s.win_size, s.ext, s.noise_meas, s.noise_walk, imupre_scale_gravity=s.imupre_scale_gravity, **R.MOTION_MAP)
    with vxba.ImuEkf(prm) as ekf:
        # the sensor at rest before the session: 4 x 8 messages (init_num 33 > 30 at the fourth), the accelerometer in metres per second squared
        state = np.concatenate([np.eye(3).reshape(9), np.zeros(6), bg, ba, np.zeros(3)]); cov = s.covs[0]
        t0 = float(s.beg_times[0])
        for k in range(4):
            end = t0 - 0.08 * (3 - k)
            r = ekf.process(state, cov, (np.ones((1, 3), dtype=np.float32), np.zeros(1, dtype=np.float32)),
                            E.stationary_imus(end - 0.08, 8, 0.01, end - 0.001, acc=np.array([0.0, 0.0, 9.8]) + ba, gyr=bg, seed=60 + k), end - 0.08, end)
            assert not r["ready"] and r["init_num"] == 8 * (k + 1) + 1
            state = r["state"]
        assert r["scale_gravity"] == 1.0 and abs(np.linalg.norm(state[21:24]) - 9.8) < 0.1
        # the session starts from its own first pose (synth.make_init_session), with the handle's gravity
        R0 = R.so3_exp(np.array([0.05, -0.02, 0.1]))
        state = np.concatenate([R0.T.reshape(9), [0.2, -0.1, 0.05], [0.5, 0.2, -0.05], bg, ba, state[21:24]])
        a, b = mk(), mk()
        codes_a, codes_b = [], []
        for i in range(s.win_size):
            end = float(s.imus[i][0][-1])
            code, r = feed_initializer(a, ekf, state, cov, s.scans[i], s.imus[i], float(s.beg_times[i]), end)
            assert r["ready"] and r["imus"][0][0] == (t0 if i == 0 else float(s.imus[i - 1][0][-1])) and r["imus"][0][-1] == end
            codes_a.append(code)
            codes_b.append(b.push_scan(s.scans[i], r["imus"], r["state"], r["cov"], float(s.beg_times[i]), scan_odom=ekf.read_scan()))
            state, cov = a.states[-1], a.covs[-1]
        print("codes", codes_a)
        assert codes_a == codes_b and codes_a[:-1] == [0] * (s.win_size - 1) and codes_a[-1] in (1, -1)
        assert np.stack(a.states).tobytes() == np.stack(b.states).tobytes()
        ra, rb = a.report, b.report
        assert ra["flag"] == rb["flag"] and len(ra["rounds"]) == len(rb["rounds"]) and ra["eig"].tobytes() == rb["eig"].tobytes() and ra["hess"].tobytes() == rb["hess"].tobytes()
        for x, y in zip(ra["rounds"], rb["rounds"]):
            assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x), (x, y)
