"""vxba_intake_* and vxba_imuekf_process_device on the GPU against tests/_intake_ref.py: every case of tests/_intake_cases.py bit for bit -- every
operation of the intake is exactly specified, so there is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

from tests import _imuekf_ref as E
from tests import _intake_cases as IC
from tests import _intake_ref as R

pytestmark = pytest.mark.gpu

CASES = IC.cases()


@pytest.fixture(scope="module")
def intake():
    from voxel_slam_amd import vxba
    with vxba.ScanIntake() as h:
        yield h


def _push(h, name):
    c = CASES[name]
    return h.push(c["layout"], c["data"], c["pfn"], c["blind"], IC.time_head(name))


def _device_copy(h):
    """The resident cloud read through the device pointers of vxba_intake_device (the push has waited for its stream)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    px, pt, n = h.device()
    xyz, toff = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    assert hip.hipMemcpy(xyz.ctypes.data, px, xyz.nbytes, 2) == 0 and hip.hipMemcpy(toff.ctypes.data, pt, toff.nbytes, 2) == 0
    return xyz, toff


def _same_cloud(h, rec, ref):
    assert rec["record"].tobytes() == ref["record"].tobytes(), (rec["record"], ref["record"])
    xyz, toff = h.read()
    assert xyz.tobytes() == ref["xyz"].tobytes() and toff.tobytes() == ref["toff"].tobytes()
    dx, dt = _device_copy(h)
    assert dx.tobytes() == xyz.tobytes() and dt.tobytes() == toff.tobytes()
    assert h.stats()["n"] == ref["xyz"].shape[0] == rec["n_out"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_push_equals_the_checker(intake, name):
    from voxel_slam_amd import vxba
    c, ref = CASES[name], IC.reference(name)
    if c["expect"] == "ok":
        _same_cloud(intake, _push(intake, name), ref)
        assert intake.stats()["launches"] == 2
        return
    before_ref = IC.reference("grid-livox19-n65-f3")
    _push(intake, "grid-livox19-n65-f3")
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_UNSUPPORTED" if c["expect"] == "unsupported" else "VXBA_ERR_ARG"):
        _push(intake, name)
    if c["expect"] == "all_trimmed":                   # reported after the run: the record is written, the handle holds no cloud
        assert intake.last_record.tobytes() == ref["record"].tobytes() and intake.stats()["n"] == 0 and intake.device()[2] == 0
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_STATE"):
            intake.read()
    else:                                              # nothing launched, the previous result still readable
        assert not intake.last_record.any() and intake.stats()["launches"] == 2
        xyz, toff = intake.read()
        assert xyz.tobytes() == before_ref["xyz"].tobytes() and toff.tobytes() == before_ref["toff"].tobytes()


def test_every_refusal_leaves_the_previous_result_readable(intake):
    from voxel_slam_amd import front, vxba
    S = vxba.ScanLayout
    good = "grid-velodyne22-n257-f3"
    ref = IC.reference(good)
    _same_cloud(intake, _push(intake, good), ref)
    c = CASES[good]
    stats = intake.stats()
    assert (stats["launches"], stats["n"], stats["n_decoded"]) == (2, ref["xyz"].shape[0], 257)
    hes = CASES["grid-hesai23-n64-f1"]
    bad = {
        "point_filter_num 0": (c["layout"], c["data"], 0, 1.0, 0.0),
        "point_filter_num -3": (c["layout"], c["data"], -3, 1.0, 0.0),
        "point_step smaller than the time field's end": (S(21, 0, 4, 8, 18, S.TIME_F32, S.RULE_AS_IS, 1), c["data"][:21 * 100], 1, 1.0, 0.0),
        "point_step smaller than z's end": (S(13, 0, 4, 10, 0, S.TIME_NONE, S.RULE_NONE, 0), c["data"][:13 * 100], 1, 1.0, 0.0),
        "point_step below 12": (S(11, 0, 4, 7, 0, S.TIME_NONE, S.RULE_NONE, 0), c["data"][:11 * 100], 1, 1.0, 0.0),
        "point_step above the limit": (S(S.MAX_STEP + 1, 0, 4, 8, 12, S.TIME_F32, S.RULE_AS_IS, 1), c["data"][:(S.MAX_STEP + 1) * 10], 1, 1.0, 0.0),
        "x overlaps y": (S(22, 0, 2, 8, 18, S.TIME_F32, S.RULE_AS_IS, 1), c["data"], 1, 1.0, 0.0),
        "time overlaps z": (S(22, 0, 4, 8, 10, S.TIME_F32, S.RULE_AS_IS, 1), c["data"], 1, 1.0, 0.0),
        "f64 time overlaps x": (S(23, 16, 5, 9, 12, S.TIME_F64, S.RULE_MINUS_HEAD, 1), hes["data"], 1, 1.0, 0.0),
        "a negative offset": (S(22, -1, 4, 8, 18, S.TIME_F32, S.RULE_AS_IS, 1), c["data"], 1, 1.0, 0.0),
        "u32 time as is": (S(22, 0, 4, 8, 18, S.TIME_U32, S.RULE_AS_IS, 1), c["data"], 1, 1.0, 0.0),
        "no time field under nanoseconds": (S(22, 0, 4, 8, 18, S.TIME_NONE, S.RULE_NANOSECONDS, 1), c["data"], 1, 1.0, 0.0),
        "filter 2": (S(22, 0, 4, 8, 18, S.TIME_F32, S.RULE_AS_IS, 2), c["data"], 1, 1.0, 0.0),
        "an empty message minus head": (hes["layout"], b"", 1, 1.0, 0.0),
        "blind NaN": (c["layout"], c["data"], 1, float("nan"), 0.0),
        "time_head inf": (hes["layout"], hes["data"], 1, 1.0, float("inf")),
    }
    for why, (lay, data, pfn, blind, head) in bad.items():
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            intake.push(lay, data, pfn, blind, head)
        assert not intake.last_record.any() and intake.stats() == stats, why
    # n_points >= 2^31: through the C entry point, which turns it away before it looks at the bytes
    rec = np.zeros(6)
    buf = np.frombuffer(c["data"], dtype=np.uint8)
    assert intake._L.vxba_intake_push(intake._h, C.byref(c["layout"]), 2 ** 31, buf.ctypes.data_as(C.c_void_p), 1, 1.0, 0.0, rec) == 1
    assert intake._L.vxba_intake_push(intake._h, C.byref(c["layout"]), -1, buf.ctypes.data_as(C.c_void_p), 1, 1.0, 0.0, rec) == 1
    assert intake._L.vxba_intake_push(intake._h, C.byref(c["layout"]), 257, None, 1, 1.0, 0.0, rec) == 1 and not rec.any()
    xyz, toff = intake.read()
    assert xyz.tobytes() == ref["xyz"].tobytes() and toff.tobytes() == ref["toff"].tobytes()
    dx, dt = _device_copy(intake)
    assert dx.tobytes() == xyz.tobytes() and dt.tobytes() == toff.tobytes()
    # front.ScanIntake turns an empty Hesai message away itself (it would have to read point 0)
    f = front.ScanIntake(front.HESAI, hes["layout"])
    with pytest.raises(vxba.VxbaError):
        f.push(b"", 1.0)
    f.close()


def test_growth_and_reuse():
    """One handle pushed with 4099, then 1, then 4099 points: the buffers grow once (one more wait), are reused, and every cloud is the checker's."""
    from voxel_slam_amd import vxba
    waits = []
    with vxba.ScanIntake() as h:
        for name in ("grid-ouster48-n4099-f1", "grid-ouster48-n1-f1", "grid-ouster48-n4099-f3", "grid-livox19-n4099-f1", "grid-hesai23-n1-f1"):
            _same_cloud(h, _push(h, name), IC.reference(name))
            waits.append(h.stats()["waits"])
    assert waits == [2, 1, 1, 1, 1]


def test_launches_and_waits_do_not_depend_on_n():
    from voxel_slam_amd import vxba
    seen = {}
    with vxba.ScanIntake() as h:
        _push(h, "grid-ouster48-n4099-f1")                                  # the largest message first: no growth afterwards
        for kind in ("livox19", "velodyne22", "ouster48", "tartanair16"):
            for n in IC.SIZES:
                name = f"grid-{kind}-n{n}" + ("" if kind == "tartanair16" else "-f1")
                _push(h, name)
                s = h.stats()
                seen[name] = (s["launches"], s["waits"])
    print("stats", sorted(set(seen.values())))
    assert set(seen.values()) == {(2, 1)}, seen


def _ekf(kw):
    from voxel_slam_amd import vxba
    return vxba.ImuEkf(vxba.ImuEkfParams.make(**E.filter_options(kw)))


def _message_of(scan, kind, seed=0):
    """A scan's arrays as a driver message of KINDS[kind], and the checker's decode of it."""
    from voxel_slam_amd import synth
    lidar, lay = IC.KINDS[kind]
    data = synth.make_driver_message(scan[0], synth.raw_times(scan[1], lay, IC.HEAD), lay, seed=seed)
    return lidar, lay, data


def test_process_device_equals_process_on_the_read_back_arrays(intake):
    from voxel_slam_amd import vxba
    kw = dict(n=257, K=5, seed=51, lag=E.LAG)
    a, b = _ekf(kw), _ekf(kw)
    with a, b:
        c, _, _, got_a = E.run_case(a, kw)
        _, _, _, got_b = E.run_case(b, kw)
        assert got_a["ready"] and got_a["state"].tobytes() == got_b["state"].tobytes()
        state, cov, t_end = got_a["state"], got_a["cov"], c["end"]
        for n, kind in ((1025, "ouster48"), (63, "livox19"), (4099, "hesai23")):
            nxt = E.make_case(n, 5, seed=70 + n, t_end=t_end, ties=True)
            lidar, lay, data = _message_of(nxt["scan"], kind, seed=n)
            want = R.process(data, lay, lidar, 1, 36.0, nxt["beg"])
            head = want["time_head"]
            _same_cloud(intake, intake.push(lay, data, 1, 36.0, head), want)
            arrays = intake.read()
            assert 1 < arrays[0].shape[0] < n                                    # the blind test took some
            ra = a.process(state, cov, arrays, nxt["imus"], nxt["beg"], nxt["end"])
            rb = b.process_device(state, cov, intake, nxt["imus"], nxt["beg"], nxt["end"])
            assert ra["ready"] and rb["ready"] and rb["compensated"] == -1 and ra["compensated"] >= 0
            for k in ("state", "cov"):
                assert ra[k].tobytes() == rb[k].tobytes()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ra["imus"], rb["imus"]))
            assert (ra["heads"], ra["point0_applications"], ra["t"]) == (rb["heads"], rb["point0_applications"], rb["t"])
            assert a.read_scan().tobytes() == b.read_scan().tobytes() and a.pose_table().tobytes() == b.pose_table().tobytes()
            assert (b.stats()["launches"], b.stats()["n"]) == (1, arrays[0].shape[0])
            state, cov, t_end = ra["state"], ra["cov"], nxt["end"]
    # a handle that is not initialised does not look at the scan, on either route
    a, b = _ekf(kw), _ekf(kw)
    with a, b:
        st = np.concatenate([np.eye(3).reshape(9), np.zeros(15)])
        imus = E.stationary_imus(99.9, 10, 0.01, 100.0 - E.LAG)
        ra = a.process(st, np.eye(15) * 1e-4, intake.read(), imus, 99.9, 100.0)
        rb = b.process_device(st, np.eye(15) * 1e-4, intake, imus, 99.9, 100.0)
        assert not ra["ready"] and not rb["ready"] and ra["state"].tobytes() == rb["state"].tobytes() and ra["init_num"] == rb["init_num"] == 11
        assert rb["imus"] is None and b.stats()["launches"] == 0
    # a ready handle and an intake without a cloud: the empty scan
    c = _ekf(kw)
    with c, vxba.ScanIntake() as empty:
        cc, _, _, got = E.run_case(c, kw)
        nxt = E.make_case(10, 5, seed=3, t_end=cc["end"])
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            c.process_device(got["state"], got["cov"], empty, nxt["imus"], nxt["beg"], nxt["end"])


def test_step_message_equals_step_on_the_decoded_arrays():
    """A short stream of make_raw_odometry_step scans packed by make_driver_message, paired with their IMU messages by PackageSync: step_message (the
    scan crosses the bus once, as bytes) and step on the checker's decode of the same bytes give the same bytes."""
    from voxel_slam_amd import front, synth, vxba
    pm = synth.make_plane_map(n_roots=800, extent=6, seed=17)
    kw = dict(lag=E.LAG)
    ext = E.ext_default()
    ref = E.ImuEkfRef(**E.filter_options(kw))
    st, _ = E.initialise(ref, t_end=100.0, lag=E.LAG)
    steps = [synth.make_raw_odometry_step(pm, ref.last_imu, 100.0, st[21:24], scale_gravity=ref.scale_gravity, n_points=2000, K=20, ext=ext)]
    steps.append(synth.make_raw_odometry_step(pm, steps[0].last_imu, steps[0].end_time, st[21:24], scale_gravity=ref.scale_gravity, truth_prev=steps[0].truth_end,
                                              n_points=2000, K=20, ext=ext, seed=synth.MASTER_SEED + 977))
    lidar, lay = IC.KINDS["velodyne22"]
    ea, eb = _ekf(kw), _ekf(kw)
    with ea, eb:
        E.initialise(ea, t_end=100.0, lag=E.LAG); E.initialise(eb, t_end=100.0, lag=E.LAG)
        la = vxba.LioEstimator(pm.voxel_size, pm.max_layer); la.map_update(*pm.args())
        lb = vxba.LioEstimator(pm.voxel_size, pm.max_layer); lb.map_update(*pm.args())
        fa, fb = front.OdometryFront(ea, la, ext, down_size=0.1), front.OdometryFront(eb, lb, ext, down_size=0.1)
        fi = front.ScanIntake(lidar, lay, point_filter_num=1, blind=0.01)
        sync = front.PackageSync()
        state, cov = steps[0].state_prev, steps[0].cov
        pending = []                                                                  # IMU messages not yet handed to the synchroniser
        for k, s in enumerate(steps):
            data = synth.make_driver_message(s.scan[0], synth.raw_times(s.scan[1], lay), lay, seed=k)
            want = R.process(data, lay, lidar, 1, 0.01, s.beg_time)
            beg = fi.push(data, s.beg_time)
            assert beg == s.beg_time and fi.record["record"].tobytes() == want["record"].tobytes()
            sync.add_scan(k, beg, float(fi.record["toff_last"]))
            msgs = pending if k else list(zip(*s.imus))                                  # step k's first message went in behind step k - 1
            nxt = list(zip(*steps[k + 1].imus)) if k + 1 < len(steps) else [(s.end_time + 0.01, s.imus[1][-1], s.imus[2][-1])]
            imus = []
            for m in msgs:
                sync.add_imu(*m)
            assert sync.sync(imus)[0] is False and sync.pl_ready                        # no message behind the scan's end yet: the scan persists
            sync.add_imu(*nxt[0]); pending = nxt[1:]
            ok, token, imus, b0, e0 = sync.sync(imus)
            assert ok and token == k and b0 == beg and e0 == beg + float(want["toff"][-1]) and len(imus) == 20
            packed = front.PackageSync.pack(imus)
            assert all(np.array_equal(x, y) for x, y in zip(packed, s.imus))
            ra = fa.step(state, cov, (want["xyz"], want["toff"]), packed, b0, e0)
            rb = fb.step_message(state, cov, fi, packed, b0, e0)
            assert ra["ready"] and rb["ready"] and ra["ok"] == rb["ok"] and ra["n_filtered"] == rb["n_filtered"] >= 500 and ra["half_size"] == rb["half_size"]
            for key in ("state", "cov", "state_prop", "cov_prop", "pwld"):
                assert ra[key].tobytes() == rb[key].tobytes(), key
            assert ea.read_scan().tobytes() == eb.read_scan().tobytes() and ea.filtered().tobytes() == eb.filtered().tobytes()
            state, cov = ra["state"], ra["cov"]
        fi.close(); la.close(); lb.close()
