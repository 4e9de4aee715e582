"""vxba_intake_push_yaw on the GPU against the loop-faithful replay of tests/_intake_yaw_ref.py: every case of tests/_intake_yaw_cases.py byte for byte
(tests/test_intake_yaw_cpu.py shows why the inputs allow that), the refusals, the launch and wait counts, the hand-on to the de-skew, and the routing
of front.ScanIntake."""
import ctypes as C

import numpy as np
import pytest

from tests import _imuekf_ref as E
from tests import _intake_cases as IC
from tests import _intake_ref as R
from tests import _intake_yaw_cases as YC
from tests import _intake_yaw_ref as YR

pytestmark = pytest.mark.gpu

CASES = YC.cases()
LAUNCHES = 6


@pytest.fixture(scope="module")
def intake():
    from voxel_slam_amd import vxba
    with vxba.ScanIntake() as h:
        yield h


def _push(h, name):
    c = CASES[name]
    return h.push_yaw(c["layout"], c["data"], c["pfn"], c["blind"], c["omega_l"])


def _same_cloud(h, rec, ref):
    assert rec["record"].tobytes() == ref["record"].tobytes(), (rec["record"], ref["record"])
    xyz, toff = h.read()
    assert xyz.tobytes() == ref["xyz"].tobytes() and toff.tobytes() == ref["toff"].tobytes()
    assert h.stats()["n"] == ref["xyz"].shape[0] == rec["n_out"]
    info = h.yaw_info()
    assert [info[k] for k in YR.COUNTS] == ref["counts"].tolist(), (info, ref["counts"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_push_yaw_equals_the_replay(intake, name):
    ref = YC.reference(name)
    _same_cloud(intake, _push(intake, name), ref)
    s = intake.stats()
    assert s["launches"] == LAUNCHES and s["n_decoded"] == CASES[name]["n"]


def test_every_refusal_leaves_the_previous_result_readable(intake):
    from voxel_slam_amd import vxba
    S = vxba.ScanLayout
    good = "cw_n257"
    c, ref = CASES[good], YC.reference(good)
    lay = YC.LAYOUTS["velodyne22"]
    data22 = next(v["data"] for _, v in sorted(CASES.items()) if v["layout_name"] == "velodyne22" and v["n"] == 257)
    _same_cloud(intake, _push(intake, good), ref)
    stats, info = intake.stats(), intake.yaw_info()
    bad = {
        "a layout that is not RULE_YAW": (S(22, 0, 4, 8, 18, S.TIME_F32, S.RULE_AS_IS, 1), data22, 1, 1.0, 3610.0),
        "no rule at all": (S(22, 0, 4, 8, 0, S.TIME_NONE, S.RULE_NONE, 0), data22, 1, 1.0, 3610.0),
        "omega_l 0": (lay, data22, 1, 1.0, 0.0),
        "omega_l negative": (lay, data22, 1, 1.0, -3610.0),
        "omega_l NaN": (lay, data22, 1, 1.0, float("nan")),
        "omega_l inf": (lay, data22, 1, 1.0, float("inf")),
        "u32 time under the yaw rule": (S(22, 0, 4, 8, 18, S.TIME_U32, S.RULE_YAW, 1), data22, 1, 1.0, 3610.0),
        "f64 time under the yaw rule": (S(22, 0, 4, 8, 12, S.TIME_F64, S.RULE_YAW, 1), data22, 1, 1.0, 3610.0),
        "filter 0 under the yaw rule": (S(22, 0, 4, 8, 18, S.TIME_F32, S.RULE_YAW, 0), data22, 1, 1.0, 3610.0),
        "point_filter_num 0": (lay, data22, 0, 1.0, 3610.0),
        "point_step below 12": (S(11, 0, 4, 7, 0, S.TIME_NONE, S.RULE_YAW, 1), data22[:11 * 100], 1, 1.0, 3610.0),
        "point_step above the limit": (S(S.MAX_STEP + 1, 0, 4, 8, 0, S.TIME_NONE, S.RULE_YAW, 1), data22[:(S.MAX_STEP + 1) * 10], 1, 1.0, 3610.0),
        "point_step smaller than z's end": (S(13, 0, 4, 10, 0, S.TIME_NONE, S.RULE_YAW, 1), data22[:13 * 100], 1, 1.0, 3610.0),
        "x overlaps y": (S(22, 0, 2, 8, 18, S.TIME_F32, S.RULE_YAW, 1), data22, 1, 1.0, 3610.0),
        "the ignored time field overlaps z": (S(22, 0, 4, 8, 10, S.TIME_F32, S.RULE_YAW, 1), data22, 1, 1.0, 3610.0),
        "blind NaN": (lay, data22, 1, float("nan"), 3610.0),
    }
    for why, (layout, msg, pfn, blind, omega) in bad.items():
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            intake.push_yaw(layout, msg, pfn, blind, omega)
        assert not intake.last_record.any() and intake.stats() == stats and intake.yaw_info() == info, why
    # plain push with a RULE_YAW layout: omega_l is missing
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        intake.push(lay, data22, 1, 1.0)
    assert not intake.last_record.any() and intake.stats() == stats
    # n_points out of range and a null message: the C entry point
    rec = np.zeros(6)
    buf = np.frombuffer(data22, dtype=np.uint8)
    for n_points, ptr in ((2 ** 31, buf.ctypes.data_as(C.c_void_p)), (-1, buf.ctypes.data_as(C.c_void_p)), (257, None)):
        assert intake._L.vxba_intake_push_yaw(intake._h, C.byref(lay), n_points, ptr, 1, 1.0, 3610.0, rec) == 1 and not rec.any()
    xyz, toff = intake.read()
    assert xyz.tobytes() == ref["xyz"].tobytes() and toff.tobytes() == ref["toff"].tobytes()
    # yaw_info belongs to a yaw push only
    plain = "grid-livox19-n65-f3"
    p = IC.cases()[plain]
    intake.push(p["layout"], p["data"], p["pfn"], p["blind"], IC.time_head(plain))
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_STATE"):
        intake.yaw_info()
    assert intake.stats()["launches"] == 2
    _same_cloud(intake, _push(intake, good), ref)


def test_launches_and_waits_do_not_depend_on_n():
    from voxel_slam_amd import vxba
    seen = {}
    with vxba.ScanIntake() as h:
        _push(h, "cw_n4097")                                                # the largest message first: no growth afterwards
        for name in ("cw_n257", "cw_n4097", "cw_n0", "cw_n1", "cw_n1025", "gaussian_n4097", "all_specials_n2049", "specials_65"):
            _push(h, name)
            s = h.stats()
            seen[name] = (s["launches"], s["waits"])
    print("stats", seen)
    assert seen["cw_n257"] == seen["cw_n4097"] and set(seen.values()) == {(LAUNCHES, 1)}, seen


def test_growth_and_reuse():
    """One handle pushed with 4097, then 1, then 4097 points on the yaw route and a plain push in between: the buffers grow once and every cloud is
    the replay's."""
    from voxel_slam_amd import vxba
    waits = []
    with vxba.ScanIntake() as h:
        for name in ("gaussian_n4097", "cw_n1", "cw_n4097"):
            _same_cloud(h, _push(h, name), YC.reference(name))
            waits.append(h.stats()["waits"])
        p = IC.cases()["grid-livox19-n65-f3"]
        h.push(p["layout"], p["data"], p["pfn"], p["blind"], 0.0)
        _same_cloud(h, _push(h, "events_at_small_angles"), YC.reference("events_at_small_angles"))
    assert waits[0] == 2 and waits[1] == 1


def _ekf(kw):
    from voxel_slam_amd import vxba
    return vxba.ImuEkf(vxba.ImuEkfParams.make(**E.filter_options(kw)))


def test_process_device_on_a_yaw_timed_cloud_equals_process_on_the_read_back_arrays(intake):
    kw = dict(n=257, K=5, seed=51, lag=E.LAG)
    a, b = _ekf(kw), _ekf(kw)
    with a, b:
        c, _, _, got_a = E.run_case(a, kw)
        _, _, _, got_b = E.run_case(b, kw)
        assert got_a["ready"] and got_a["state"].tobytes() == got_b["state"].tobytes()
        state, cov, t_end = got_a["state"], got_a["cov"], c["end"]
        for name in ("cw_n1025", "cw_start-179.9_jitter3_n2049"):
            n = CASES[name]["n"]
            nxt = E.make_case(n, 5, seed=70 + n, t_end=t_end, ties=True)
            _same_cloud(intake, _push(intake, name), YC.reference(name))
            arrays = intake.read()
            assert 1 < arrays[0].shape[0] <= n
            ra = a.process(state, cov, arrays, nxt["imus"], nxt["beg"], nxt["end"])
            rb = b.process_device(state, cov, intake, nxt["imus"], nxt["beg"], nxt["end"])
            assert ra["ready"] and rb["ready"] and rb["compensated"] == -1 and ra["compensated"] >= 0
            for k in ("state", "cov"):
                assert ra[k].tobytes() == rb[k].tobytes()
            assert a.read_scan().tobytes() == b.read_scan().tobytes() and a.pose_table().tobytes() == b.pose_table().tobytes()
            assert (b.stats()["launches"], b.stats()["n"]) == (1, arrays[0].shape[0])
            state, cov, t_end = ra["state"], ra["cov"], nxt["end"]


def test_front_routes_by_layout_and_by_the_last_time():
    """front.ScanIntake(yaw_times=True): a RULE_YAW layout and an AS_IS message whose last time fails upstream's test go to the yaw route, a message
    with good times goes to the plain one; without yaw_times the bad-time message is refused as before."""
    from voxel_slam_amd import front, synth, vxba
    lidar, lay = IC.KINDS["velodyne22"]
    assert int(lay.time_rule) == vxba.ScanLayout.RULE_AS_IS
    c = next(v for k, v in sorted(CASES.items()) if v["layout_name"] == "velodyne22" and v["n"] == 2049 and k.startswith("cw_"))
    ref = YR.replay(c["x"], c["y"], c["z"], 3, 1.0, 3610.0)
    xyz = np.stack([c["x"], c["y"], c["z"]], axis=1)
    bad = synth.make_driver_message(xyz, np.zeros(c["n"], dtype=np.float32), lay, seed=5)            # a driver that leaves the time field zero
    t = np.linspace(0.0, 0.09, c["n"]).astype(np.float32)
    good = synth.make_driver_message(xyz, t, lay, seed=5)
    want_good = R.process(good, lay, lidar, 3, 1.0, 100.25)
    f = front.ScanIntake(front.VELODYNE, lay, point_filter_num=3, blind=1.0, yaw_times=True)
    try:
        assert f.push(bad, 100.25) == 100.25 and f.route == "yaw"
        assert f.record["record"].tobytes() == ref["record"].tobytes()
        xyz_g, toff_g = f.read()
        assert xyz_g.tobytes() == ref["xyz"].tobytes() and toff_g.tobytes() == ref["toff"].tobytes()
        assert f.dev.yaw_info()["active"] == int(ref["counts"][1])
        assert f.push(good, 100.25) == 100.25 and f.route == "push"
        xyz_g, toff_g = f.read()
        assert xyz_g.tobytes() == want_good["xyz"].tobytes() and toff_g.tobytes() == want_good["toff"].tobytes()
    finally:
        f.close()
    # a RULE_YAW layout from the field list: no time field needed
    lay16 = front.layout_velodyne_yaw([("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 12, 7)], 16)
    assert lay16.as_tuple() == (16, 0, 4, 8, 0, 0, vxba.ScanLayout.RULE_YAW, 1)
    f = front.ScanIntake(front.VELODYNE, lay16, point_filter_num=3, blind=1.0, yaw_times=True)
    try:
        assert f.push(synth.make_driver_message(xyz, None, lay16, seed=6), 7.5) == 7.5 and f.route == "yaw"
        assert f.record["record"].tobytes() == ref["record"].tobytes() and f.read()[1].tobytes() == ref["toff"].tobytes()
    finally:
        f.close()
    # the defaults are today's behaviour: the bad-time message is refused
    f = front.ScanIntake(front.VELODYNE, lay, point_filter_num=3, blind=1.0)
    try:
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_UNSUPPORTED"):
            f.push(bad, 100.25)
        assert f.push(good, 100.25) == 100.25 and f.route == "push"
    finally:
        f.close()
    # the field-list checks are layout_from_fields'
    for fields, step in (([("x", 0, 7), ("y", 4, 7)], 16), ([("x", 0, 7), ("y", 2, 7), ("z", 8, 7)], 16), ([("x", 0, 7), ("y", 4, 7), ("z", 8, 8)], 16),
                         ([("x", 0, 7), ("y", 4, 7), ("z", 8, 7)], 11), ([("x", 0, 7), ("y", 4, 7), ("z", 14, 7)], 16)):
        with pytest.raises(ValueError):
            front.layout_velodyne_yaw(fields, step)
