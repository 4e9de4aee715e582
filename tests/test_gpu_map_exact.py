"""The incremental local map on the GPU (csrc/vxba_map.hip) on its own against exact arithmetic: every case of tests/_map_cases.py through
vxba.LocalMap and vxba.LidarFactor in lockstep with the plain reference of tests/_map_ref.py (pinned to the oracle and to the fix-form golden
by tests/test_map_cpu.py, which also asserts that each case takes the path it was built for).  After every stage structure, sequential sums
and the stored points (vxba_map_leaf_points) are array_equal with the reference's; eigen-pairs, margi's sums and the plane records are held to
the criteria and constants recorded in tests/_map_cases.py (C = 4 K, K measured on CPU reference code)."""
import numpy as np
import pytest

from tests import _map_cases as Cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


@pytest.mark.parametrize("name", Cs.CASE_NAMES)
def test_case(vx, monkeypatch, name):
    case = Cs.get_case(name)
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    side = Cs.DeviceSide(vx, case["prm"])
    try:
        ref, err = Cs.run(case, side)
        print(name, {k: round(v[0], 2) for k, v in err.worst.items()})
        Cs.check_errors(err, Cs.FACTOR_DEVICE, label=name)
        if case.get("env"):
            assert side.m.fix_pool()["compactions"] >= 1          # the pool really moved under the leaves
    finally:
        side.close()


def test_pool_moves_change_no_bit(vx, monkeypatch):
    """The same operations with the fix pool compacted on the way and without: every leaf's table and stored points equal bit for bit."""
    tables = []
    for compact in (False, True):
        case = Cs.case_pool_moves(compact)
        for k, v in case.get("env", {}).items():
            monkeypatch.setenv(k, v)
        side = Cs.DeviceSide(vx, case["prm"])
        try:
            ref, _ = Cs.run(case, side)
            lv = side.leaves()
            pts = [side.m.leaf_points(int(i), w) for i in lv["node_id"] for w in range(-1, case["prm"]["win_size"])]
            tables.append((lv, pts))
        finally:
            side.close()
    (la, pa), (lb, pb) = tables
    assert all(np.array_equal(v, lb[k]) for k, v in la.items() if isinstance(v, np.ndarray))
    assert len(pa) == len(pb) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(pa, pb))


def test_leaf_points_refuses_what_it_cannot_answer(vx):
    with vx.LocalMap(win_size=3, thread_num=1) as m:
        with pytest.raises(vx.VxbaError):
            m.leaf_points(12345, -1)                      # no leaf has this id (the map is empty)
        case = Cs.get_case("fc1_ml2")
        m.cut_voxel_fix(case["ops"][0][1], case["ops"][0][2], 0.0)
        nid = int(m.leaves()["node_id"][0])
        p, v = m.leaf_points(nid, -1)
        assert np.array_equal(p, case["ops"][0][1]) and np.array_equal(v, case["ops"][0][2])
        assert m.leaf_points(nid, 0)[0].shape == (0, 3)   # no window on a leaf that only holds loaded points
        with pytest.raises(vx.VxbaError):
            m.leaf_points(nid, 3)                         # beyond the window
