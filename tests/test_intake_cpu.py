"""CPU checks of the driver-message intake: the checker (tests/_intake_ref.py) pinned to hand-computed cases and to properties, front.PackageSync against
the loop-by-loop restatement of sync_packages, the host build of csrc/vxba_intake_math.hpp against the checker on every case, the vxba_scan_layout
mirror against the C compiler, layout_from_fields' refusals and make_driver_message's round trips."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _intake_cases as IC
from tests import _intake_ref as R
from voxel_slam_amd import front, synth, vxba

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = IC.cases()
OK = sorted(n for n, c in CASES.items() if c["expect"] == "ok")
F = np.float32


def _livox(points):
    """A Livox message from (offset_time, x, y, z) tuples: CustomPoint is offset_time u32, x y z f32, reflectivity, tag, line u8."""
    return b"".join(struct.pack("<Ifff3B", t, x, y, z, 7, 0, 1) for t, x, y, z in points)


# ---- the checker against cases worked out by hand -----------------------------------------------------------------------------------------
def test_checker_hand_computed_livox():
    """Six points, point_filter_num 2, blind 1: indices 0, 2, 4 are candidates; (0.5, 0.5, 0.5) has range 0.75 and is blind; the other two come out by
    time, 0.02 s before 0.05 s although it came later."""
    pts = [(50000000, 2.0, 0.0, 0.0), (1, 9.0, 9.0, 9.0), (10000000, 0.5, 0.5, 0.5), (2, 9.0, 9.0, 9.0), (20000000, 0.0, -3.0, 0.0), (3, 9.0, 9.0, 9.0)]
    r = R.process(_livox(pts), front.layout_livox(), R.LIVOX, 2, 1.0, 12.5)
    assert r["xyz"].tolist() == [[0.0, -3.0, 0.0], [2.0, 0.0, 0.0]] and r["beg_time"] == 12.5
    assert r["toff"].tobytes() == np.array([F(20000000) / F(1e9), F(50000000) / F(1e9)], dtype=np.float32).tobytes()
    assert r["record"].tolist() == [2.0, float(F(0.02)), float(F(0.05)), 0.0, 6.0, 2.0]


def test_checker_strict_comparisons_and_trim():
    """Range exactly blind is dropped (strictly greater passes); the float 0.11 lies below the double 0.11 and stays, the next float above goes."""
    e = F(0.11)
    up = np.nextafter(e, F(1))
    assert float(e) < 0.11 < float(up)
    lay = IC.KINDS["velodyne22"][1]
    xyz = np.array([[2, 0, 0], [0, 2, 0], [0, 0, 2.0000002], [3, 0, 0], [3, 0, 0], [4, 0, 0]], dtype=np.float32)
    t = np.array([0.01, 0.02, 0.03, e, up, 0.05], dtype=np.float32)
    r = R.process(synth.make_driver_message(xyz, t, lay), lay, R.VELODYNE, 1, 4.0, 0.0)
    assert r["xyz"].tolist() == [[0, 0, F(2.0000002)], [4, 0, 0], [3, 0, 0]] and r["toff"].tolist() == [F(0.03), F(0.05), e]
    assert r["record"].tolist() == [3.0, float(F(0.03)), float(e), 0.0, 6.0, 4.0]


def test_checker_fallback_is_exact():
    for name in sorted(CASES):
        if name.startswith(("all-blind", "all-decimated")) or re.fullmatch(r"grid-(livox19|velodyne22|ouster48|tartanair16)-n0(-f\d+)?", name):
            r = IC.reference(name)
            assert r["xyz"].tobytes() == np.zeros((2, 3), np.float32).tobytes() and r["toff"].tobytes() == np.array([0.0, 0.09], np.float32).tobytes(), name
            assert r["record"].tolist() == [2.0, 0.0, float(F(0.09)), 1.0, float(CASES[name]["n"]), 0.0]


def test_checker_errors():
    assert {n for n in CASES if CASES[n]["expect"] != "ok"} == {n for n in CASES if "error" in IC.reference(n)}
    for n, c in CASES.items():
        if c["expect"] != "ok":
            assert IC.reference(n)["error"] == c["expect"], n
    r = IC.reference("all-trimmed-livox19")
    assert r["record"][:5].tolist() == [0.0, 0.0, 0.0, 0.0, 200.0] and 0 < r["record"][5] <= 50          # point_filter_num 4: at most 50 candidates


def _vectorised(c):
    """The same cloud without a loop: masks on the original indices, one stable argsort."""
    lay, lidar = c["layout"], c["lidar_type"]
    x, y, z, t = R.unpack(c["data"], lay)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        if lidar in (R.LIVOX, R.OUSTER):
            cur = t.astype(np.float32) / F(1e9)
        elif lidar == R.VELODYNE:
            cur = t.astype(np.float32)
        elif lidar in (R.HESAI, R.ROBOSENSE):
            cur = (t - t[0]).astype(np.float32)
        else:
            cur = np.zeros(n, np.float32)
        cur = np.where(cur == 0, F(0), cur).astype(np.float32)
        keep = np.ones(n, bool)
        if lidar != R.TARTANAIR:
            s = ((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32) + (z * z).astype(np.float32)
            keep = (np.arange(n) % c["pfn"] == 0) & (s.astype(np.float64) > c["blind"])
        keep &= np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & np.isfinite(cur)
    idx = np.flatnonzero(keep)
    if idx.size == 0:
        return np.zeros((2, 3), np.float32), np.array([0.0, 0.09], np.float32), idx
    idx = idx[cur[idx].astype(np.float64) <= 0.11]
    idx = idx[np.argsort(cur[idx], kind="stable")]
    return np.stack([x[idx], y[idx], z[idx]], axis=1), cur[idx], idx


@pytest.mark.parametrize("name", OK)
def test_checker_properties(name):
    """Decimation on the original indices, the strict comparisons and a stable sort of the survivors: the loop-faithful checker equals a vectorised
    restatement bit for bit; times ascend, and equal times keep their input order."""
    c, r = CASES[name], IC.reference(name)
    xyz, toff, idx = _vectorised(c)
    assert r["xyz"].tobytes() == xyz.tobytes() and r["toff"].tobytes() == toff.tobytes()
    assert (np.diff(r["toff"]) >= 0).all() and not np.signbit(r["toff"][r["toff"] == 0]).any()
    if idx.size:
        assert (idx % (c["pfn"] if c["lidar_type"] != R.TARTANAIR else 1) == 0).all()
        same = np.diff(toff) == 0
        assert (np.diff(idx)[same] > 0).all()
        assert r["record"][0] == idx.size and r["record"][3] == 0 and r["record"][4] == c["n"]


def test_cases_reach_what_they_are_for():
    """The honesty of the case list: ties of 16 and 128 survive into the output, the blind edge drops exactly the points at and below, the u32 cases
    hold values whose float conversion rounds, negative times exist."""
    r = IC.reference("ties-livox19")
    _, counts = np.unique(r["toff"], return_counts=True)
    assert counts.max() >= 100 and (counts >= 16).sum() >= 2
    below, at, above, s0 = IC._blind_triplet()
    r = IC.reference("blind-edge-livox19")
    got = {tuple(p) for p in r["xyz"].tolist()}
    perms = lambda p: {tuple(float(F(v)) for v in q) for q in ((p[0], p[1], p[2]), (p[1], p[0], p[2]), (p[2], -p[1], -p[0]))}
    assert perms(above) <= got and not (perms(below) | perms(at)) & got and CASES["blind-edge-livox19"]["blind"] == float(s0)
    raw = R.unpack(CASES["u32-rounding-livox19"]["data"], front.layout_livox())[3]
    assert (raw[:18].astype(np.float32).astype(np.float64) != raw[:18].astype(np.float64)).sum() >= 8 and raw.max() == 2 ** 32 - 1
    assert IC.reference("before-head-hesai23")["toff"][0] < 0 and IC.reference("before-head-robosense31")["beg_time"] == IC.time_head("before-head-robosense31")
    assert {c["layout"].point_step for c in CASES.values()} >= {19, 22, 23, 48} and {c["n"] for c in CASES.values()} >= set(IC.SIZES)


# ---- sync_packages ---------------------------------------------------------------------------------------------------------------------------
def _script(seed, notime):
    """Interleaved handler calls and sync attempts: ("imu", stamp) | ("scan", beg, toff_last) | ("sync",)."""
    rng = np.random.Generator(np.random.PCG64([99, seed]))
    ev, t_imu, t_scan = [], 10.0, 10.0
    for _ in range(120):
        u = rng.random()
        if u < 0.55:
            t_imu += float(rng.choice([0.005, 0.01, 0.02, 0.04]))
            ev.append(("imu", t_imu))
        elif u < 0.7:
            t_scan += 0.1
            ev.append(("scan", t_scan, float(rng.choice([0.0, 0.05, 0.0999, 0.1]))))
        else:
            ev.append(("sync",))
    return ev


@pytest.mark.parametrize("notime", [0, 1])
@pytest.mark.parametrize("seed", range(8))
def test_package_sync_equals_the_restatement(seed, notime):
    a, b = R.SyncRef(notime), front.PackageSync(bool(notime))
    returns = set()
    ia, ib = [], []
    for k, e in enumerate(_script(seed, notime)):
        if e[0] == "imu":
            a.imu_handler(e[1]); b.add_imu(e[1], np.full(3, e[1]), np.full(3, -e[1]))
        elif e[0] == "scan":
            a.pcl_handler(k, e[1], e[2]); b.add_scan(k, e[1], e[2])
        else:
            try:
                ra = a.sync_packages(ia)
            except SystemExit:
                with pytest.raises(RuntimeError):
                    b.sync(ib)
                returns.add("exit")
                break
            ok, scan, _, beg, end = b.sync(ib)
            assert ok == ra and [m[0] for m in ib] == ia and b.pl_ready == a.pl_ready
            if a.pl_ptr is not None:
                assert (scan, beg, end) == (a.pl_ptr, a.pcl_beg_time, a.pcl_end_time)
            assert len(b.imu_buf) == len(a.imu_buf) and len(b.pcl_buf) == len(a.pcl_buf) and b.last_pcl_time == a.last_pcl_time
            returns.add((ra, a.pl_ready, len(ia) > 4))
            if ra or not a.pl_ready:
                ia, ib = [], []                       # the caller's deque is cleared once a package was formed, complete or not
    assert len(returns) >= 2


def test_package_sync_every_early_return():
    s = front.PackageSync()
    assert s.sync([])[0] is False                                        # no scan
    s.add_scan("a", 1.0, 0.1)
    assert s.sync([])[0] is False and s.pl_ready and s.scan == "a"       # no IMU behind the scan's end (imu_last_time -1)
    for k in range(3):
        s.add_imu(1.0 + 0.03 * k, np.zeros(3), np.zeros(3))
    assert s.sync([])[0] is False and s.pl_ready                         # imu_last_time 1.06 <= 1.1: the scan persists
    s.add_imu(1.1, np.zeros(3), np.zeros(3))
    assert s.sync([])[0] is False and s.pl_ready                         # == end: still <=
    s.add_imu(1.2, np.zeros(3), np.zeros(3))
    imus = []
    ok, scan, _, beg, end = s.sync(imus)
    assert ok is False and not s.pl_ready and [m[0] for m in imus] == [1.0, 1.03, 1.06, 1.1] and len(s.imu_buf) == 1      # <= 4 messages: false, yet consumed
    assert (scan, beg, end) == ("a", 1.0, 1.1)
    s.add_scan("b", 1.1, 0.15)
    for t in (1.21, 1.22, 1.23, 1.24, 1.25, 1.26):
        s.add_imu(t, np.zeros(3), np.zeros(3))
    imus = []
    ok = s.sync(imus)[0]
    assert ok is True and [m[0] for m in imus] == [1.2, 1.21, 1.22, 1.23, 1.24, 1.25] and s.end_time == 1.25      # a stamp equal to the end is taken, then the condition ends the loop
    s.add_scan("c", 1.25, 0.1)
    s.add_imu(1.3, np.zeros(3), np.zeros(3)); s.add_imu(1.4, np.zeros(3), np.zeros(3))
    imus = []
    assert s.sync(imus)[0] is False and [m[0] for m in imus] == [1.26, 1.3] and [m[0] for m in s.imu_buf] == [1.4]   # the `>` break
    n = front.PackageSync(point_notime=True)
    n.add_scan("a", 5.0, 0.0); n.add_scan("b", 5.1, 0.0)
    n.add_imu(5.05, np.zeros(3), np.zeros(3))
    assert n.sync([])[0] is False and not n.pl_ready and n.last_pcl_time == 5.0          # point_notime: the first scan only sets last_pcl_time
    n.add_imu(5.4, np.zeros(3), np.zeros(3))
    imus = []
    assert n.sync(imus) == (False, "b", imus, 5.0, 5.1) and [m[0] for m in imus] == [5.05]      # the shuffle: beg is the previous scan's stamp, end this one's
    e = front.PackageSync()
    e.add_scan("a", 1.0, 0.1); e.imu_last_time = 2.0
    with pytest.raises(RuntimeError, match="imu buf empty"):
        e.sync([])


# ---- the host build of the product's header against the checker ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "intake_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libintake_hostcheck.so")
    hdr = os.path.join(ROOT, "voxel-slam_amd", "csrc", "vxba_intake_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.ikh_decode.argtypes = [C.c_void_p, C.c_longlong, C.POINTER(vxba.ScanLayout), C.c_longlong, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def host_cloud(hm, c, head, shift):
    """What the device does with decode_point's verdicts: candidates to slots, a stable sort of (key, slot), survivors in front."""
    n = c["n"]
    out, verdict, key = np.zeros((max(n, 1), 4), np.float32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32)
    buf = np.frombuffer(c["data"], dtype=np.uint8)
    pfn = c["pfn"] if c["layout"].filter else 1
    hm.ikh_decode(buf.ctypes.data if n else None, n, C.byref(c["layout"]), pfn, c["blind"], head, shift, out.ctypes.data, verdict.ctypes.data, key.ctypes.data)
    out, verdict, key = out[:n], verdict[:n], key[:n]
    passed = int((verdict >= 3).sum())
    if passed == 0:
        return np.zeros((2, 3), np.float32), np.array([0.0, 0.09], np.float32), np.array([2.0, 0.0, float(F(0.09)), 1.0, n, 0.0])
    idx = np.flatnonzero(verdict == 4)
    assert (key[idx] != 0xFFFFFFFF).all()
    idx = idx[np.argsort(key[idx], kind="stable")]
    xyz, toff = out[idx, :3].copy(), out[idx, 3].copy()
    return xyz, toff, np.array([idx.size, float(toff[0]) if idx.size else 0.0, float(toff[-1]) if idx.size else 0.0, 0.0, n, passed])


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["expect"] in ("ok", "all_trimmed")))
def test_host_math_equals_the_checker(hm, name):
    c, r = CASES[name], IC.reference(name)
    for shift in (0, 3) if c["n"] > 300 else (0, 1, 2, 3):
        xyz, toff, rec = host_cloud(hm, c, IC.time_head(name), shift)
        assert rec.tolist() == r["record"].tolist()
        if c["expect"] == "ok":
            assert xyz.tobytes() == r["xyz"].tobytes() and toff.tobytes() == r["toff"].tobytes()


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_scan_layout_mirror_has_the_layout_the_c_compiler_gives(tmp_path, hm):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    (tmp_path / "layout.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vxba.h"\nint main(void) {\n'
                                       '  printf("%zu %zu %d %d\\n", sizeof(vxba_scan_layout), offsetof(vxba_scan_layout, filter), VXBA_SCAN_MAX_STEP, VXBA_INTAKE_REC_LEN);\n'
                                       '  printf("%d %d %d %d %d %d %d %d\\n", VXBA_SCAN_TIME_NONE, VXBA_SCAN_TIME_F32, VXBA_SCAN_TIME_U32, VXBA_SCAN_TIME_F64, VXBA_SCAN_RULE_NONE,\n'
                                       '         VXBA_SCAN_RULE_AS_IS, VXBA_SCAN_RULE_NANOSECONDS, VXBA_SCAN_RULE_MINUS_HEAD);\n  return 0;\n}\n')
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    a, b = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    S = vxba.ScanLayout
    assert [int(v) for v in a.split()] == [C.sizeof(S), S.filter.offset, S.MAX_STEP, len(vxba.ScanIntake.REC)]
    assert [int(v) for v in b.split()] == [S.TIME_NONE, S.TIME_F32, S.TIME_U32, S.TIME_F64, S.RULE_NONE, S.RULE_AS_IS, S.RULE_NANOSECONDS, S.RULE_MINUS_HEAD]
    assert [f for f, _ in S._fields_] == ["point_step", "off_x", "off_y", "off_z", "off_time", "time_type", "time_rule", "filter"]
    k = (C.c_int32 * 5)()
    hm.ikh_constants(k)
    assert list(k) == [S.MAX_STEP, 4, 0, 3, C.sizeof(S)]


def test_layouts():
    assert front.layout_livox().as_tuple() == (19, 4, 8, 12, 0, 2, 2, 1)
    assert IC.KINDS["velodyne22"][1].as_tuple() == (22, 0, 4, 8, 18, 1, 1, 1)
    assert IC.KINDS["hesai23"][1].as_tuple() == (23, 1, 5, 9, 14, 3, 3, 1)
    assert IC.KINDS["tartanair16"][1].as_tuple() == (16, 0, 4, 8, 0, 0, 0, 0)


XYZ = [("x", 0, 7), ("y", 4, 7), ("z", 8, 7)]


@pytest.mark.parametrize("fields,step,lidar,kw", [
    (XYZ + [("time", 12, 7)], 16, front.VELODYNE, {"is_bigendian": True}),        # big-endian
    (XYZ + [("time", 12, 7)], 16, front.LIVOX, {}),                                # not a PointCloud2 sensor
    (XYZ + [("time", 12, 7)], 16, 9, {}),                                          # no such sensor
    ([("x", 0, 8), ("y", 8, 7), ("z", 12, 7), ("time", 16, 7)], 20, front.VELODYNE, {}),   # x as FLOAT64
    (XYZ[:2] + [("time", 12, 7)], 16, front.VELODYNE, {}),                         # no z
    (XYZ, 12, front.VELODYNE, {}),                                                 # no time field
    (XYZ + [("t", 12, 6)], 16, front.VELODYNE, {}),                                # another sensor's name
    (XYZ + [("time", 12, 8)], 20, front.VELODYNE, {}),                             # time as FLOAT64
    (XYZ + [("t", 12, 7)], 16, front.OUSTER, {}),                                  # t as FLOAT32
    (XYZ + [("timestamp", 12, 7)], 16, front.HESAI, {}),                           # timestamp as FLOAT32
    (XYZ + [("timestamp", 12, 8)], 16, front.ROBOSENSE, {}),                       # the field ends behind point_step
    (XYZ + [("time", 10, 7)], 16, front.VELODYNE, {}),                             # time overlaps z
    (XYZ + [("time", 12, 7), ("time", 16, 7)], 20, front.VELODYNE, {}),            # listed twice
    (XYZ + [("time", 12, 7)], 300, front.VELODYNE, {}),                            # point_step above the limit
    ([("x", -4, 7), ("y", 4, 7), ("z", 8, 7)], 16, front.TARTANAIR, {}),           # a negative offset
])
def test_layout_from_fields_refusals(fields, step, lidar, kw):
    with pytest.raises(ValueError):
        front.layout_from_fields(fields, step, lidar, **kw)


@pytest.mark.parametrize("kind", sorted(IC.KINDS))
def test_make_driver_message_round_trips(kind):
    lidar, lay = IC.KINDS[kind]
    rng = np.random.Generator(np.random.PCG64(5))
    xyz = rng.normal(size=(37, 3)).astype(np.float32); xyz[3, 1] = np.nan; xyz[4, 2] = -0.0
    toff = rng.uniform(0, 0.1, 37)
    raw = synth.raw_times(toff, lay, 1.7e9)
    a, b = synth.make_driver_message(xyz, raw, lay, seed=1), synth.make_driver_message(xyz, raw, lay, seed=2)
    assert len(a) == 37 * lay.point_step
    x, y, z, t = R.unpack(a, lay)
    assert np.stack([x, y, z], axis=1).tobytes() == xyz.tobytes()
    if raw is None:
        assert t is None
    else:
        assert t.tobytes() == np.ascontiguousarray(raw).tobytes()
    # the padding is noise: two seeds differ exactly outside the fields
    used = np.zeros(lay.point_step, bool)
    for o in (lay.off_x, lay.off_y, lay.off_z):
        used[o:o + 4] = True
    if raw is not None:
        used[lay.off_time:lay.off_time + np.asarray(raw).dtype.itemsize] = True
    da, db = np.frombuffer(a, np.uint8).reshape(37, -1), np.frombuffer(b, np.uint8).reshape(37, -1)
    assert (da[:, used] == db[:, used]).all() and (used.all() or (da[:, ~used] != db[:, ~used]).any())
