"""Yaw-derived Velodyne point times (feature_point.hpp:200-252) without a GPU: the loop-faithful replay against the restated parallel form, the
honesty of every input the GPU test uses, the host build of the arithmetic the kernels run, and degraded variants that the cases must catch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _intake_yaw_cases as YC
from tests import _intake_yaw_ref as YR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = sorted(YC.cases())


@pytest.fixture(scope="module")
def host():
    src = os.path.join(HERE, "hostmath", "intake_yaw_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libintake_yaw_hostcheck.so")
    hdr = os.path.join(ROOT, "voxel-slam_amd", "csrc", "vxba_intake_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.ikh_yaw_class.argtypes = [C.c_longlong, vp, vp]
    L.ikh_yaw_constants.argtypes = [vp]
    L.ikh_yaw_compose.argtypes = [vp]
    L.ikh_yaw_walk.argtypes = [C.c_longlong, vp, vp, vp, C.c_longlong, C.c_double, C.c_double, vp, vp, vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_axes_of_the_cases_are_all_there():
    cs = YC.cases()
    assert {c["n"] for c in cs.values()} >= set(YC.SIZES)
    assert {c["pfn"] for c in cs.values()} == {1, 3, 4} and {c["omega_l"] for c in cs.values()} == set(YC.OMEGAS)
    assert {c["layout_name"] for c in cs.values()} == set(YC.LAYOUTS)
    assert {(int(c["layout"].point_step), int(c["layout"].time_type)) for c in cs.values()} == {(22, 1), (16, 0), (19, 0)}
    assert all(int(c["layout"].time_rule) == 4 and len(c["data"]) == c["n"] * int(c["layout"].point_step) for c in cs.values())


@pytest.mark.parametrize("name", NAMES)
def test_replay_and_parallel_form_agree(name):
    """Kept indices, time bits, the double yaw of every active point, the counts and the cloud behind pcl_handler."""
    c = YC.cases()[name]
    ref, par = YC.reference(name), YR.parallel(c["x"], c["y"], c["z"], c["pfn"], c["blind"], c["omega_l"])
    assert np.array_equal(ref["kept"], par["kept"])
    assert ref["times"].tobytes() == par["times"].tobytes() and ref["yaw"].tobytes() == par["yaw"].tobytes()
    assert np.array_equal(ref["counts"], par["counts"])
    assert YR.same(ref, par)


def test_every_decision_keeps_its_distance_from_180():
    """Upstream decides on (r_j - bias) - yaw_last, the product on r_j - r_p: the two can only part within 2^-40 degrees of the threshold.  No case
    comes nearer than 1e-9 degrees."""
    worst = min((float(YC.reference(n)["margins"].min()), n) for n in NAMES if YC.reference(n)["margins"].size)
    print("smallest margin", worst)
    assert worst[0] >= 1e-9, worst


def test_no_point_lies_near_a_rounding_tie_of_the_float_atan2():
    """The device rounds a double atan2 to float; that is the correctly rounded float atan2 unless the exact value lies within the double routine's
    error of a tie between two floats.  mpmath: for every non-skipped point of every case the exact atan2 is farther than 2^-45 (relative) from both
    neighbouring ties, and the float64-then-float32 rounding the replay uses is the correct rounding."""
    import mpmath
    mp = mpmath.mp
    mp.prec = 120
    seen, worst = set(), None
    for name in NAMES:
        c = YC.cases()[name]
        x, y, z = c["x"], c["y"], c["z"]
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~(np.abs(x).astype(np.float64) < 0.1)
        for i in np.flatnonzero(ok):
            key = (x[i].tobytes(), y[i].tobytes())
            if key in seen:
                continue
            seen.add(key)
            exact = mp.atan2(mp.mpf(float(y[i])), mp.mpf(float(x[i])))
            got = YR.atan2f(y[i], x[i])
            if exact == 0:
                assert got == 0
                continue
            lo, hi = np.nextafter(got, np.float32(-4)), np.nextafter(got, np.float32(4))
            ties = [(mp.mpf(float(got)) + mp.mpf(float(lo))) / 2, (mp.mpf(float(got)) + mp.mpf(float(hi))) / 2]
            assert ties[0] < exact < ties[1], (name, i)                      # got is the correct rounding
            rel = min(abs(exact - t) for t in ties) / abs(exact)
            worst = rel if worst is None or rel < worst else worst
            assert rel > mp.mpf(2) ** -45, (name, i, float(rel))
    print("points", len(seen), "nearest tie (relative)", float(worst))
    assert len(seen) > 10000


def test_the_census_of_table_cells_and_seams_is_complete():
    cs, refs = YC.cases(), {n: YC.reference(n) for n in NAMES}
    cells = set().union(*(r["cells"] for r in refs.values()))
    # every cell of the table that angles can reach (d == 180 exactly is reached through the class function, below)
    assert cells >= {("cand", 0, True), ("cand", 0, False), ("cand", 1, None), ("ident", 0, None), ("ident", 1, None), ("set", 0, None), ("set", 1, None)}, cells
    par = {n: YR.parallel(cs[n]["x"], cs[n]["y"], cs[n]["z"], cs[n]["pfn"], cs[n]["blind"], cs[n]["omega_l"]) for n in NAMES}
    n_specials = {n: par[n]["specials"].size for n in NAMES}
    assert {64, 65} <= set(n_specials.values()) and 0 in n_specials.values()
    assert n_specials["all_specials_n2049"] == 2048                          # many chunks of the resolver
    assert n_specials["gaussian_n4097"] > 4097 // 5
    events = {n: int(refs[n]["counts"][3]) for n in NAMES}
    assert max(events.values()) >= 3 and min(events.values()) == 0
    # 999 apart: the second candidate is blocked and leaves q = 1, which the third one only takes back -- one event; 1000 and 1001: all three are events
    assert events["candidates_999_apart"] == 1 and events["candidates_1000_apart"] == 3 and events["candidates_1001_apart"] == 3
    assert events["candidates_1000_apart_skips_between"] == 3 and refs["candidates_1000_apart_skips_between"]["counts"][0] > 600
    # an event and specials behind it inside one chunk of 64 (the resolver scans the rest of the chunk again), and an event in a later chunk
    assert any(events[n] >= 1 and 2 <= n_specials[n] <= 64 for n in NAMES) and any(events[n] >= 2 and n_specials[n] > 128 for n in NAMES)
    # q = 1 at the last point of a workgroup: its governing special sits in the workgroup before
    q1 = refs["q1_across_workgroups"]
    assert par["q1_across_workgroups"]["specials"].tolist() == [250, 262] and not np.isin(np.arange(250, 262), q1["kept"]).any() and np.isin([249, 262], q1["kept"]).all()
    # fallback, the first point blind, nothing active, the blind boundary, non-finite coordinates
    assert refs["ccw_n257"]["record"][3] == 1 and refs["all_skipped"]["counts"][0] == 65 and refs["all_blind"]["counts"][1:].tolist() == [0, 0, 0]
    assert refs["all_blind"]["record"][3] == 1 and refs["cw_n0"]["record"][3] == 1
    assert 40 in refs["range_equals_blind"]["kept"] and refs["non_finite"]["counts"][0] >= 6
    fb = cs["first_point_blind"]
    assert abs(float(fb["x"][0])) < 0.1 and YR._range2(fb["x"][1], fb["y"][1], fb["z"][1]) < 1.0
    # survivors exist in every clockwise case with points
    assert all(refs[n]["record"][3] == 0 for n in NAMES if n.startswith("cw_") and cs[n]["n"] >= 63)


def test_class_function_at_the_exact_boundaries(host):
    """Synthetic d around -180 and 180, one ulp either side included: the host build of the header, the table, and the ``>=`` variant that must differ."""
    d = np.array([180.0, np.nextafter(180.0, 0.0), np.nextafter(180.0, 400.0), -180.0, np.nextafter(-180.0, 0.0), np.nextafter(-180.0, -400.0), 0.0, -0.0, 359.9, -359.9, 360.0, -360.0])
    want = [YR.RESET, YR.IDENT, YR.CAND, YR.IDENT, YR.IDENT, YR.SET, YR.IDENT, YR.IDENT, YR.CAND, YR.SET, YR.CAND, YR.SET]
    got = np.zeros(d.size, dtype=np.int32)
    assert host.ikh_yaw_class(d.size, _p(d), _p(got)) == 0
    k = np.zeros(6, dtype=np.int32)
    host.ikh_yaw_constants(_p(k))
    assert k.tolist() == [4, YR.IDENT, YR.SET, YR.RESET, YR.CAND, 1000]
    assert got.tolist() == want == [YR.classify(v) for v in d]
    assert [YR.classify(v, "ge_180") for v in d] != want
    ok = np.zeros(32, dtype=np.int32)
    host.ikh_yaw_compose(_p(ok))
    assert ok.all()


@pytest.mark.parametrize("name", NAMES)
def test_host_build_of_the_math_header_against_the_replay(host, name):
    """The functions of vxba_intake_math.hpp strung together as the kernels string them (the resolver pass by pass over 64 lanes): kept points, time
    bits, the double yaw of every active point and the four counts equal the replay's; the resolver needs at most ceil(S / 64) + events passes."""
    c, ref = YC.cases()[name], YC.reference(name)
    n = c["n"]
    m = max(n, 1)
    x, y, z = (np.ascontiguousarray(np.resize(c[k], m) if n else np.zeros(1, dtype=np.float32)) for k in "xyz")
    kept, t, yaw = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.float32), np.full(m, np.nan)
    counts, passes = np.zeros(4, dtype=np.int64), np.zeros(1, dtype=np.int64)
    assert host.ikh_yaw_walk(n, _p(x), _p(y), _p(z), c["pfn"], c["blind"], c["omega_l"], _p(kept), _p(t), _p(yaw), _p(counts), _p(passes)) == 0
    idx = np.flatnonzero(kept[:n])
    assert np.array_equal(idx, ref["kept"]) and t[idx].tobytes() == ref["times"].tobytes()
    assert yaw[:n].tobytes() == ref["yaw"].tobytes() and np.array_equal(counts, ref["counts"])
    S = YR.parallel(c["x"], c["y"], c["z"], c["pfn"], c["blind"], c["omega_l"])["specials"].size
    assert int(passes[0]) <= -(-S // 64) + int(counts[3])


@pytest.mark.parametrize("variant", YR.DEGRADED)
def test_degraded_variants_are_caught(variant):
    """Each deliberate defect of the parallel form parts from the replay on at least one case.  ``>=`` for ``>`` at 180 cannot part on angles (no
    difference of two float angles times 57.2957 is 180 exactly, and the margins above forbid it): it is caught on the synthetic boundary."""
    if variant == "ge_180":
        assert YR.classify(180.0, variant) != YR.classify(180.0) == YR.RESET
        return
    caught = []
    for name in NAMES:
        c = YC.cases()[name]
        if not YR.same(YC.reference(name), YR.parallel(c["x"], c["y"], c["z"], c["pfn"], c["blind"], c["omega_l"], variant=variant)):
            caught.append(name)
    print(variant, "caught by", caught)
    assert caught
    # and where the cloud itself shows it (what the GPU test compares), not only the double yaw
    if variant != "event_one_subtraction":
        assert any(YC.reference(n)["toff"].tobytes() != YR.parallel(*(YC.cases()[n][k] for k in ("x", "y", "z", "pfn", "blind", "omega_l")), variant=variant)["toff"].tobytes()
                   or YC.reference(n)["xyz"].tobytes() != YR.parallel(*(YC.cases()[n][k] for k in ("x", "y", "z", "pfn", "blind", "omega_l")), variant=variant)["xyz"].tobytes()
                   for n in caught)


def test_layout_velodyne_yaw_and_the_constants_of_the_binding(tmp_path):
    """front.layout_velodyne_yaw needs no time field and keeps layout_from_fields' checks; RULE_YAW is the header's VXBA_SCAN_RULE_YAW."""
    import shutil
    from voxel_slam_amd import front, vxba
    lay = front.layout_velodyne_yaw([("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 12, 7)], 16)
    assert lay.as_tuple() == (16, 0, 4, 8, 0, vxba.ScanLayout.TIME_NONE, vxba.ScanLayout.RULE_YAW, 1)
    assert front.layout_velodyne_yaw([("time", 18, 7), ("z", 13, 7), ("y", 7, 7), ("x", 1, 7)], 22).as_tuple() == (22, 1, 7, 13, 0, 0, 4, 1)
    for fields, step, big in (([("x", 0, 7), ("y", 4, 7)], 16, False), ([("x", 0, 7), ("y", 2, 7), ("z", 8, 7)], 16, False), ([("x", 0, 7), ("y", 4, 7), ("z", 8, 8)], 16, False),
                              ([("x", 0, 7), ("y", 4, 7), ("z", 8, 7)], 11, False), ([("x", 0, 7), ("y", 4, 7), ("z", 14, 7)], 16, False),
                              ([("x", 0, 7), ("x", 4, 7), ("y", 4, 7), ("z", 8, 7)], 16, False), ([("x", 0, 7), ("y", 4, 7), ("z", 8, 7)], 16, True)):
        with pytest.raises(ValueError):
            front.layout_velodyne_yaw(fields, step, is_bigendian=big)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    (tmp_path / "rule.c").write_text('#include <stdio.h>\n#include "vxba.h"\nint main(void) { printf("%d\\n", VXBA_SCAN_RULE_YAW); return 0; }\n')
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "rule"), str(tmp_path / "rule.c")], check=True)
    assert int(subprocess.run([str(tmp_path / "rule")], check=True, capture_output=True, text=True).stdout) == vxba.ScanLayout.RULE_YAW == 4
    assert {"vxba_intake_push_yaw", "vxba_intake_yaw_info"} <= set(vxba.EXPORTS)
