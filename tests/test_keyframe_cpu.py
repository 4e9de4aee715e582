"""Keyframe builder, CPU side: the numpy checker (tests/_keyframe_ref.py) against the reference's own filter (tests/golden/keyframe/keyframe.npz), the
host build of the device arithmetic (csrc/vxba_keyframe_math.hpp) against the checker, the keyframe rule against a hand-written expectation, and
the honesty of the inputs the GPU suite (tests/test_gpu_keyframe.py) runs."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import _keyframe_cases as KC
from tests import _keyframe_ref as K

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def G():
    spec = importlib.util.spec_from_file_location("tests._make_golden_keyframe", os.path.join(HERE, "golden", "keyframe", "make_golden_keyframe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(G):
    return G.load_fixture()


@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "keyframe_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libkeyframe_hostcheck.so")
    hdr = os.path.join(HERE, "..", "voxel-slam_amd", "csrc", "vxba_keyframe_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.kfh_delta.argtypes = [C.c_int, f64p, f64p, f64p, f64p]
    L.kfh_transform.argtypes = [C.c_int, f64p, f64p, f64p, f64p]
    L.kfh_keys.argtypes = [C.c_int, f64p, C.c_double, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"), np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")]
    L.kfh_mean.argtypes = [C.c_int, f64p, f64p]
    L.kfh_rule.argtypes = [f64p, f64p, f64p]
    return L


def run_case(case):
    b = K.KeyframeRef(case["win"], case["voxel_size"])
    emitted = [b.push_scan(*s) for s in case["scans"]]
    assert emitted == [False] * (case["win"] - 1) + [True]
    return b.keyframe


# ---- the checker against the reference ----------------------------------------------------------------------------------------------
def test_checker_matches_the_reference_keyframe(golden, G):
    b = K.KeyframeRef(golden["poses"].shape[0], float(golden["voxel_size"]))
    emitted = [b.push_scan(*s) for s in G.scans_of(golden)]
    assert emitted == [False, False, True]
    kf = b.keyframe
    assert kf["full"].shape == golden["full"].shape and np.array_equal(bits(kf["full"]), bits(golden["full"]))
    assert kf["down"].shape[0] == golden["down"].shape[0]
    assert np.array_equal(bits(kf["down"]), bits(golden["down"]))
    # the golden's rows are sorted by the reference's own voxel index: it is the checker's key order
    gi = golden["down_index"] + K.KEY_OFF
    assert np.array_equal((gi[:, 0] << 42) | (gi[:, 1] << 21) | gi[:, 2], kf["keys"].astype(np.int64))
    assert (kf["counts"] > 1).sum() > 100 and kf["counts"].max() >= 4      # the recurrence is exercised, not only copies


def test_golden_regenerates(golden, G):
    if not os.path.exists(os.path.join(G.REF_SRC, "voxel_map.hpp")):
        pytest.skip("the reference's sources are not present")
    with tempfile.TemporaryDirectory() as td:
        L, backend = G.load_reference(G.compile_harness(td))
        d = G.build(L, backend)
    for k in G.ARRAYS:
        assert np.array_equal(np.asarray(d[k]), golden[k]), k


def test_vectorised_filter_is_the_sequential_map_loop():
    for case in KC.all_cases():
        kf = run_case(case)
        down, index, counts = K.down_sampling_pvec_map(kf["q"], kf["var"], case["voxel_size"] / 10)
        assert np.array_equal(bits(down), bits(kf["down"])) and np.array_equal(counts, kf["counts"]), case["name"]


# ---- the host build of the device arithmetic against the checker -----------------------------------------------------------------------
def test_hostcheck_delta_and_transform(hm, golden):
    rng = np.random.default_rng(3)
    from voxel_slam_amd import synth
    n = 40
    Rs = np.stack([synth.rodrigues(rng.normal(size=3)) for _ in range(2 * n)])
    P = synth.pack_poses(Rs, 10 * rng.normal(size=(2 * n, 3)))
    xc, bl = np.ascontiguousarray(P[:n]), np.ascontiguousarray(P[n:])
    bl[0] = xc[0]                                                       # the newest scan against itself
    dR = np.zeros((n, 9)); dp = np.zeros((n, 3))
    hm.kfh_delta(n, xc.reshape(-1), bl.reshape(-1), dR.reshape(-1), dp.reshape(-1))
    pts = np.ascontiguousarray(golden["pnt"][:500])
    for k in range(n):
        rR, rp = K.delta_pose(xc[k], bl[k])
        assert np.array_equal(bits(rR), bits(dR[k])) and np.array_equal(bits(rp), bits(dp[k]))
        q = np.zeros_like(pts)
        hm.kfh_transform(pts.shape[0], np.ascontiguousarray(dR[k]), np.ascontiguousarray(dp[k]), pts.reshape(-1), q.reshape(-1))
        assert np.array_equal(bits(q), bits(K.transform(rR, rp, pts)))


def edge_coordinates():
    vs = KC.VS
    T = KC.TOP
    tiny = np.nextafter(0.0, 1.0)
    return np.array([0.0, -0.0, tiny, -tiny, -1e-30, vs, -vs, 2 * vs, -2 * vs, np.nextafter(vs, 0), np.nextafter(-vs, 0), np.nextafter(-vs, -1), 0.1, -0.1, 0.3, -0.3, 1e-3,
                     T * vs, -(T - 0.5) * vs, -(T - 1) * vs, (T + 1) * vs, -T * vs, np.nextafter((T + 1) * vs, 0), (T + 0.999) * vs, -(T + 5) * vs, 1e30, -1e30, 1e300, np.inf, -np.inf, np.nan])


def test_hostcheck_keys(hm, golden):
    e = edge_coordinates()
    rng = np.random.default_rng(4)
    q = np.concatenate([np.stack([e, np.zeros_like(e), np.zeros_like(e)], 1), np.stack([np.full_like(e, 0.1), e, np.full_like(e, -0.1)], 1), np.stack([e[::-1], e, e], 1),
                        20 * rng.normal(size=(3000, 3)), golden["pnt"][:600]])
    q = np.ascontiguousarray(q)
    for vs in (KC.VS, 0.1, 0.05):
        key = np.zeros(q.shape[0], np.uint64); ok = np.zeros(q.shape[0], np.uint8)
        hm.kfh_keys(q.shape[0], q.reshape(-1), vs, key, ok)
        rk, rok = K.voxel_keys(q, vs)
        assert np.array_equal(ok.astype(bool), rok) and np.array_equal(key, rk), vs
    # what the edge list is there for, at vs = 0.25: -vs is voxel -2 (a negative exact multiple moves one voxel down), -0.0 and the negative denormal (its float quotient is -0.0f, which is not < 0) are voxel 0, -1e-30 is voxel -1,
    # the outermost indices are accepted and the next ones refused
    idx, ok = K.voxel_index(e, KC.VS)
    look = dict(zip([repr(float(v)) for v in e], zip(idx.tolist(), ok.tolist())))
    assert look[repr(-KC.VS)] == (-2, True) and look["-0.0"] == (0, True) and look[repr(-float(np.nextafter(0.0, 1.0)))] == (0, True) and look["-1e-30"] == (-1, True)
    assert look[repr(KC.TOP * KC.VS)] == (KC.TOP, True) and look[repr(-(KC.TOP - 0.5) * KC.VS)] == (-KC.TOP, True)
    assert not look[repr((KC.TOP + 1) * KC.VS)][1] and not look[repr(-KC.TOP * KC.VS)][1] and not look["nan"][1] and not look["inf"][1] and not look["1e+300"][1]


def test_hostcheck_mean_recurrence(hm):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 300):
        rows = np.ascontiguousarray(rng.normal(size=(n, 6)) * np.array([50, 50, 5, 1e-3, 1e-3, 1e-3]))
        out = np.zeros(6)
        hm.kfh_mean(n, rows.reshape(-1), out)
        m = rows[0].copy()
        for c in range(1, n):
            m = K.mean_step(m, c, rows[c])
        assert np.array_equal(bits(out), bits(m)), n
    # through the whole filter: every voxel of the heavy case, bit for bit, the 300-point one included
    case = KC.heavy_voxel()
    kf = run_case(case)
    order = np.argsort(K.voxel_keys(kf["q"], KC.VS)[0], kind="stable")
    rows = np.ascontiguousarray(np.concatenate([kf["q"], kf["var"]], 1)[order])
    start = 0
    for v, cnt in enumerate(kf["counts"]):
        out = np.zeros(6)
        hm.kfh_mean(int(cnt), rows[start:start + cnt].reshape(-1), out)
        assert np.array_equal(bits(out.astype(np.float32)), bits(kf["down"][v]))
        start += cnt


def test_hostcheck_rule_metrics(hm):
    from voxel_slam_amd import synth
    rng = np.random.default_rng(6)
    for k in range(60):
        w = rng.normal(size=3) * (1e-5 if k % 3 == 0 else 0.05 if k % 3 == 1 else 1.0)
        Ra = synth.rodrigues(rng.normal(size=3))
        P = synth.pack_poses(np.stack([Ra, Ra @ synth.rodrigues(w)]), rng.normal(size=(2, 3)) * (0.05 if k % 2 else 1.0))
        out = np.zeros(2)
        hm.kfh_rule(np.ascontiguousarray(P[0]), np.ascontiguousarray(P[1]), out)
        ang, ln = K.rule_metrics(P[0], P[1])
        assert out[1] == ln and abs(out[0] - ang) <= 1e-12 * max(1.0, ang)      # acos / sin come from two libraries: the last bit may differ; len is exact


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_rule_against_hand_written_expectation():
    b = K.KeyframeRef(3)
    stream = KC.rule_stream()
    for k, s in enumerate(stream):
        assert b.push_scan(*s) == bool(KC.RULE_EMITTED[k]), k
        assert b.action == KC.RULE_ACTION[k] and len(b.ring) == KC.RULE_BUFFERED[k], k
        if KC.RULE_EMITTED[k]:
            kf = b.keyframe
            assert kf["id"] == KC.RULE_IDS[k] and kf["jour"] == KC.RULE_JOUR[k] and np.array_equal(kf["pose"], s[0])
            assert kf["full"].shape[0] == sum(i + 1 for i in KC.RULE_SCANS[k])
    P, V = b.scan_poses()
    assert P.shape == (14, 12) and np.array_equal(P, np.stack([s[0] for s in stream])) and np.array_equal(V[:, 0], 1e-4 * np.arange(1, 15))
    # after clear: no keyframe, no poses, and a stationary first window still emits (buf_base is not beyond win_size yet), with id 2 and jour 0
    b.clear()
    assert b.keyframe is None and b.num_scans() == 0 and b.jour == 0.0
    assert [b.push_scan(stream[3][0], stream[3][1], stream[k][2]) for k in range(3)] == [False, False, True]
    assert b.keyframe["id"] == 2 and b.keyframe["jour"] == 0.0 and b.keyframe["full"].shape[0] == 6
    # the next stationary window is dropped scan by scan
    assert [b.push_scan(stream[3][0], stream[3][1], stream[k][2]) for k in range(4)] == [False] * 4 and b.action == "drop" and len(b.ring) == 2


def test_bad_input_changes_nothing():
    for name, bad in KC.bad_cases():
        b = K.KeyframeRef(3, KC.VOXEL_SIZE)
        for k in range(3):
            b.push_scan(KC.IDENT, KC.V6, KC.lattice(4, 10 * k))
        before = (b.keyframe["id"], b.num_scans(), len(b.ring), b.buf_base)
        b.push_scan(KC.IDENT, KC.V6, KC.lattice(4, 40)); b.push_scan(KC.IDENT, KC.V6, KC.lattice(4, 50))
        with pytest.raises(ValueError):
            b.push_scan(KC.MOVED, KC.V6, bad)
        assert (b.keyframe["id"], b.num_scans() - 2, len(b.ring) - 2, b.buf_base - 2) == before, name
        assert b.push_scan(KC.MOVED, KC.V6, KC.lattice(4, 60)) and b.keyframe["id"] == 5 and b.keyframe["jour"] == 1.0, name


# ---- honesty of the GPU suite's inputs ----------------------------------------------------------------------------------------------------
def test_gpu_cases_contain_what_they_claim():
    cases = {c["name"]: c for c in KC.all_cases()}
    kfs = {n: run_case(c) for n, c in cases.items()}
    assert [s[2].shape[0] for s in cases["ragged"]["scans"]] == [257, 0, 64] and kfs["ragged"]["full"].shape[0] == 321
    assert kfs["ragged"]["counts"].max() >= 2 and not np.array_equal(cases["ragged"]["scans"][0][0], cases["ragged"]["scans"][2][0])
    # a voxel of at least 300 points whose rows straddle the key kernel's workgroup boundary, among single-point voxels
    hv = kfs["heavy_voxel"]
    key = K.voxel_keys(hv["q"], KC.VS)[0]
    big = hv["keys"][np.argmax(hv["counts"])]
    rows = np.flatnonzero(key == big)
    assert hv["counts"].max() >= 300 and rows.min() < KC.KEY_BLOCK <= rows.max() and rows.max() < cases["heavy_voxel"]["scans"][0][2].shape[0]
    assert (hv["counts"] == 1).sum() == hv["counts"].size - 1 and hv["counts"].size > 200
    assert (kfs["distinct"]["counts"] == 1).all() and kfs["distinct"]["down"].shape[0] == kfs["distinct"]["full"].shape[0] == 210
    assert kfs["single_point"]["full"].shape[0] == 1 and kfs["single_point"]["down"].shape[0] == 1
    assert kfs["voxels_1"]["down"].shape[0] == 1 and kfs["voxels_1"]["full"].shape[0] == 3
    assert kfs["voxels_65"]["down"].shape[0] == 65 and kfs["voxels_65"]["counts"].min() >= 2
    # negative coordinates on exact multiples of vs, -0.0, a negative denormal, and the outermost indices +-(2^20 - 1)
    ed = cases["edges"]["scans"][0][2]
    assert np.array_equal(kfs["edges"]["q"][: ed.shape[0]], ed)                      # identity poses: the merged point IS the body point
    x = ed[:, 0]
    assert -KC.VS in x and -2 * KC.VS in x and (x / KC.VS == np.round(x / KC.VS))[x < -1e-3].sum() >= 2
    assert any(v == 0 and np.signbit(v) for v in x) and any(v < 0 and abs(v) < 1e-300 for v in x)
    idx, ok = K.voxel_index(kfs["edges"]["q"], KC.VS)
    assert ok.all() and idx.max() == KC.TOP and idx.min() == -KC.TOP
    # the bad inputs: each is refused for the reason it names
    for name, bad in KC.bad_cases():
        idx, ok = K.voxel_index(bad, KC.VS)
        assert (~ok).sum() == 1, name
    far = dict(KC.bad_cases())
    assert far["index_2^20"][3, 0] / KC.VS == 2.0 ** 20 and far["index_-2^20"][1, 2] / KC.VS == -(2.0 ** 20 - 1) and np.isnan(far["nan"]).sum() == 1
    # the stream the helper test runs has a stationary stretch longer than a window, which makes the rule drop, and an empty scan
    from voxel_slam_amd import synth
    st = synth.make_scanpose_stream(12, 400, 3)
    assert st.stationary[1] > 3 and st.empty >= 0 and st.points[st.empty].shape[0] == 0
    assert all(np.array_equal(st.poses[st.stationary[0]], st.poses[k]) for k in range(st.stationary[0], sum(st.stationary)))
    b = K.KeyframeRef(3)
    actions = []
    for s in st:
        b.push_scan(*s); actions.append(b.action)
    assert actions.count("drop") >= 1 and actions.count("emit") >= 3
    st2 = synth.make_scanpose_stream(12, 400, 3)
    assert all(np.array_equal(a, c) for a, c in zip(st.points, st2.points)) and np.array_equal(st.poses, st2.poses)
