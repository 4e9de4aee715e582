"""CPU suite of the saved-session feature: the file layer (voxel_slam_amd/sessionio.py) against the reference's formats, the numpy checker
(tests/_session_ref.py) against mathematics and literal loops, and the host build of csrc/vxba_session_math.hpp against the checker's bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _session_cases as SC
from tests import _session_ref as S
from voxel_slam_amd import multisession, sessionio as IO, synth, vxba

HERE = os.path.dirname(os.path.abspath(__file__))


def random_states(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([vxba.pack_state(synth.rodrigues(rng.normal(size=3) * (3.0 if k % 3 == 0 else 0.4)), 50 * rng.normal(size=3), rng.normal(size=3),
                                     1e-3 * rng.normal(size=3), 1e-2 * rng.normal(size=3), np.array([0.0, 0.0, -9.8]) + 1e-2 * rng.normal(size=3)) for k in range(n)])


# ---- alidarState.txt ----
def test_lidarstate_round_trip(tmp_path):
    n = 120
    st = random_states(n)
    # rotations by pi about each axis and near them: trace <= 0, every branch of Eigen's rule
    for k, ax in enumerate(np.eye(3)):
        st[k, :9] = synth.rodrigues(np.pi * ax).T.reshape(9)
        st[3 + k, :9] = synth.rodrigues((np.pi - 1e-3) * (ax + 0.1 * np.roll(ax, 1)) / np.linalg.norm(ax + 0.1 * np.roll(ax, 1))).T.reshape(9)
    t = 1.7e9 + 0.1 * np.arange(n) + 1e-7
    v6 = 1e-4 * (1 + np.arange(6 * n).reshape(n, 6) % 7)
    p = str(tmp_path / "alidarState.txt")
    assert IO.write_lidarstate(p, t, st, v6) is True
    lines = open(p).read().splitlines()
    assert len(lines) == n and all(len(ln.split(" ")) == 26 for ln in lines)
    first = lines[0].split(" ")
    assert len(first[0].split(".")[1]) == 6 and all(len(s.split(".")[1]) == 7 for s in first[1:])      # fixed, 6 then 7 decimals
    t2, st2, v62 = IO.read_lidarstate(p)
    assert np.abs(t2 - t).max() <= 5e-7
    assert np.abs(st2[:, 9:] - st[:, 9:]).max() <= 5e-8 and np.abs(v62 - v6).max() <= 5e-8
    assert np.abs(st2[:, :9] - st[:, :9]).max() <= 1e-6


def test_lidarstate_hundred_scan_rule(tmp_path):
    st = random_states(99)
    p = str(tmp_path / "a.txt")
    assert IO.write_lidarstate(p, np.arange(99.0), st, np.zeros(6)) is False and not os.path.exists(p)
    assert IO.write_lidarstate(p, np.arange(100.0), random_states(100), np.zeros(6)) is True and os.path.exists(p)
    assert IO.write_lidarstate(str(tmp_path / "b.txt"), np.arange(3.0), st[:3], np.zeros(6), min_scans=1) is True


def test_lidarstate_short_lines_and_raw_quaternion(tmp_path):
    p = tmp_path / "s.txt"
    nums26 = [12.5, 1, 2, 3, 0.0, 0.0, 0.0, 1.0] + [0.1 * k for k in range(1, 13)] + [1e-4 * k for k in range(1, 7)]
    rows = [nums26[:8], nums26[:20], nums26, [7.0, 0, 0, 0, 0.0, 0.0, 2.0, 0.0]]      # the last: a quaternion of norm 2
    p.write_text("\n".join(" ".join(repr(float(v)) for v in r) for r in rows) + "\n")
    t, st, v6 = IO.read_lidarstate(str(p))
    assert t.tolist() == [12.5, 12.5, 12.5, 7.0] and np.array_equal(st[:3, 9:12], np.tile([1.0, 2.0, 3.0], (3, 1)))
    assert not st[0, 12:].any() and not v6[0].any()                                       # 8 columns: nothing further
    assert np.allclose(st[1, 12:24], nums26[8:20]) and not v6[1].any()                    # 20: the state, no v6
    assert np.allclose(st[2, 12:24], nums26[8:20]) and np.allclose(v6[2], nums26[20:26])  # 26
    assert np.array_equal(st[0, :9].reshape(3, 3), np.eye(3))
    # Quaterniond(w=0, x=0, y=0, z=2).matrix() without normalising: 1 - 2 z^2 = -7 on two diagonal entries
    assert np.array_equal(st[3, :9].reshape(3, 3).T, np.diag([-7.0, -7.0, 1.0]))
    with pytest.raises(ValueError):
        p.write_text("1 2 3\n")
        IO.read_lidarstate(str(p))


def test_quaternion_is_eigens():
    rng = np.random.default_rng(2)
    for k in range(50):
        R = synth.rodrigues(rng.normal(size=3) * (3.1 if k % 2 else 1.0))
        q = IO.quat_from_rot(R)
        assert abs(np.linalg.norm(q) - 1) < 1e-12 and np.abs(IO.rot_from_quat(*q) - R).max() < 1e-12
        i = int(np.argmax(np.diag(R)))
        assert (q[3] > 0) if np.trace(R) > 0 else (q[i] > 0)      # the leading component is the positive root


# ---- PCD ----
def test_pcd_round_trip_is_bit_exact(tmp_path):
    rng = np.random.default_rng(3)
    for n in (0, 1, 1000):
        xyz = (rng.normal(size=(n, 3)) * 30).astype(np.float32)
        p = str(tmp_path / f"{n}.pcd")
        IO.write_pcd(p, xyz)
        raw = open(p, "rb").read()
        head, _, body = raw.partition(b"DATA binary\n")
        assert len(body) == 16 * n and b"FIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n" in head and f"POINTS {n}\n".encode() in head
        got, fields = IO.read_pcd(p, want_fields=True)
        assert got.dtype == np.float32 and got.tobytes() == xyz.tobytes() and not fields["intensity"].any()


def test_pcd_general_header(tmp_path):
    xyz = np.array([[1.5, -2.25, 3.0], [0.1, 0.2, 0.3]], dtype=np.float32)
    # reordered and extra fields, a double, a counted field, binary
    dt = np.dtype([("intensity", "<f4"), ("z", "<f4"), ("ring", "<u2"), ("x", "<f4"), ("time", "<f8"), ("normal", "<f4", (3,)), ("y", "<f4")])
    rec = np.zeros(2, dtype=dt)
    rec["x"], rec["y"], rec["z"], rec["ring"], rec["time"], rec["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], [3, 9], [0.5, 0.75], [7, 8]
    hdr = ("# comment\nVERSION 0.7\nFIELDS intensity z ring x time normal y\nSIZE 4 4 2 4 8 4 4\nTYPE F F U F F F F\nCOUNT 1 1 1 1 1 3 1\nWIDTH 2\nHEIGHT 1\n"
           "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS 2\nDATA binary\n")
    p = tmp_path / "g.pcd"
    p.write_bytes(hdr.encode() + rec.tobytes())
    got, f = IO.read_pcd(str(p), want_fields=True)
    assert got.tobytes() == xyz.tobytes() and f["ring"].tolist() == [3, 9] and f["time"].tolist() == [0.5, 0.75] and f["normal"].shape == (2, 3)
    # ascii body
    p.write_text("VERSION 0.7\nFIELDS y x z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 2\nHEIGHT 1\nPOINTS 2\nDATA ascii\n-2.25 1.5 3\n0.2 0.1 0.3\n")
    assert IO.read_pcd(str(p)).tobytes() == xyz.tobytes()
    p.write_text("VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 2\nHEIGHT 1\nPOINTS 2\nDATA binary_compressed\n")
    with pytest.raises(ValueError, match="binary_compressed"):
        IO.read_pcd(str(p))


# ---- edge.txt ----
def test_edges_inversion_absent_lines_and_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    names = ["a", "b", "c"]
    R = synth.rodrigues(rng.normal(size=3)); tr = rng.normal(size=3) * 5
    q = IO.quat_from_rot(R)
    # written with 7 digits -- what the reference writes -- the quaternion is a unit one to 1e-7 only, and R^T differs from R^-1 by as much; the lines
    # here carry every digit, so that the inversion rule can be held against the composed poses at 1e-12
    num = lambda v: " ".join(repr(float(x)) for x in v)
    lines = [f"a b 3 7 {num(tr)} {num(q)}", f"c a 11 5 {num(tr)} {num(q)}", f"zz a 1 2 {num(tr)} {num(q)}", f"bag b 1 2 {num(tr)} {num(q)}", "", f"b b 4 9 {num(tr)} {num(q)}"]
    p = str(tmp_path / "edge.txt")
    open(p, "w").write("\n".join(lines) + "\n")
    edges, absent = IO.read_edges(p, names, "bag")
    assert absent == [lines[2]] and len(edges) == 3                                   # the running bag's line is neither parsed nor kept
    Rq = IO.rot_from_quat(*q); tq = tr
    e0, e1, e2 = edges
    assert (e0["m1"], e0["m2"], e0["id1"], e0["id2"]) == (0, 1, 3, 7) and np.array_equal(e0["rot"], Rq) and np.array_equal(e0["tra"], tq)
    assert (e1["m1"], e1["m2"], e1["id1"], e1["id2"]) == (0, 2, 5, 11)               # "c a 11 5" inverted
    assert (e2["m1"], e2["m2"]) == (1, 1) and np.all(e0["v6"] == 1e-6)
    # the inversion against composing the poses: X_c^-1 X_a = (X_a^-1 X_c)^-1
    Xa = (synth.rodrigues(rng.normal(size=3)), rng.normal(size=3))
    Xc = (Xa[0] @ Rq.T, Xa[1] - Xa[0] @ Rq.T @ tq)                                    # so that X_c^-1 X_a = (Rq, tq)
    assert np.abs(Xc[0].T @ Xa[0] - Rq).max() < 1e-12 and np.abs(Xc[0].T @ (Xa[1] - Xc[1]) - tq).max() < 1e-12
    assert np.abs(Xa[0].T @ Xc[0] - e1["rot"]).max() < 1e-12 and np.abs(Xa[0].T @ (Xc[1] - Xa[1]) - e1["tra"]).max() < 1e-12
    # into SessionEdges and back out: the absent line first, 7 significant digits, groups in order
    se = multisession.SessionEdges()
    for e in edges:
        se.push(**e)
    out = str(tmp_path / "edge2.txt")
    IO.write_edges(out, names, se, absent)
    wl = open(out).read().splitlines()
    assert wl[0] == lines[2] and wl[2].split()[:4] == ["a", "c", "5", "11"] and len(wl) == 4
    assert wl[1].split() == ["a", "b", "3", "7"] + [f"{x:.7g}" for x in np.concatenate([tr, q])]        # setprecision(7) without fixed
    edges2, absent2 = IO.read_edges(out, names, "bag")
    assert absent2 == absent and len(edges2) == 3
    for a, b in zip(edges, edges2):
        assert (a["m1"], a["m2"], a["id1"], a["id2"]) == (b["m1"], b["m2"], b["id1"], b["id2"])
        assert np.abs(a["rot"] - b["rot"]).max() < 1e-6 and np.abs(a["tra"] - b["tra"]).max() < 1e-5
    IO.write_edges(out, names, edges, absent)
    assert open(out).read().splitlines() == wl                                         # the list form writes the same file


def test_previous_map_names():
    assert IO.parse_previous_maps("a:0.45, #b:0.5, c:0.4") == (["a", "c"], [0.45, 0.4])
    assert IO.parse_previous_maps(" a : 0.45 ,\tc:0.4,") == (["a", "c"], [0.45, 0.4])      # all white space goes, inside names too
    assert IO.parse_previous_maps("a:0.45, broken, c:0.4") == (["a"], [0.45])              # a malformed entry ends the parse
    assert IO.parse_previous_maps("a:1:2, c:0.4") == ([], []) and IO.parse_previous_maps("") == ([], [])
    # the corners of the reference's text: an empty name is a name; a skipped entry's number is never read; stod takes the numeric prefix; a kept
    # entry without one is an error (upstream: an uncaught exception), a missing number is malformed
    assert IO.parse_previous_maps(":0.4, c:0.5") == (["", "c"], [0.4, 0.5])
    assert IO.parse_previous_maps("a:0.45, #b:x, c:0.4") == (["a", "c"], [0.45, 0.4])
    assert IO.parse_previous_maps("a:0.4x, c:1e-1, d:.5") == (["a", "c", "d"], [0.4, 0.1, 0.5])
    assert IO.parse_previous_maps("a:0.45, b:, c:0.4") == (["a"], [0.45])
    with pytest.raises(ValueError, match="is no number"):
        IO.parse_previous_maps("a:0.45, b:x")


def test_session_directory_round_trip(tmp_path):
    c = SC.main_case()
    n = len(c["scans"])
    st = np.concatenate([c["poses"], np.zeros((n, 12))], axis=1)
    d = str(tmp_path / "sess")
    assert IO.save_session(d, c["scans"], np.arange(n) * 0.1, st, 1e-4 * np.ones(6)) is False          # 7 scans: the clouds are there, the state file is not
    assert os.path.exists(os.path.join(d, "6.pcd")) and not os.path.exists(os.path.join(d, IO.STATE_FILE))
    assert IO.save_session(d, c["scans"], np.arange(n) * 0.1, st, 1e-4 * np.ones(6), min_scans=1) is True
    scans, t, st2, v6 = IO.read_session(d)
    assert len(scans) == n and all(a.tobytes() == b.tobytes() for a, b in zip(scans, c["scans"]))
    assert np.abs(st2[:, :12] - c["poses"]).max() < 1e-6 and np.allclose(v6, 1e-4)
    gp = IO.global_path([c["poses"], c["poses"][:2]], [1, 0])
    assert gp.dtype == np.float32 and gp.shape == (2 + n, 4) and gp[:2, 3].tolist() == [1.0, 1.0] and np.array_equal(gp[2:, :3], c["poses"][:, 9:].astype(np.float32))


# ---- the checker against mathematics ----
def test_checker_identity_and_translation():
    rng = np.random.default_rng(6)
    scans = [SC.cloud(50, rng) for _ in range(3)]
    ident = synth.pack_poses(np.stack([np.eye(3)] * 3), np.zeros((3, 3)))
    merged, ids, x0 = S.merge_scans(scans, ident, 3)
    assert ids.tolist() == [2] and merged[0].tobytes() == np.concatenate(scans).tobytes()
    # pure translation: a scan at p_j seen from p_c sits at its points + (p_j - p_c), in double, rounded once
    ps = np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0], [2.0, 2.25, 3.0]])
    tr = synth.pack_poses(np.stack([np.eye(3)] * 3), ps)
    merged, _, x0 = S.merge_scans(scans, tr, 3)
    want = np.concatenate([(s.astype(np.float64) + (ps[j] - ps[2])).astype(np.float32) for j, s in enumerate(scans)])
    assert merged[0].tobytes() == want.tobytes() and np.array_equal(x0[0], tr[2])
    # the filter: every point of a voxel the same -> that point; the mean of two points of one voxel; output sorted by voxel index
    pts = np.array([[0.25, 0.05, 0.05], [-0.05, 0.05, 0.05], [0.25, 0.05, 0.05], [0.01, 0.02, 0.03], [0.03, 0.04, 0.05]], dtype=np.float32)
    down = S.down_sampling_voxel(pts, 0.1)
    assert down.shape == (3, 3) and np.array_equal(down[0], pts[1]) and np.array_equal(down[2], pts[0])
    assert np.array_equal(down[1], ((pts[3] * np.float32(1) + pts[4]) / np.float32(2)))
    assert S.down_sampling_voxel(pts, 0.0005).tobytes() == pts.tobytes()
    with pytest.raises(ValueError):
        S.down_sampling_voxel(np.array([[0.0, 2.0e5, 0.0]], dtype=np.float32), 0.1)
    # the globalmap expression under the identity returns the points; under a translation, points + p
    g = S.globalmap([([pts], [tr[1]], 4)], 100)
    assert g["jump"] == 1 and np.array_equal(g["xyzi"][:, :3], (pts.astype(np.float64) + ps[1]).astype(np.float32)) and np.all(g["xyzi"][:, 3] == 4.0)


def test_window_counts_against_a_literal_loop():
    L = vxba.load_library()
    for Kf in range(0, 40):
        for ac, mg in ((10, 5), (3, 1), (1, 1), (4, 7), (5, 5)):
            n, i = 0, 0
            while i + ac < Kf:
                n += 1; i += mg
            assert len(S.windows(Kf, ac, mg)) == n == L.vxba_session_num_windows(Kf, ac, mg), (Kf, ac, mg)
    assert S.windows(10, 10, 5) == [] and S.windows(11, 10, 5) == [0] and S.windows(5, 3, 1) == [0, 1] and S.windows(3, 3, 1) == []


def test_globalmap_jump_counts_and_chunks_against_a_literal_loop(hm):
    rng = np.random.default_rng(8)
    sizes = [[25, 0, 31, 7], [40, 40], [1, 2, 3, 50, 64]]
    sets = [([SC.cloud(n, rng) for n in sz], SC.poses_for(len(sz), s), 3 - s) for s, sz in enumerate(sizes)]
    for interval in (40, 1, 1000):
        g = S.globalmap(sets, interval)
        psize = sum(sum(sz) for sz in sizes)
        jump = psize // (10 * interval) + 1
        assert g["jump"] == jump == hm.ssh_jump(psize, interval)
        pl, chunks, counts, total = 0, [0], [], 0
        for sz in sizes:
            for n in sz:
                c = len(range(0, n, jump))
                assert c == hm.ssh_count(n, jump)
                counts.append(c); pl += c; total += c
                if pl > interval:
                    chunks.append(total); pl = 0
        chunks.append(total)
        assert g["counts"].tolist() == counts and g["chunk_ptr"].tolist() == chunks and g["xyzi"].shape[0] == total
    assert S.globalmap(sets, 40)["jump"] == 1 and len(S.globalmap(sets, 40)["chunk_ptr"]) > 3
    assert hm.ssh_jump(5 * 10 ** 9, 5 * 10 ** 6) == 101          # 64-bit: upstream's uint would have wrapped to 705032704 / 5e7 + 1 = 15


# ---- the host build of the device header against the checker's bits ----
@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "session_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libsession_hostcheck.so")
    hdrs = [os.path.join(HERE, "..", "voxel-slam_amd", "csrc", h) for h in ("vxba_session_math.hpp", "vxba_keyframe_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS"); f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    L.ssh_move.argtypes = [C.c_int, f64p, f64p, f32p, f32p]
    L.ssh_pose.argtypes = [C.c_int, f64p, f32p, f32p]
    L.ssh_keys.argtypes = [C.c_int, f32p, C.c_double, np.ctypeslib.ndpointer(dtype=np.uint64), np.ctypeslib.ndpointer(dtype=np.uint8)]
    L.ssh_mean.argtypes = [C.c_int, f32p, f32p]
    L.ssh_owner.argtypes = [np.ctypeslib.ndpointer(dtype=np.int64), C.c_longlong, C.c_longlong]
    for f in (L.ssh_owner, L.ssh_jump, L.ssh_count):
        f.restype = C.c_longlong
    L.ssh_jump.argtypes = [C.c_longlong, C.c_longlong]; L.ssh_count.argtypes = [C.c_longlong, C.c_longlong]
    return L


def test_hostcheck_merged_floats_and_map_points(hm):
    rng = np.random.default_rng(9)
    P = SC.poses_for(6, 3)
    for k in range(5):
        pts = np.ascontiguousarray((rng.normal(size=(200, 3)) * 20).astype(np.float32))
        out = np.zeros_like(pts)
        hm.ssh_move(200, P[5], P[k], pts, out)
        assert out.tobytes() == S.move(P[5], P[k], pts).tobytes()
        hm.ssh_pose(200, P[k], pts, out)
        assert out.tobytes() == S.globalmap([([pts], [P[k]], 0)], 10 ** 6)["xyzi"][:, :3].tobytes()


def test_hostcheck_keys_and_range(hm):
    rng = np.random.default_rng(10)
    b = np.arange(-8, 9, dtype=np.float64) * 0.1
    edge = np.concatenate([b, np.nextafter(b.astype(np.float32), np.float32(9)), np.nextafter(b.astype(np.float32), np.float32(-9))]).astype(np.float32)
    far = np.array([104857.5, 104857.7, -104857.5, -104857.7, 104860.0, -104870.0, np.inf, -np.inf, np.nan, 3e38], dtype=np.float32)
    col = np.concatenate([edge, far, (rng.normal(size=300) * 3).astype(np.float32)])
    pts = np.ascontiguousarray(np.stack([col, np.roll(col, 1), np.full_like(col, -0.05)], axis=1))
    n = pts.shape[0]
    key = np.zeros(n, dtype=np.uint64); ok = np.zeros(n, dtype=np.uint8)
    hm.ssh_keys(n, pts, 0.1, key, ok)
    rk, rok = S.voxel_keys_f32(pts, 0.1)
    assert np.array_equal(ok.astype(bool), rok) and np.array_equal(key, rk) and 0 < rok.sum() < n
    # the range is vxba_down_sampling_voxel's: index -2^20 is inside, 2^20 is not
    idx, good = S.voxel_index_f32(np.array([[-104857.55, 0, 0], [104857.6, 0, 0], [104857.55, 0, 0]], dtype=np.float32), 0.1)
    assert idx[0, 0] == -(1 << 20) and good.tolist() == [True, False, True]


def test_hostcheck_mean_and_owner(hm):
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 9, 400):
        rows = np.ascontiguousarray((0.05 + 0.01 * rng.normal(size=(n, 3))).astype(np.float32))      # all in voxel (0, 0, 0) of edge 0.1
        out = np.zeros(3, dtype=np.float32)
        hm.ssh_mean(n, rows, out)
        ref = S.down_sampling_voxel(np.clip(rows, 0.001, 0.099), 0.1)
        hm.ssh_mean(n, np.ascontiguousarray(np.clip(rows, 0.001, 0.099)), out)
        assert ref.shape == (1, 3) and out.tobytes() == ref[0].tobytes()
    ptr = np.array([0, 0, 3, 3, 3, 7, 8, 8], dtype=np.int64)
    owners = [int(hm.ssh_owner(ptr, ptr.size - 1, g)) for g in range(8)]
    assert owners == [1, 1, 1, 4, 4, 4, 4, 5]


def test_cases_contain_what_they_claim():
    c = SC.main_case()
    clouds, ids, x0 = S.build_keyframes(c["scans"], c["poses"], c["win_size"], c["voxel_size"])
    merged, _, _ = S.merge_scans(c["scans"], c["poses"], c["win_size"])
    assert [s.shape[0] for s in c["scans"]][:3] == [300, 0, 1] and ids.tolist() == [2, 5] and len(clouds) == 2
    assert all(0 < cl.shape[0] < m.shape[0] for cl, m in zip(clouds, merged)) and (merged[0] < 0).any() and merged[0].shape[0] + merged[1].shape[0] > 512
    idx, _ = S.voxel_index_f32(merged[1], 0.1)
    assert np.unique(idx, axis=0).shape[0] == clouds[1].shape[0]
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    kidx, _ = S.voxel_index_f32(clouds[1], 0.1)
    assert np.array_equal(kidx, np.unique(idx[order], axis=0))                                          # rows ascend by (x, y, z) voxel index
    assert S.build_keyframes(c["scans"][:2], c["poses"][:2], 3, 1.0)[0] == []                           # fewer scans than win_size: no keyframe
    # the border points and the twins close the group's last scan, so they close the merged cloud: 6 on the borders, 6 + 6 a millionth to either
    # side of them, 2 identical.  After the merge (the relative pose is the identity only up to rounding) the two sides of every border still lie
    # 2e-6 apart and in NEIGHBOURING voxels along x, and the twins are one point twice in one voxel.
    tail, tidx = merged[1][-20:], idx[-20:]
    plus, minus = slice(6, 12), slice(12, 18)
    assert np.all(np.abs(tail[plus, 0] - tail[minus, 0]) < 3e-6) and np.array_equal(tidx[plus, 0], tidx[minus, 0] + 1)
    # a point ON a border goes to either side (upstream's index of a negative whole number is one lower; the merge may round 0 to -0 or 1e-17)
    assert np.all((tidx[:6, 0] == tidx[plus, 0]) | (tidx[:6, 0] == tidx[minus, 0])) and np.array_equal(tidx[3:6, 0], tidx[plus, 0][3:6])
    assert tail[18].tobytes() == tail[19].tobytes() and np.array_equal(tidx[18], tidx[19])
