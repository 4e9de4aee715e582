"""CPU half of the loop search's tests: the checker (tests/_loopsearch_ref.py) against mathematics, the device header
(csrc/vxba_loopsearch_math.hpp) compiled for the host against the checker, and the honesty of every input the GPU tests use."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import _loopreg_ref as LR
from tests import _loopsearch_cases as K
from tests import _loopsearch_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")

# An integer or a verdict of the device and of the checker can differ only where a real-valued argument lies within the scatter of two float64
# evaluation orders (~1e-15 relative) of a truncation boundary or a threshold.  The GPU tests compare for EQUALITY, so every input they use must
# give the same integers and verdicts with every such argument moved by RELATIVE either way -- six orders above the scatter -- and keep every
# distance against 3.0 and every gate quantity of the score DECISIVE away: conditions on the inputs, not tolerances.
RELATIVE = 1e-9
DECISIVE = 1e-6


@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "loopsearch_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libloopsearch_hostcheck.so")
    hdr = os.path.join(HERE, "..", "voxel-slam_amd", "csrc", "vxba_loopsearch_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.lsh_triangles.argtypes = [C.c_int, f32p, f32p, f32p, C.c_double, C.c_double, u8p, f64p, i64p, i32p]
    L.lsh_cells.argtypes = [C.c_int, f64p, i32p, i32p, f64p]
    L.lsh_similarity.argtypes = [C.c_int, u64p, u64p, f64p]
    L.lsh_pose.argtypes = [C.c_int, f64p, f64p, f64p, f64p, f64p]
    L.lsh_votes.argtypes = [C.c_int, f64p, f64p, f64p, C.c_double, u8p]
    return L


@functools.lru_cache(maxsize=None)
def session_run(revisit):
    """The checker over a whole session, keyframe by keyframe: (scenario, descriptors, search result per keyframe)."""
    sc = K.session_scenario(revisit)
    prm = sc["params"][0]
    db = S.Database()
    ds, rs = [], []
    for loc, occ, rows in list(sc["frames"]) + [sc["query"]]:
        d = S.describe(loc, occ, prm)
        rs.append(db.search(d, rows, prm)); ds.append(d)
        db.add(d, rows)
    return sc, ds, rs


# ---- the checker against mathematics --------------------------------------------------------------------------------------------------------
def test_descriptors_are_invariant_under_a_rigid_motion_exact_in_float32():
    rng = np.random.default_rng(1)
    pts = []
    while len(pts) < 40:                                               # multiples of 1/64 below 64: exact in float32, and so is every image below
        p = np.round(rng.random(3) * np.array([40.0, 20.0, 6.0]) * 64) / 64
        if all(np.linalg.norm(p - q) >= 2.2 for q in pts):
            pts.append(p)
    loc = np.array(pts); occ = K.random_occupancy(rng, 40)
    a = S.describe(loc, occ)
    assert a["triangle"].shape[0] > 500 and a["knn_ties"] == 0
    for R, t in ((np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([100.0, -7.0, 3.0])), (np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]), np.array([-50.0, 20.0, 0.5]))):
        moved = loc @ R.T + t
        assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)
        b = S.describe(moved, occ)
        assert np.array_equal(a["corners"], b["corners"]) and np.array_equal(a["key"], b["key"]) and np.array_equal(a["cell"], b["cell"])
        assert np.array_equal(a["triangle"], b["triangle"])            # differences of exact coordinates are permuted and negated, nothing else
        assert np.allclose(b["centre"], a["centre"] @ R.T + t, rtol=0, atol=1e-12)
    perm = rng.permutation(40)                                         # a relabelling of the corners relabels the descriptors' corners and reorders the list
    c = S.describe(loc[perm], occ[perm])
    assert sorted(map(tuple, np.sort(a["key"], axis=1).tolist())) == sorted(map(tuple, np.sort(c["key"], axis=1).tolist()))


def test_vertex_assignment_and_sorting():
    # sides given as (|p1 p2|, |p1 p3|, |p2 p3|): A is shared by the two shortest, C by the two longest
    a, b, c, v = S.sort_sides(np.array([5.0, 3.0, 4.0, 4.0]), np.array([3.0, 4.0, 4.0, 4.0]), np.array([4.0, 5.0, 3.0, 4.0]))
    assert (a.tolist(), b.tolist(), c.tolist()) == ([3.0, 3.0, 3.0, 4.0], [4.0, 4.0, 4.0, 4.0], [5.0, 5.0, 4.0, 4.0])
    # (5, 3, 4): a = |p1 p3|, b = |p2 p3|, c = |p1 p2| -> A = p3, B = p1, C = p2
    assert v[0].tolist() == [2, 0, 1]
    assert v[1].tolist() == [0, 1, 2]                                  # already sorted: A = p1 (a, b), B = p2 (a, c), C = p3 (b, c)
    assert v[3].tolist() == [0, 1, 2]                                  # equal sides: no swap (strict >), the reference's assignment
    assert v[2].tolist() == [1, 2, 0]                                  # (4, 4, 3): b <-> c, then a <-> b: a = |p2 p3|, b = |p1 p2|, c = |p1 p3| -> A = p2, B = p3, C = p1
    for row, sides in zip(v, ((5.0, 3.0, 4.0), (3.0, 4.0, 5.0), (4.0, 4.0, 3.0))):
        ends = {0: {0, 1}, 1: {0, 2}, 2: {1, 2}}                       # the vertices of |p1 p2|, |p1 p3|, |p2 p3|
        order = np.argsort(np.array(sides), kind="stable")
        if len(set(sides)) == 3:
            sa, sb, sc_ = (ends[int(k)] for k in order)
            assert row.tolist() == [(sa & sb).pop(), (sa & sc_).pop(), (sb & sc_).pop()]


def test_recovered_rotation_equals_the_applied_one_for_noise_free_triangles():
    rng = np.random.default_rng(2)
    n = 200
    sl = rng.uniform(-20, 20, (n, 3, 3))
    sc = sl.mean(axis=1)
    worst = 0.0
    poses_true = []
    rl = np.zeros_like(sl); rc = np.zeros_like(sc)
    for k in range(n):
        R = K.rot_axis(rng.normal(size=3), rng.uniform(0, np.pi)); t = rng.uniform(-30, 30, 3)
        rl[k] = sl[k] @ R.T + t; rc[k] = sc[k] @ R.T + t
        poses_true.append(LR.pose_of(R, t))
    got = S.kabsch(sl, sc, rl, rc)
    for k in range(n):
        worst = max(worst, *LR.pose_diff(got[k], poses_true[k]))
    assert worst < 1e-11, worst
    R = got[:, :9].reshape(n, 3, 3).transpose(0, 2, 1)
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-12)


def test_first_max_and_ordering_rules_on_hand_built_votes():
    assert S.select_candidates([0, 7, 5, 7, 4, 9], 20) == [(5, 9), (1, 7), (3, 7), (2, 5)]          # votes descending, frame ascending, >= 5 only
    assert S.select_candidates([0, 7, 5, 7, 4, 9], 2) == [(5, 9), (1, 7)]
    assert S.select_candidates([4, 4, 4], 20) == [] and S.select_candidates([], 3) == []
    assert S.first_max([3, 9, 9, 2]) == (1, 9) and S.first_max([0, 0, 0]) == (0, 0) and S.first_max([4]) == (0, 4)
    assert [M // (M // 50 + 1) for M in (49, 50, 51, 101)] == [49, 25, 25, 33] and [M // 50 + 1 for M in (49, 50, 51, 101)] == [1, 2, 2, 3]


def test_similarity_values_and_the_empty_word():
    full = K.FULL
    p = np.array([[full, full, full], [full, full, full], [0, full, full]], np.uint64)
    q = np.array([[K._occ_common(15), K._occ_common(14), K._occ_common(14)], [K._occ_common(14), K._occ_common(14), K._occ_common(13)], [0, full, full]], np.uint64)
    s = S.similarity(p, q)
    assert abs(s[0] - 2.15 / 3) < 1e-15 and abs(s[1] - 2.05 / 3) < 1e-15 and np.isnan(s[2])
    assert not (s[2] > 0.7)                                            # 0 / 0 is no match


# ---- the device header on the host against the checker -------------------------------------------------------------------------------------
def test_host_sides_keys_and_vertices_equal_the_checkers(hm):
    rng = np.random.default_rng(3)
    n = 20000
    p1 = rng.uniform(-40, 40, (n, 3)).astype(np.float32); p2 = (p1 + rng.uniform(-12, 12, (n, 3))).astype(np.float32); p3 = (p1 + rng.uniform(-12, 12, (n, 3))).astype(np.float32)
    p3[:50] = p2[:50] + np.float32(0.5) * (p2[:50] - p1[:50])          # near-collinear
    p2[50:60] = p1[50:60]                                               # a zero side
    ok = np.zeros(n, np.uint8); sides = np.zeros((n, 3)); keys = np.zeros((n, 3), np.int64); v = np.zeros((n, 3), np.int32)
    hm.lsh_triangles(n, p1, p2, p3, 2.0, 50.0, ok, sides, keys, v)
    a, b, c = S.side(p1, p2), S.side(p1, p3), S.side(p3, p2)
    good = ~((a > 50.0) | (b > 50.0) | (c > 50.0) | (a < 2.0) | (b < 2.0) | (c < 2.0))
    a, b, c, vv = S.sort_sides(a, b, c)
    good &= ~(np.abs(c - (a + b)) < 0.2)
    assert np.array_equal(sides, np.stack([a, b, c], axis=1)) and np.array_equal(v, vv)
    assert np.array_equal(ok.astype(bool), good) and good.sum() > 1000 and (~good).sum() > 100       # both verdicts well represented
    assert np.array_equal(keys, np.stack([(s * 1000.0).astype(np.float32).astype(np.int64) for s in (a, b, c)], axis=1))


def test_host_cells_and_similarity_equal_the_checkers(hm):
    rng = np.random.default_rng(4)
    n = 5000
    tri = rng.uniform(10.0, 250.0, (n, 3)); tri[:100] = np.round(tri[:100]) + rng.choice([0.49999, 0.5, 0.50001, 0.0, 1e-12], (100, 3))
    add = np.zeros((n, 3), np.int32); query = np.zeros((n, 27, 3), np.int32); dist = np.zeros((n, 27))
    hm.lsh_cells(n, tri, add, query, dist)
    inc = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], dtype=np.float64)
    cell = (tri[:, None, :] + inc[None]).astype(np.int64)
    assert np.array_equal(add, (tri + 0.5).astype(np.int64)) and np.array_equal(query, cell)
    assert np.array_equal(dist, S.norm3(tri[:, None, :] - (cell.astype(np.float64) + 0.5)))
    p = rng.integers(0, 1 << 50, (n, 3), dtype=np.uint64); q = p ^ rng.integers(0, 1 << 50, (n, 3), dtype=np.uint64) & rng.integers(0, 1 << 50, (n, 3), dtype=np.uint64)
    p[:5] = 0; q[:5] = 0
    s = np.zeros(n)
    hm.lsh_similarity(n, np.ascontiguousarray(p), np.ascontiguousarray(q), s)
    assert np.array_equal(s, S.similarity(p, q), equal_nan=True) and np.isnan(s[:5]).all()


def test_host_pose_agrees_with_the_checkers_svd_to_rounding(hm):
    """The closed form of triangle_pose against numpy.linalg.svd, on the pairs the session's candidates are verified with (noisy, not congruent) and on
    mirrored pairs, where the sign fix on the smallest singular direction decides."""
    sc, ds, rs = session_run(True)
    res = rs[-1]
    d = ds[-1]
    # rebuild the database to reach the entries of the matches
    db = S.Database()
    for dd, (_, _, rows) in zip(ds[:-1], sc["frames"]):
        db.add(dd, rows)
    rows_, g, _ = db.matches(d, sc["params"][0])
    q = rows_[:, 0]
    sl, scn, rl, rcn = d["loc"][q], d["centre"][q], db.loc[g], db.ctr[g]
    rng = np.random.default_rng(5)
    sel = rng.choice(q.shape[0], 2000, replace=False)
    sl, scn, rl, rcn = (np.ascontiguousarray(x[sel]) for x in (sl, scn, rl, rcn))
    rl_m = rl.copy(); rl_m[:, :, 2] *= -1.0; rc_m = rcn.copy(); rc_m[:, 2] *= -1.0       # a mirrored reference: det(V U^T) < 0 before the fix
    worst = 0.0
    for a, b, c, e in ((sl, scn, rl, rcn), (sl, scn, np.ascontiguousarray(rl_m), np.ascontiguousarray(rc_m))):
        n = a.shape[0]
        P = np.zeros((n, 12))
        hm.lsh_pose(n, a.reshape(n, 9), b, c.reshape(n, 9), e, P)
        want = S.kabsch(a, b, c, e)
        for k in range(n):
            worst = max(worst, *LR.pose_diff(P[k], want[k]))
        ok = np.zeros(n, np.uint8)
        hm.lsh_votes(n, np.ascontiguousarray(P[0]), a.reshape(n, 9), c.reshape(n, 9), 3.0, ok)
        R = want[0, :9].reshape(3, 3).T
        dist = S.norm3((a @ R.T + want[0, 9:]) - c)
        assert np.abs(dist - 3.0).min() > DECISIVE and np.array_equal(ok.astype(bool), (dist < 3.0).all(axis=1))
    print(f"closed form against svd: at most {worst:.3e} (m, rad)")
    assert worst < 1e-10, worst
    bad = np.zeros(12)
    hm.lsh_pose(1, np.zeros(9), np.zeros(3), np.zeros(9), np.zeros(3), bad)             # a degenerate triangle: not finite, votes 0
    ok = np.ones(1, np.uint8)
    hm.lsh_votes(1, bad, np.zeros(9), np.zeros(9), 3.0, ok)
    assert not np.isfinite(bad).all() and ok[0] == 0


# ---- honesty: every input of the GPU tests ----------------------------------------------------------------------------------------------------
INT_FIELDS = ("corners", "key", "cell")


def same_descriptors(a, b):
    return a["triangle"].shape == b["triangle"].shape and all(np.array_equal(a[k], b[k]) for k in INT_FIELDS)


def same_search(a, b):
    if not (np.array_equal(a["matches"], b["matches"]) and a["visited"] == b["visited"] and a["frame"] == b["frame"] and len(a["candidates"]) == len(b["candidates"])):
        return False
    return all(all(x[k] == y[k] for k in ("frame", "votes", "pairs", "hypotheses", "best", "max_vote", "useful")) for x, y in zip(a["candidates"], b["candidates"]))


def test_honesty_describe_inputs():
    for name, (loc, occ, prm) in K.describe_cases().items():
        base = S.describe(loc, occ, prm)
        for e in (RELATIVE, -RELATIVE):
            assert same_descriptors(base, S.describe(loc, occ, prm, e)), name
        assert (base["knn_ties"] == 0) == (name not in K.TIE_CASES), name              # float32 KNN ties only in the inputs built to have them


@pytest.mark.parametrize("name", sorted(K.scenarios()))
def test_honesty_scenarios(name):
    sc = K.scenarios()[name]
    base = K.run_checker(sc)
    assert sum(d["knn_ties"] for d in base["described"]) == 0
    for e in (RELATIVE, -RELATIVE):
        other = K.run_checker(sc, e)
        assert all(same_descriptors(a, b) for a, b in zip(base["described"], other["described"]))
        assert all(same_search(a, b) for a, b in zip(base["searches"], other["searches"]))
    for s in base["searches"]:
        for c in s["candidates"]:
            assert c["margin"] >= DECISIVE and c["ties"] == 0, (name, c["frame"], c["margin"])


@pytest.mark.parametrize("revisit", [True, False])
def test_honesty_sessions(revisit):
    sc, ds, rs = session_run(revisit)
    prm = sc["params"][0]
    assert sum(d["knn_ties"] for d in ds) == 0
    frames = list(sc["frames"]) + [sc["query"]]
    assert [r["frame"] for r in rs[:-1]] == [-1] * (K.N_KEYFRAMES - 1)                   # nothing is found before the last keyframe ...
    assert all(len(r["candidates"]) == 0 for r in rs[:-1])
    assert rs[-1]["frame"] == (3 if revisit else -1)                                      # ... which finds the keyframe it revisits, or nothing
    for e in (RELATIVE, -RELATIVE):
        db = S.Database()
        for k, (loc, occ, rows) in enumerate(frames):
            d = S.describe(loc, occ, prm, e)
            assert same_descriptors(ds[k], d), k
            if k in (5, K.N_KEYFRAMES - 1):                                               # the searches the GPU tests look into
                assert same_search(rs[k], db.search(d, rows, prm, e)), k
            db.add(d, rows)
    for c in rs[-1]["candidates"]:
        assert c["margin"] >= DECISIVE and c["ties"] == 0, (c["frame"], c["margin"])
    if revisit:
        c = rs[-1]["candidates"][0]
        assert c["frame"] == 3 and c["max_vote"] > 0.9 * c["pairs"]
        dt, dr = LR.pose_diff(rs[-1]["pose"], K.true_relative(sc["R"], sc["p"], 3, K.N_KEYFRAMES - 1))
        assert dt < 0.5 and dr < 0.1
        scores = [x["score"] for x in rs[-1]["candidates"]]
        assert scores[0] > max(scores[1:]), scores                                         # strictly greatest: SearchLoop's choice does not hang on an order
