"""Deterministic inputs of the loop-search tests (tests/test_loopsearch_cpu.py checks every one of them for honesty on the CPU; the GPU tests use
them as they are).

Two kinds.  SESSIONS: a landmark world -- corners at least 2.2 m apart in a corridor box, each with a 50-bit occupancy of 12-24 set bits -- seen by
keyframes along the corridor within a radius, in their own frames, with location noise (sigma 0.01 m) and occupancy bit flips (2 %); the last keyframe
revisits an early one from another heading (or, without a revisit, drives on).  Plane clouds are (centre, normal) rows of a floor / wall lattice seen
within the same radius.  TRIPLES: keyframes made of well separated corner triples; with descriptor_near_num = 3 every triple is exactly one
descriptor, which lets a test place a triangle, its cell, its occupancy and its frame where it wants them.
"""
import numpy as np

from tests import _loopreg_ref as LR
from tests import _loopsearch_ref as S

BOX = (104.0, 10.0, 4.0)
RADIUS = 12.5
N_KEYFRAMES = 25
SESSION_PARAMS = dict(skip_near_num=10)
TRIPLE_SPACING = 100.0


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_axis(axis, a):
    k = np.asarray(axis, dtype=np.float64); k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def random_occupancy(rng, n, bits=50):
    out = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        k = int(rng.integers(12, 25))
        sel = rng.choice(bits, size=k, replace=False)
        out[i] = np.uint64(sum(1 << int(b) for b in sel))
    return out


def flip_bits(rng, occ, p=0.02, bits=50):
    f = rng.random((occ.shape[0], bits)) < p
    m = (f.astype(np.uint64) << np.arange(bits, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    return occ ^ m


def world(seed, n_landmarks=190, length=BOX[0]):
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n_landmarks:
        p = rng.random(3) * np.array([length + 16.0, BOX[1], BOX[2]]) - np.array([8.0, BOX[1] / 2, 0.0])
        if all(np.linalg.norm(p - q) >= 2.2 for q in pts):
            pts.append(p)
    # the lattice of plane rows: floor (z = 0, normal z) and both walls (normal y), 1 m apart, jittered off the lattice so no float32 distance ties
    xs = np.arange(-8.0, length + 8.0, 1.0)
    floor = np.array([(x, y, 0.0, 0, 0, 1.0) for x in xs for y in np.arange(-4.5, 5.0, 1.0)])
    wl = np.array([(x, -5.0, z, 0, 1.0, 0) for x in xs for z in np.arange(0.5, 4.0, 1.0)])
    wr = np.array([(x, 5.0, z, 0, 1.0, 0) for x in xs for z in np.arange(0.5, 4.0, 1.0)])
    ribs = np.array([(x, y, z, 1.0, 0, 0) for x in np.arange(-6.0, length + 8.0, 6.0) for y in (-4.5, -3.5, -2.5, 2.5, 3.5, 4.5) for z in np.arange(0.5, 4.0, 1.0)])
    planes = np.concatenate([floor, wl, wr, ribs])        # ribs across the corridor: without normals along x the ICP's eigenvalue test turns every edge away
    jit = rng.normal(0, 0.05, size=(planes.shape[0], 3))
    jit[planes[:, 5] == 1.0, 2] = 0.0; jit[planes[:, 4] == 1.0, 1] = 0.0; jit[planes[:, 3] == 1.0, 0] = 0.0          # stay in the plane
    planes[:, :3] += jit
    return dict(landmarks=np.array(pts), occupancy=random_occupancy(rng, n_landmarks), planes=planes)


def keyframe_poses(revisit=True, n_keyframes=N_KEYFRAMES):
    """(R (K, 3, 3), p (K, 3)) world <- keyframe.  Keyframe k stands at x = 4 k with a gentle yaw; the last one revisits keyframe 3 from another
    heading and a little tilt, or drives on."""
    Rs, ps = [], []
    for k in range(n_keyframes):
        Rs.append(rot_z(0.05 * np.sin(0.7 * k))); ps.append(np.array([4.0 * k, 0.3 * np.sin(0.4 * k), 1.5]))
    if revisit:
        Rs[-1] = rot_z(2.5) @ rot_axis([1.0, 0.3, 0.0], 0.04); ps[-1] = ps[3] + np.array([0.4, -0.3, 0.1])
    return np.array(Rs), np.array(ps)


def observe(w, R, p, rng, radius=RADIUS):
    """The corners and the plane rows one keyframe sees, in its own frame."""
    d = np.linalg.norm(w["landmarks"] - p, axis=1)
    sel = np.nonzero(d < radius)[0]
    sel = sel[rng.permutation(sel.size)]                                    # the corner list has no world order
    loc = (w["landmarks"][sel] - p) @ R + rng.normal(0, 0.01, size=(sel.size, 3))
    occ = flip_bits(rng, w["occupancy"][sel])
    pl = w["planes"]
    ps = pl[np.linalg.norm(pl[:, :3] - p, axis=1) < radius]
    rows = np.concatenate([(ps[:, :3] - p) @ R, ps[:, 3:] @ R], axis=1).astype(np.float32)
    return loc, occ, rows


def session(seed=5, revisit=True, n_keyframes=N_KEYFRAMES, radius=RADIUS, n_landmarks=190, skip_near_num=SESSION_PARAMS["skip_near_num"]):
    """dict(keyframes: list of (locations, occupancy, plane rows), R, p, params).  The defaults are the tests' session; scripts/run_loop_search.py
    asks for a longer corridor seen from farther."""
    w = world(seed, n_landmarks, 4.0 * (n_keyframes + 1))
    R, p = keyframe_poses(revisit, n_keyframes)
    rng = np.random.default_rng(seed + 1000)
    return dict(keyframes=[observe(w, R[k], p[k], rng, radius) for k in range(n_keyframes)], R=R, p=p, params=S.Params(skip_near_num=skip_near_num))


def pose_records(R, p):
    return np.array([LR.pose_of(R[k], p[k]) for k in range(R.shape[0])])


def true_relative(R, p, i, j):
    """The pose that maps keyframe j's coordinates into keyframe i's."""
    return LR.pose_of(R[i].T @ R[j], R[i].T @ (p[j] - p[i]))


# ---- corner lists with a known answer ----------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def spread(n, seed):
    """n corners with no two float32 distances equal among a corner's nearest (checked by the honesty tests)."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        p = rng.random(3) * np.array([30.0, 12.0, 4.0])
        if all(np.linalg.norm(p - q) >= 2.2 for q in pts):
            pts.append(p)
    return np.array(pts), random_occupancy(rng, n)


def describe_cases():
    """name -> (locations, occupancy, Params)."""
    P = S.Params
    out = {}
    for n in (0, 1, 2, 3, 7, 15, 100):
        loc, occ = spread(n, 40 + n) if n else (np.zeros((0, 3)), np.zeros(0, np.uint64))
        out[f"n{n}"] = (loc, occ, P())
    sq = 10.0 * np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float64)
    out["square"] = (sq, np.array([0xF0F0F, 0xFF00FF, 0x3333333, 0x5555555], np.uint64), P())         # four congruent triangles, one key: KNN ties on purpose
    h = np.sqrt(3.0) / 2
    out["equilateral"] = (np.array([[0, 0, 0], [8.0, 0, 0], [4.0, 8.0 * h, 0]]), np.array([0xFFF, 0xFFF0, 0xFFF00], np.uint64), P())
    out["collinear"] = (np.array([[0, 0, 0], [5.5, 0.3, 0], [12.0, 0, 0], [3.0, 9.0, 1.0]]), np.array([0xFFF, 0xFFF0, 0xFFF00, 0xFFF000], np.uint64), P())
    out["close_pair"] = (np.array([[0, 0, 0], [1.5, 0.2, 0], [7.0, 1.0, 0.5], [3.0, 8.0, 1.0]]), np.array([0xFFF, 0xFFF0, 0xFFF00, 0xFFF000], np.uint64), P())
    return out


TIE_CASES = ("square", "equilateral")       # the inputs built to have float32 KNN ties (equal sides)


def triangle_points(a, b, c):
    """A, B, C in the plane with |AB| = a, |AC| = b, |BC| = c (A shared by the sides a and b)."""
    x = (a * a + b * b - c * c) / (2 * a)
    y = np.sqrt(max(b * b - x * x, 0.0))
    return np.array([[0.0, 0, 0], [a, 0, 0], [x, y, 0]])


def anchors(n):
    g = int(np.ceil(np.sqrt(n)))
    return np.array([(TRIPLE_SPACING * (i % g), TRIPLE_SPACING * (i // g), 0.0) for i in range(n)])


def triple_params(**kw):
    return S.Params(**dict(dict(descriptor_near_num=3, skip_near_num=-1), **kw))


def distinct_shapes(n, seed, lo=4.0, hi=20.0):
    """n scalene triangles (a < b < c, far from collinear) whose descriptors lie at least 4 % apart: a query matches its own copy only.  Every side
    sits 0.15-0.35 of a cell above a cell boundary (resolution 0.2), so the copy's cell is the one the query visits under offset (0, 0, 0): a pair is
    never lost to the 1.5 radius, and a scenario has exactly as many pairs as shapes."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        s = np.sort(rng.uniform(lo, hi, 3))
        s = (np.floor(5.0 * s) + rng.uniform(0.15, 0.35, 3)) / 5.0
        if s[2] > 0.8 * (s[0] + s[1]) or s[1] - s[0] < 0.5 or s[2] - s[1] < 0.5:
            continue
        if all(np.linalg.norm(s - t) > 0.04 * max(np.linalg.norm(s), np.linalg.norm(t)) for t in out):
            out.append(s)
    return out


def triples_keyframe(shapes, seed, where=None, motions=None, occ=None):
    """One corner triple per shape at anchor ``where[k]`` (default: k), randomly oriented (seeded), coordinates exact in float32; ``motions[k]`` =
    (R, t) moves triple k rigidly afterwards.  Returns (locations (3 n, 3), occupancy (3 n,))."""
    rng = np.random.default_rng(seed)
    n = len(shapes)
    an = anchors(max(n, (max(where) + 1) if where is not None else n))
    pts = []
    for k, s in enumerate(shapes):
        Q = rot_axis(rng.normal(size=3), rng.uniform(0, np.pi))
        tri = f32(triangle_points(*s) @ Q.T + an[where[k] if where is not None else k] + rng.uniform(-5, 5, 3))
        if motions is not None and motions[k] is not None:
            tri = tri @ motions[k][0].T + motions[k][1]
        pts.append(tri)
    loc = np.concatenate(pts) if pts else np.zeros((0, 3))
    if occ is None:
        occ = random_occupancy(np.random.default_rng(seed + 7), 3 * n)
    return loc, np.asarray(occ, dtype=np.uint64)


def small_cloud(seed, n=40):
    """A plane cloud of n rows on three orthogonal planes, and the same cloud moved by (R, t)."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        ax = k % 3
        c = rng.uniform(-6, 6, 3); c[ax] = 0.0
        nrm = np.zeros(3); nrm[ax] = 1.0
        rows.append(np.concatenate([c, nrm]))
    return np.array(rows, dtype=np.float32)


def move_cloud(rows, R, t):
    r = np.asarray(rows, dtype=np.float64)
    return np.concatenate([r[:, :3] @ R.T + t, r[:, 3:] @ R.T], axis=1).astype(np.float32)


# ---- scenarios: frames added in order, then one query searched under one or more parameter sets -------------------------------------------
def _occ_common(k, shift=0):
    """20 set bits of which k are among bits 0..19."""
    return np.uint64((((1 << k) - 1) | (((1 << (20 - k)) - 1) << (20 + shift))))


FULL = np.uint64((1 << 20) - 1)
M1 = (rot_axis([0.2, -0.5, 1.0], 0.3), np.array([3.0, -2.0, 1.0]))


def _moved(shapes, seed, motion_of, **kw):
    """The query keyframe and a frame that holds the same triples, triple k moved by motion_of(k)."""
    q = triples_keyframe(shapes, seed, **kw)
    f = triples_keyframe(shapes, seed, motions=[motion_of(k) for k in range(len(shapes))], occ=q[1], **kw)
    return q, f


def scenarios():
    """name -> dict(frames [(locations, occupancy, plane rows)], query (locations, occupancy, plane rows), params [Params, ...])."""
    out = {}
    cloud = small_cloud(3)
    cloud_m = move_cloud(cloud, *M1)
    tp = triple_params
    s0 = (6.2503, 8.0507, 10.2504)            # 5 x the sides: a quarter cell above the cell boundaries; 1000 x the sides: 0.3-0.7 above the key boundaries
    # one cell, three frames: insertion order shows in the match list
    o3, o6 = np.array([FULL] * 3, np.uint64), np.array([FULL] * 6, np.uint64)
    out["one_cell_three_frames"] = dict(frames=[triples_keyframe([(6.2503 + 0.002 * k, 8.0507, 10.2504)], 10 + k, occ=o3) + (cloud,) for k in range(3)], query=triples_keyframe([s0], 20, occ=o3) + (cloud,),
                                        params=[tp()])
    # triangles 0.01 from a cell boundary, and one found through the neighbour cell only
    out["cell_boundary"] = dict(frames=[triples_keyframe([(5.9983, 8.0507, 10.2504), (6.1204, 9.2503, 12.0507)], 30, occ=o6) + (cloud,)], query=triples_keyframe([(6.0023, 8.0507, 10.2504), (6.0904, 9.2503, 12.0507)], 31, occ=o6) + (cloud,),
                                params=[tp()])
    # frame_cur - frame_j == skip_near_num (excluded) and skip_near_num + 1 (included); a negative skip_near_num takes every frame
    out["skip"] = dict(frames=[triples_keyframe([s0], 40 + k, occ=o3) + (cloud,) for k in range(4)], query=triples_keyframe([s0], 45, occ=o3) + (cloud,), params=[tp(skip_near_num=2), tp(skip_near_num=-3)])
    # similarity just above and just below the threshold: (0.75 + 0.7 + 0.7) / 3 and (0.7 + 0.7 + 0.65) / 3 against 0.7
    sa, sb = (6.2503, 8.0507, 10.2504), (7.6506, 11.2503, 14.8507)
    qocc = np.array([FULL] * 6, np.uint64)
    focc = np.array([_occ_common(15), _occ_common(14), _occ_common(14), _occ_common(14), _occ_common(14), _occ_common(13)], np.uint64)
    out["similarity"] = dict(frames=[triples_keyframe([sa, sb], 50, occ=focc) + (cloud,)], query=triples_keyframe([sa, sb], 51, occ=qocc) + (cloud,), params=[tp()])
    # votes: frame 0 and 2 tie at 5 (the lower first), frame 1 has 4 (never a candidate), frame 3 has 6; candidate_num 2 of three eligible
    sh = distinct_shapes(6, 60)
    q, full = _moved(sh, 61, lambda k: M1)
    def part(ks):
        idx = np.concatenate([np.arange(3 * k, 3 * k + 3) for k in ks])
        return full[0][idx], full[1][idx], cloud_m
    out["votes"] = dict(frames=[part(range(0, 5)), part(range(0, 4)), part(range(1, 6)), part(range(0, 6))], query=q + (cloud,), params=[tp(candidate_num=2), tp()])
    # verify: skip_len 1, 2, 2, 3
    for M in (49, 50, 51, 101):
        q, f = _moved(distinct_shapes(M, 70 + M), 80 + M, lambda k: M1)
        out[f"verify_{M}"] = dict(frames=[f + (cloud_m,)], query=q + (cloud,), params=[tp()])
    # max vote 3 (score -1), max vote 4, and two hypotheses with equal votes (the first wins)
    def other(j):
        return (M1[0], M1[1] + np.array([12.0 * (j + 1), 0.0, 0.0]))
    sh5, sh8 = distinct_shapes(5, 90), distinct_shapes(8, 91)
    q, f = _moved(sh5, 92, lambda k: M1 if k < 3 else other(k))
    out["max_vote_3"] = dict(frames=[f + (cloud_m,)], query=q + (cloud,), params=[tp()])
    q, f = _moved(sh5, 93, lambda k: M1 if k != 1 else other(0))
    out["max_vote_4"] = dict(frames=[f + (cloud_m,)], query=q + (cloud,), params=[tp()])
    q, f = _moved(sh8, 94, lambda k: M1 if k % 2 == 0 else other(0))
    out["equal_votes"] = dict(frames=[f + (cloud_m,)], query=q + (cloud,), params=[tp()])
    return out


def session_scenario(revisit=True, seed=5):
    s = session(seed, revisit)
    return dict(frames=s["keyframes"][:-1], query=s["keyframes"][-1], params=[s["params"]], R=s["R"], p=s["p"])


def run_checker(sc, perturb=0.0):
    """dict(described: the checker's descriptors of every frame and of the query, searches: one result per parameter set, db)."""
    prm = sc["params"][0]
    db = S.Database()
    described = []
    for loc, occ, rows in sc["frames"]:
        d = S.describe(loc, occ, prm, perturb)
        described.append(d)
        db.add(d, rows)
    loc, occ, rows = sc["query"]
    d = S.describe(loc, occ, prm, perturb)
    described.append(d)
    return dict(described=described, searches=[db.search(d, rows, p, perturb) for p in sc["params"]], db=db)
