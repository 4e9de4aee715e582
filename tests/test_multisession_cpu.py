"""The multi-session loop closure on the CPU: ``SessionEdges``, the checker of the search over several databases, and the policy of
``voxel_slam_amd.multisession.MultiSession`` -- run through scripted stand-ins for the search, the registration and the pose graph -- against the
literal restatement of thd_loop_closure / PGO_Edges / build_graph in tests/_multisession_ref.py.

The scripted streams put every compared quantity at least 1e-6 (relative) from its threshold; that margin is asserted on the RESTATEMENT's record, so
the checker alone satisfies it and the equality of the two records is a fair demand.  Floats of the two records are compared to 1e-9 relative: the two
runs add their factors in different orders, so their optimised poses (and the drifts measured from them) differ in the last bits.
"""
import dataclasses

import numpy as np
import pytest

from tests import _loopreg_ref as LR
from tests import _loopsearch_cases as K
from tests import _loopsearch_ref as S
from tests import _multisession_cases as MC
from tests import _multisession_ref as MR
from tests import _pgo_ref as PG
from voxel_slam_amd import multisession
from voxel_slam_amd.multisession import SessionEdges

I3, Z3, V6 = np.eye(3), np.zeros(3), np.full(6, 1e-4)


# ---- SessionEdges ------------------------------------------------------------------------------------------------------------------------
def chain_edges():
    e, lit = SessionEdges(), MR.PGO_Edges()
    for m1, m2 in ((0, 1), (1, 2), (3, 3)):
        for x in (e, lit):
            x.push(m1, m2, 4, 5, K.rot_z(0.1 * (m1 + 1)), np.array([1.0, m1, m2]), V6)
    return e, lit


@pytest.mark.parametrize("root", [0, 1, 2, 3, 4])
def test_connect_on_a_chain_and_an_isolated_session(root):
    e, lit = chain_edges()
    want = []
    lit.connect(root, want)
    assert e.connect(root) == want == ([0, 1, 2] if root < 3 else [root])
    assert e.mates == lit.mates


def test_connect_visits_in_insertion_order_and_sorts():
    e, lit = SessionEdges(), MR.PGO_Edges()
    for m1, m2 in ((2, 5), (0, 5), (0, 3), (3, 4), (1, 1)):
        for x in (e, lit):
            x.push(m1, m2, 0, 0, I3, Z3, V6)
    for root in range(7):
        want = []
        lit.connect(root, want)
        assert e.connect(root) == want
    assert e.connect(5) == [0, 2, 3, 4, 5] and e.connect(1) == [1] and e.mates == lit.mates


def test_a_pair_pushed_twice_is_one_group():
    e = SessionEdges()
    e.push(0, 2, 1, 7, I3, Z3, V6)
    e.push(1, 2, 3, 8, I3, Z3, V6)
    e.push(0, 2, 2, 9, K.rot_z(0.2), np.ones(3), V6)
    assert [(g["m1"], g["m2"], g["ids1"], g["ids2"]) for g in e.edges] == [(0, 2, [1, 2], [7, 9]), (1, 2, [3], [8])]
    assert e.mates == [[2], [2], [0, 1]] and e.to_arrays()["ids"].shape == (3, 2)
    e.push(2, 0, 5, 5, I3, Z3, V6)                  # the ORDERED pair: (2, 0) is another group, and another pair of mates
    assert len(e.edges) == 3 and e.mates == [[2, 2], [2], [0, 1, 0]]


def test_adapt():
    e, lit = chain_edges()
    for ids in ([0, 1, 2], [1, 2], [0, 2], [2, 1, 0], [3], [], [0, 1, 1]):
        for g, l in zip(e.edges, lit.edges):
            step = [0, 0]
            want = tuple(step) if l.is_adapt(ids, step) else None
            assert SessionEdges.adapt(g, ids) == want
    assert SessionEdges.adapt(e.edges[0], [0, 1, 2]) == (0, 1) and SessionEdges.adapt(e.edges[1], [0, 2]) is None and SessionEdges.adapt(e.edges[2], [3]) == (0, 0)


def test_array_round_trip():
    e = SessionEdges()
    rng = np.random.default_rng(1)
    for m1, m2 in ((0, 2), (1, 2), (0, 2), (2, 2), (1, 2)):
        e.push(m1, m2, int(rng.integers(50)), int(rng.integers(50)), K.rot_axis(rng.normal(size=3), 0.3), rng.normal(size=3), rng.uniform(1e-6, 1e-3, 6))
    a = e.to_arrays()
    assert all(isinstance(v, np.ndarray) and v.dtype in (np.int64, np.float64) for v in a.values())
    assert a["pairs"].tolist() == [[0, 2], [1, 2], [2, 2]] and a["ptr"].tolist() == [0, 2, 4, 5] and a["rot"].shape == (5, 9)
    b = SessionEdges.from_arrays(a)
    assert b.mates == e.mates and b.connect(0) == e.connect(0)
    for x, y in zip(b.to_arrays().values(), a.values()):
        assert np.array_equal(x, y)
    empty = SessionEdges.from_arrays(SessionEdges().to_arrays())
    assert empty.edges == [] and empty.connect(3) == [3]


# ---- the checker of the search over several databases --------------------------------------------------------------------------------------
class Stamped(S.Database):
    """BTC.cpp:1184-1186 across managers, stated directly: while the match list is made, the frame number the searched manager's entries are compared
    with is the one the CURRENT manager stamped on the query."""

    def __init__(self, db, stamp):
        self.__dict__.update(db.__dict__)
        self.stamp, self.matching = stamp, False

    @property
    def num_frames(self):
        return self.stamp if self.matching else len(self.clouds)

    def matches(self, d, prm, perturb=0.0):
        self.matching = True
        try:
            return super().matches(d, prm, perturb)
        finally:
            self.matching = False


def strip(r):
    return dict(frame=r["frame"], score=r["score"], pose=r["pose"].tolist(), matches=r["matches"].tolist(),
                candidates=[{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in c.items()} for c in r["candidates"]])


@pytest.mark.parametrize("case", list(MC.CASES))
def test_checker_search_multi_is_database_search_under_the_skip_identity(case):
    names, skips, _, p = MC.CASES[case]
    dbs, d = MC.describe_all(p)
    cf = MC.cur_frames(case, dbs)
    rows = MC.world()["query"][2]
    got = MR.search_multi([dbs[n] for n in names], d, rows, cf, skips, p)
    voff = 0
    for s, n in enumerate(names):
        direct = Stamped(dbs[n], cf).search(d, rows, dataclasses.replace(p, skip_near_num=skips[s]))
        assert strip(got["sessions"][s]) == strip(direct)
        part = got["matches"][got["offsets"][s]:got["offsets"][s + 1]]
        assert np.array_equal(part[:, [0, 2]], direct["matches"][:, [0, 2]]) and np.array_equal(part[:, 1] - voff, direct["matches"][:, 1])
        voff += dbs[n].num_frames
    longer = [n for n in names if dbs[n].num_frames > cf]
    shorter = [n for n in names if 0 < dbs[n].num_frames < cf]
    if case == "shorter_current":
        assert longer and got["sessions"][0]["matches"].shape[0] < 20           # frames 2 and 3 of "votes" are too new for a current handle of one frame
    if case == "skip_equal_and_one_more":
        assert shorter == ["skip", "skip", "votes"]


@pytest.mark.parametrize("candidate_num", [1, 20])
def test_honesty_of_the_union_query(candidate_num):
    """No integer and no verdict of the checker moves under a relative perturbation of 1e-9; every verify distance and every gate of the score keeps 1e-6."""
    p = MC.params(candidate_num=candidate_num)
    rows = MC.world()["query"][2]
    runs = []
    for eps in (0.0, 1e-9, -1e-9):
        dbs, d = MC.describe_all(p, eps)
        runs.append({n: db.search(d, rows, dataclasses.replace(p, skip_near_num=MC.ALL), eps) for n, db in dbs.items()})
        assert d["knn_ties"] == 0
    ints = lambda r: (r["frame"], r["matches"].tolist(), [(c["frame"], c["votes"], c["hypotheses"], c["best"], c["max_vote"], c["useful"], list(c["hyp_votes"])) for c in r["candidates"]])
    for n in runs[0]:
        assert ints(runs[0][n]) == ints(runs[1][n]) == ints(runs[2][n])
        for c in runs[0][n]["candidates"]:
            assert c["margin"] >= 1e-6 and c["ties"] == 0


# ---- the policy against the restatement -------------------------------------------------------------------------------------------------------
def pose_at(i, lane=0.0):
    """Scan i of a drive along x, two metres a scan, with a slow yaw."""
    return LR.pose_of(K.rot_z(0.01 * i), np.array([2.0 * i, lane, 0.0]))


def guess_for(xx, xc, drift):
    """The registered pose (current -> matched frame) that puts the current scan ``drift`` (a vector) from where it stands: drift_p = |drift|."""
    Rx, Rc = xx[:9].reshape(3, 3).T, xc[:9].reshape(3, 3).T
    return LR.pose_of(Rx.T @ Rc, Rx.T @ (xc[9:] + np.asarray(drift, dtype=np.float64) - xx[9:]))


class Product:
    def __init__(self, imported, **policy):
        self.plan, self.reject = {}, set()
        search_cls, reg_cls = MR.scripted(self.plan, self.reject)
        self.ms = multisession.MultiSession(search_cls=search_cls, reg_cls=reg_cls, graph_cls=PG.RefPoseGraph, **policy)
        for frames, poses, v6, jud in imported:
            self.ms.import_session(frames, poses, v6, jud)
        self.reg = self.ms.reg

    def pose(self, sid, scan):
        return self.ms.sessions[sid].poses[scan]

    def cloud(self, sid, frame):
        return self.ms.sessions[sid].cloud_ids[frame]

    def frames(self):
        return self.ms.current.search.num_frames()

    cur_id = property(lambda self: self.ms.cur_id)
    scan = lambda self, x, v6: self.ms.push_scan(x, v6)
    key = lambda self, cloud, step: self.ms.push_keyframe((None, None), cloud, jour_step=step)
    reset = lambda self: self.ms.new_session()
    state = lambda self: dict(jours=[s.jour for s in self.ms.sessions], relc=[s.relc_count for s in self.ms.sessions], g_update=self.ms.g_update)

    def graph(self):
        return self.ms.graph_factors()

    def build(self):
        self.ms.build_graph(1)
        return self.ms.ids, self.ms.stepsizes


class Restated:
    def __init__(self, imported, **policy):
        self.plan, self.reject = {}, set()
        search_cls, reg_cls = MR.scripted(self.plan, self.reject)
        self.reg = reg_cls()
        self.lit = MR.Literal(search_cls, self.reg, imported=imported, **policy)

    def pose(self, sid, scan):
        return self.lit.multimap_scanPoses[sid][scan].x

    def cloud(self, sid, frame):
        return self.lit.std_managers[sid].cloud_ids[frame]

    def frames(self):
        return self.lit.std_manager.num_frames()

    cur_id = property(lambda self: len(self.lit.std_managers) - 1)
    scan = lambda self, x, v6: self.lit.push_scan(x, v6)
    key = lambda self, cloud, step: self.lit.push_keyframe((None, None), cloud, step)
    reset = lambda self: self.lit.reset()
    state = lambda self: dict(jours=[float(j) for j in self.lit.jours], relc=list(self.lit.relc_counts), g_update=self.lit.g_update)

    def graph(self):
        be, pr = self.lit.flat_graph()
        return be, [(n, x, v) for n, x, v in pr]

    def build(self):
        self.lit.build_graph(self.cur_id, 1)
        return self.lit.ids, self.lit.stepsizes


def imported_session(n_frames, lane, jud=None):
    """A session of 2 n_frames scans whose keyframe k was made at scan 2 k + 1."""
    return ([((None, None), np.zeros((1, 6), np.float32), 2 * k + 1) for k in range(n_frames)], np.array([pose_at(i, lane) for i in range(2 * n_frames)]),
            np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]), jud)


def drive(runner, stream, lane):
    """stream: ("key", jour_step, [(session, frame, score, drift, accepted)]) -- two scans, then the keyframe with the scripted answers -- or ("reset",).
    Returns the records and the state after every keyframe."""
    out, n = [], 0
    for op in stream:
        if op[0] == "reset":
            runner.reset()
            n = 0
            continue
        _, step, answers = op
        for _ in range(2):
            runner.scan(pose_at(n, lane + 0.003 * n * n), np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]) * (1 + n))
            n += 1
        cloud = runner.reg.add_cloud(np.zeros((1, 6), np.float32))
        xc = runner.pose(runner.cur_id, n - 1)
        for sid, frame, score, drift, accepted in answers:
            xx = runner.pose(sid, 2 * frame + 1)
            runner.plan[(runner.cur_id, runner.frames(), sid)] = (frame, score, guess_for(xx, xc, [drift * 0.6, drift * 0.8, 0.0]))
            if not accepted:
                runner.reject.add((cloud, runner.cloud(sid, frame)))
        rec = runner.key(cloud, step)
        out.append((rec, runner.state()))
    return out


FLOATS = ("score", "jud", "drift_p", "span", "jour", "ratio", "ratio_threshold", "drift_threshold")
EXACT = ("id", "frame", "tried", "accept", "ord_bl", "kind", "relc_count", "halt", "push", "step", "node_i", "node_j")


def assert_margins(rec):
    """On the restatement's record: every quantity at least 1e-6 relative from the threshold it was compared with."""
    for d in rec["sessions"]:
        pairs = [(d["score"], d["jud"])]
        if "ratio" in d:
            pairs.append((d["ratio"], d["ratio_threshold"]))
        if "drift_threshold" in d:
            pairs.append((d["drift_p"], d["drift_threshold"]))
        for q, t in pairs:
            assert not np.isnan(q) and abs(q - t) >= 1e-6 * max(abs(t), 1e-300), (q, t, d)
        if "relc_count" in d:
            assert isinstance(d["relc_count"], int) and isinstance(d["halt"], int)


def assert_same(got, want):
    for (g, gs), (w, ws) in zip(got, want):
        assert_margins(w)
        for k in ("session", "keyframe", "scan_index", "isGraph", "isOpt", "match_num", "g_update", "ids", "stepsizes"):
            assert g[k] == w[k], (k, g[k], w[k])
        assert len(g["sessions"]) == len(w["sessions"])
        for a, b in zip(g["sessions"], w["sessions"]):
            assert set(a) == set(b), (sorted(a), sorted(b))
            assert {k: a.get(k) for k in EXACT} == {k: b.get(k) for k in EXACT}
            for k in FLOATS:
                if k in b:
                    assert np.isclose(a[k], b[k], rtol=1e-9, atol=0.0) or a[k] == b[k], (k, a[k], b[k])
        assert (g["optimised"] is None) == (w["optimised"] is None)
        if w["optimised"] is not None:
            assert max(max(LR.pose_diff(x, y)) for x, y in zip(g["optimised"]["poses"], w["optimised"]["poses"])) < 1e-9
            assert np.allclose(g["optimised"]["dx"][0], w["optimised"]["dx"][0], atol=1e-9) and np.allclose(g["optimised"]["dx"][1], w["optimised"]["dx"][1], atol=1e-9)
        assert gs["relc"] == ws["relc"] and gs["g_update"] == ws["g_update"] and np.allclose(gs["jours"], ws["jours"], rtol=1e-12, atol=0.0)
    assert len(got) == len(want)


POLICY = dict(curr_halt=2, prev_halt=3, ratio_drift=0.05)

# one session.  relc_count starts at prev_halt = 3 and is 1 after the keyframe that optimised; keyframe k sees relc_count = k - 2 from keyframe 4 on
IN_SESSION = [
    ("key", 0.0, []),
    ("key", 4.0, []),
    ("key", 4.0, []),
    ("key", 4.0, [(0, 0, 0.90, 0.50, True)]),      # 3: ratio 0.5 / 12 < 0.05, relc 6 > 2, drift 0.5 > 0.10: push, optimise
    ("key", 4.0, [(0, 1, 0.90, 0.70, True)]),      # 4: ratio 0.7 / 12 = 0.058: rejected by ratio_drift
    ("key", 4.0, [(0, 1, 0.90, 0.50, True)]),      # 5: relc 2 = curr_halt: push, no optimisation
    ("key", 4.0, [(0, 2, 0.90, 0.09, True)]),      # 6: relc 3 = curr_halt + 1, drift 0.09 < 0.10: push, no optimisation
    ("key", 4.0, [(0, 2, 0.90, 0.11, True)]),      # 7: relc 4, drift 0.11 > 0.10: push, optimise
    ("key", 0.0, [(0, 7, 0.90, 0.30, True)]),      # 8: no journey since keyframe 7: span 0, ratio inf: not pushed
    ("key", 4.0, [(0, 3, 0.44, 0.01, True)]),      # 9: score below jud 0.45: not tried
    ("key", 4.0, [(0, 3, 0.46, 0.01, True)]),      # 10: score above jud: tried, pushed
    ("key", 4.0, [(0, 4, 0.90, 0.01, False)]),     # 11: the registration turns it away
]

# sessions 0 (5 keyframes) and 1 (4 keyframes, jud 0.6) imported, session 2 running
CROSS_SESSION = [
    ("key", 0.0, [(0, 1, 0.90, 3.00, True)]),                                  # 0: first contact with 0: isGraph, isOpt, g_update, jours[0] = 0 -- whatever the drift
    ("key", 4.0, [(0, 1, 0.90, 0.19, True)]),                                  # 1: 0.19 / 4 < 0.05: push; relc 1: no optimisation; jours[0] = 1e-6
    ("key", 4.0, [(0, 2, 0.90, 0.21, True), (1, 0, 0.55, 0.10, True)]),        # 2: 0.21 / 4 > 0.05: rejected; session 1's 0.55 is below its jud 0.6: not tried
    ("key", 4.0, [(0, 2, 0.90, 0.30, True)]),                                  # 3: 0.30 / 8: push; relc 3 = prev_halt: no optimisation
    ("key", 8.0, [(0, 3, 0.90, 0.24, True)]),                                  # 4: relc 4 > prev_halt, drift 0.24 < 0.25: push, no optimisation
    ("key", 8.0, [(0, 3, 0.90, 0.26, True)]),                                  # 5: drift 0.26 > 0.25: push, optimise
    ("key", 8.0, [(0, 4, 0.90, 0.20, True), (1, 2, 0.90, 5.00, True)]),        # 6: two sessions answer: 0 connected, 1 first contact
    ("key", 8.0, [(0, 4, 0.90, 0.10, True), (1, 3, 0.90, 0.10, True), (2, 1, 0.90, 0.30, True)]),      # 7: all three, the running session among them
]

AFTER_RESET = [
    ("key", 0.0, []),
    ("key", 4.0, []),
    ("key", 4.0, []),
    ("reset",),
    ("key", 0.0, []),
    ("key", 4.0, [(0, 1, 0.90, 2.00, True)]),      # into the session just closed: first contact
    ("key", 4.0, [(0, 2, 0.90, 0.10, True), (1, 0, 0.90, 0.05, True)]),
]


def imports_of(name):
    return [imported_session(5, 0.0), imported_session(4, 1.5, jud=0.6)] if name == "cross" else []


@pytest.mark.parametrize("name, stream", [("in_session", IN_SESSION), ("cross", CROSS_SESSION), ("after_reset", AFTER_RESET)])
def test_policy_equals_the_restatement(name, stream):
    lane = 3.0 if name == "cross" else 0.0
    got = drive(Product(imports_of(name), **POLICY), stream, lane)
    want = drive(Restated(imports_of(name), **POLICY), stream, lane)
    assert_same(got, want)
    w = [r for r, _ in want]
    first = lambda r: r["sessions"][0]
    if name == "in_session":      # every branch the stream was written for was taken
        assert [r["isOpt"] for r in w] == [False, False, False, True, False, False, False, True, False, False, False, False]
        assert [bool(r["sessions"]) and first(r).get("push", False) for r in w] == [False, False, False, True, False, True, True, True, False, False, True, False]
        assert (first(w[5])["relc_count"], first(w[6])["relc_count"]) == (POLICY["curr_halt"], POLICY["curr_halt"] + 1)
        assert first(w[8])["span"] == 0.0 and first(w[8])["ratio"] == np.inf
        assert not first(w[9])["tried"] and first(w[10])["tried"] and first(w[11])["accept"] is False
        assert all(r["ids"] == [0] and not r["isGraph"] for r in w)
    if name == "cross":
        assert first(w[0])["kind"] == "first_contact" and w[0]["isGraph"] and w[0]["isOpt"] and w[0]["g_update"] and want[0][1]["jours"][0] == 0.0 and w[0]["ids"] == [0, 2]
        assert [first(r)["push"] for r in w[1:6]] == [True, False, True, True, True] and [r["isOpt"] for r in w[1:6]] == [False, False, False, False, True]
        assert (first(w[3])["relc_count"], first(w[4])["relc_count"]) == (POLICY["prev_halt"], POLICY["prev_halt"] + 1)
        assert w[2]["sessions"][1]["tried"] is False and want[1][1]["jours"][0] == 1e-6
        assert [d["kind"] for d in w[6]["sessions"]] == ["connected", "first_contact"] and w[6]["ids"] == [0, 1, 2] and w[6]["match_num"] == 2
        assert [d["kind"] for d in w[7]["sessions"]] == ["connected", "connected", "current"] and first(w[7])["node_i"] == 9 and w[7]["sessions"][2]["step"] == 2
    if name == "after_reset":
        assert [r["session"] for r in w] == [0, 0, 0, 1, 1, 1] and w[3]["ids"] == [1] and w[3]["stepsizes"] == [0, 2]
        assert first(w[4])["kind"] == "first_contact" and w[4]["isGraph"] and w[4]["ids"] == [0, 1] and w[4]["stepsizes"] == [0, 6, 10]
        assert [d["kind"] for d in w[5]["sessions"]] == ["connected", "current"] and [d["push"] for d in w[5]["sessions"]] == [True, True]


def test_new_session_closes_the_database_for_every_distance():
    p = Product([], **POLICY)
    drive(p, AFTER_RESET[:3], 0.0)
    assert p.ms.sessions[0].skip is None
    p.reset()
    assert p.ms.sessions[0].skip == -(3 + 10) and p.ms.cur_id == 1 and p.ms.ids == [1] and p.ms.stepsizes == [0, 0] and p.ms.initial.shape == (0, 12)
    assert p.ms.current.relc_count == POLICY["prev_halt"] and p.ms.current.jud == 0.45 and p.ms.graph_factors() == ([], [])
    seen = []
    p.ms.current.search.search_multi = lambda dbs, skips, cloud, params=None, f=p.ms.current.search.search_multi: (seen.append(list(skips)), f(dbs, skips, cloud, params))[1]
    drive(p, AFTER_RESET[4:5], 0.0)
    assert seen == [[-13, p.ms.params.skip_near_num]]
    imp = Product([imported_session(5, 0.0)], **POLICY)
    assert imp.ms.sessions[0].skip == -(5 + 10) and imp.ms.cur_id == 1 and imp.ms.sessions[0].scan_index == [1, 3, 5, 7, 9]


def assert_same_graph(a, b):
    """Two flattened graphs hold the same factors: between factors by (i, j) with records within 1e-9, priors likewise."""
    (abe, apr), (bbe, bpr) = a, b
    key = lambda t: (t[0], t[1])
    assert [key(t) for t in sorted(abe, key=key)] == [key(t) for t in sorted(bbe, key=key)]
    for x, y in zip(sorted(abe, key=key), sorted(bbe, key=key)):
        assert np.allclose(x[2], y[2], rtol=0.0, atol=1e-9)
    assert [(n, float(v)) for n, _, v in apr] == [(n, float(v)) for n, _, v in bpr]
    for x, y in zip(apr, bpr):
        assert np.allclose(x[1], y[1], rtol=0.0, atol=1e-9)


def test_build_graph_over_sessions_0_and_2_with_session_1_unconnected():
    runs = [Product(imports_of("cross"), **POLICY), Restated(imports_of("cross"), **POLICY)]
    recs = [drive(r, CROSS_SESSION[:6], 3.0) for r in runs]
    assert_same(*recs)
    p, lit = runs
    assert p.ms.ids == lit.lit.ids == [0, 2] and p.ms.stepsizes == lit.lit.stepsizes == [0, 10, 22]
    # the running graph: built at keyframe 0 (10 + 2 scans), grown since; its chain edges of the running session's later scans were measured at push time
    run_be, run_pr = p.graph()
    lit_be, lit_pr = lit.graph()
    assert_same_graph((run_be, run_pr), (lit_be, lit_pr))
    assert [(n, v) for n, _, v in run_pr] == [(0, 1e-9)]
    cur = p.ms.sessions[2].poses
    stale = [np.abs(d[:12] - multisession.MultiSession._between(cur[i - 10], cur[j - 10], d[12:])[:12]).max() for i, j, d in run_be if j == i + 1 and i >= 12]
    assert len(stale) == 9 and max(stale) > 1e-6            # the optimisation at keyframe 5 moved those scans; the running graph still holds what was measured
    # build_graph: every chain re-derived from the current poses, under each scan's own v6
    ids, steps = p.build()
    assert (ids, steps) == (list(lit.build()[0]), [0, 10, 22]) and ids == [0, 2]
    be, pr = p.graph()
    assert_same_graph((be, pr), lit.graph())
    assert len(pr) == 1 and pr[0][0] == 0 and pr[0][2] == 1e-9 and np.array_equal(pr[0][1], p.ms.sessions[0].poses[0])
    chain = [(i, j, d) for i, j, d in be if j == i + 1]
    loops = [(i, j, d) for i, j, d in be if j != i + 1]
    assert [(i, j) for i, j, _ in chain] == [(k, k + 1) for k in range(9)] + [(k, k + 1) for k in range(10, 21)]
    for i, j, d in chain:
        s, o = (p.ms.sessions[0], 0) if j < 10 else (p.ms.sessions[2], 10)
        assert np.allclose(d, multisession.MultiSession._between(s.poses[i - o], s.poses[j - o], s.v6[i - o]), rtol=0.0, atol=1e-12) and np.array_equal(d[12:], s.v6[i - o])
    pushed = [(r["sessions"][0]["ord_bl"], r["scan_index"]) for r, _ in recs[1] if r["sessions"] and r["sessions"][0].get("push")]
    assert [(i, j - 10) for i, j, _ in loops] == pushed == [(3, 1), (3, 3), (5, 7), (7, 9), (7, 11)]
    assert all(np.array_equal(d[12:], np.full(6, 1e-4)) for _, _, d in loops)
    assert p.ms.edges.connect(1) == [1] and len(p.ms.edges.edges) == 1 and (p.ms.edges.edges[0]["m1"], p.ms.edges.edges[0]["m2"]) == (0, 2)
