"""The search over several sessions on the GPU (vxba_loopsearch_search_multi, vxba.LoopSearch.search_multi) and the policy on top of it
(voxel_slam_amd.multisession) on real handles.

``search_multi`` is compared three ways on the cases of tests/_multisession_cases.py: row s against ``vxba_loopsearch_search`` on session s's handle
holding the same current set under skip_near_num[s] - (num_frames(cur) - num_frames(session s)) -- integers equal, doubles BIT FOR BIT --; against
the numpy checker (tests/_multisession_ref.search_multi) by the rules of tests/test_gpu_loopsearch.py (integers and scores equal, poses inside
1e-7 m / 1e-7 rad; tests/test_multisession_cpu.py shows the cases honest); and its match list and offsets against the checker's.
"""
import functools

import numpy as np
import pytest

from tests import _loopreg_ref as LR
from tests import _multisession_cases as MC
from tests import _multisession_ref as MR
from tests.test_gpu_loopsearch import POSE_CONTRACT, check_search, dev_params
from voxel_slam_amd import multisession, vxba

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    """One registration handle, one search handle per session of the cases' world (each holding the query as its current set), the query's cloud."""
    w = MC.world()
    prm = dev_params(MC.params())
    reg = vxba.LoopRegistration()
    handles = {}
    for name, frames in w["sessions"].items():
        ls = vxba.LoopSearch(reg)
        for loc, occ, rows in frames:
            ls.describe(loc, occ, prm)
            ls.add(reg.add_cloud(rows))
        ls.describe(w["query"][0], w["query"][1], prm)
        handles[name] = ls
    cloud = reg.add_cloud(w["query"][2])
    yield dict(reg=reg, handles=handles, cloud=cloud, prm=prm, w=w)
    for ls in handles.values():
        ls.close()
    reg.close()


@functools.lru_cache(maxsize=None)
def checker(candidate_num):
    return MC.describe_all(MC.params(candidate_num=candidate_num))


def current_handle(rig, case):
    """(handle, owned): the session's own handle, or a fresh one holding the query and ``n`` frames."""
    names, _, cur, _ = MC.CASES[case]
    if isinstance(cur, tuple):
        return rig["handles"][names[cur[1]]], False
    ls = vxba.LoopSearch(rig["reg"])
    ls.describe(rig["w"]["query"][0], rig["w"]["query"][1], rig["prm"])
    for _ in range(int(cur)):
        ls.add(rig["cloud"])
    return ls, True


def same_result(a, b):
    assert a["frame"] == b["frame"] and a["score"] == b["score"] and a["pose"].tobytes() == b["pose"].tobytes()
    assert len(a["candidates"]) == len(b["candidates"])
    for x, y in zip(a["candidates"], b["candidates"]):
        assert {k: v for k, v in x.items() if k != "pose"} == {k: v for k, v in y.items() if k != "pose"}
        assert x["pose"].tobytes() == y["pose"].tobytes()


@pytest.mark.parametrize("case", list(MC.CASES))
def test_search_multi_equals_single_searches_and_the_checker(rig, case):
    names, skips, _, p = MC.CASES[case]
    prm = dev_params(p)
    cur, owned = current_handle(rig, case)
    try:
        dbs = [rig["handles"][n] for n in names]
        got = cur.search_multi(dbs, skips, rig["cloud"], prm)
        rows, offs = cur.read_matches(), cur.read_match_offsets()
        assert len(got) == len(names) and offs.shape == (len(names) + 1,) and offs[0] == 0 and offs[-1] == rows.shape[0]
        ref_dbs, d = checker(p.candidate_num)
        want = MR.search_multi([ref_dbs[n] for n in names], d, rig["w"]["query"][2], cur.num_frames(), skips, p)
        assert np.array_equal(offs, want["offsets"]) and np.array_equal(rows, want["matches"])
        voff = 0
        for s, n in enumerate(names):
            db = rig["handles"][n]
            one = db.search(rig["cloud"], dev_params(MC.params(candidate_num=p.candidate_num, skip_near_num=MR.single_skip(skips[s], cur.num_frames(), db.num_frames()))))
            same_result(got[s], one)
            part = rows[offs[s]:offs[s + 1]].copy()
            part[:, 1] -= voff
            assert np.array_equal(part, db.read_matches())
            check_search(got[s], part, want["sessions"][s])
            assert (got[s]["launches"], got[s]["host_syncs"]) == (got[0]["launches"], got[0]["host_syncs"])
            voff += db.num_frames()
        # what the cases are there for, stated on the checker's result
        ws = want["sessions"]
        if case == "two":
            assert [c["frame"] for c in ws[0]["candidates"]] == [3, 0, 2] and ws[1]["candidates"][0]["pairs"] == 101 and ws[1]["candidates"][0]["hypotheses"] == 33
            assert ws[0]["frame"] == 3 and ws[1]["frame"] == 0
        if case == "empty_among_full":
            assert ws[0]["frame"] == ws[2]["frame"] == -1 and not ws[0]["candidates"] and ws[1]["frame"] >= 0 and ws[3]["frame"] == 0
        if case == "four_next_to_votes":
            assert ws[0]["matches"].shape[0] == 4 and not ws[0]["candidates"] and ws[0]["frame"] == -1 and ws[1]["frame"] == 3
        if case == "skip_equal_and_one_more":
            assert ws[0]["matches"][:, 1].tolist() == [0, 1, 2] and ws[1]["matches"][:, 1].tolist() == [0, 1, 2, 3]
        if case == "negative_skip":
            assert ws[0]["matches"][:, 1].tolist() == [0, 1, 2, 3]
        if case == "shorter_current":
            assert sorted(set(ws[0]["matches"][:, 1].tolist())) == [0, 1] and ws[1]["matches"][:, 1].tolist() == [0, 1, 2]
        if case.startswith("candidate_num_"):
            assert len(ws[0]["candidates"]) == p.candidate_num and len(ws[1]["candidates"]) == 1
    finally:
        if owned:
            cur.close()


def test_empty_current_set_and_empty_databases(rig):
    loc, occ, rows = rig["w"]["two_corners"]
    with vxba.LoopSearch(rig["reg"]) as cur:
        assert cur.describe(loc, occ, rig["prm"]) == 0
        for r in cur.search_multi([rig["handles"]["votes"], rig["handles"]["verify"]], [-1, -1], rig["cloud"], rig["prm"]):
            assert r["frame"] == -1 and r["score"] == 0.0 and not r["candidates"]
        assert cur.read_matches().shape == (0, 3) and cur.read_match_offsets().tolist() == [0, 0, 0]
    e = rig["handles"]["empty"]
    for r in e.search_multi([e, e, e], [-1, 0, 3], rig["cloud"], rig["prm"]):
        assert r["frame"] == -1 and r["score"] == 0.0 and not r["candidates"]


def test_launches_and_host_syncs_do_not_depend_on_the_sessions(rig):
    h = rig["handles"]
    one = h["four"].search_multi([h["four"]], [-1], rig["cloud"], rig["prm"])[0]                       # 1 session, 1 frame, 4 pairs
    names, skips, _, p = MC.CASES["sixteen"]
    many = h["votes"].search_multi([h[n] for n in names], skips, rig["cloud"], dev_params(p))[0]     # 16 sessions, 35 frames, hundreds of pairs
    big = h["verify"].search_multi([h["verify"]], [-1], rig["cloud"], rig["prm"])[0]
    single = h["verify"].search(rig["cloud"], rig["prm"])
    assert (one["launches"], one["host_syncs"]) == (many["launches"], many["host_syncs"]) == (big["launches"], big["host_syncs"]) == (9, 2)
    assert (single["launches"], single["host_syncs"]) == (9, 2)


def test_argument_errors_leave_every_handle_as_it_was(rig):
    h, reg = rig["handles"], rig["reg"]
    cur, dbs, skips = h["votes"], [h["votes"], h["verify"]], [-1, -1]
    base = cur.search_multi(dbs, skips, rig["cloud"], rig["prm"])
    rows0 = cur.read_matches()
    stats = {n: ls.stats() for n, ls in h.items()}

    def same():
        for n, ls in h.items():
            st = ls.stats()
            assert all(st[k] == stats[n][k] for k in ("frames", "descriptors", "record_bytes", "table_bytes")) and ls.num_descriptors(-2) == h["votes"].num_descriptors(-2)
        assert np.array_equal(cur.read_matches(), rows0)
        again = cur.search_multi(dbs, skips, rig["cloud"], rig["prm"])
        for a, b in zip(again, base):
            same_result(a, b)

    with vxba.LoopRegistration() as other_reg, vxba.LoopSearch(other_reg) as stranger:
        bad = [([], []), ([h["votes"]] * 17, [-1] * 17), ([h["votes"], None], skips), ([h["votes"], stranger], skips)]
        for d, k in bad:
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
                cur.search_multi(d, k, rig["cloud"], rig["prm"])
            same()
    for cid in (-1, reg.num_clouds()):
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            cur.search_multi(dbs, skips, cid, rig["prm"])
        same()
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        cur.search_multi(dbs, skips, rig["cloud"], vxba.LoopSearchParams(descriptor_near_num=3, candidate_num=65))
    same()
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        cur.search_multi(dbs, [-1], rig["cloud"], rig["prm"])
    same()
    single = cur.search(rig["cloud"], rig["prm"])                        # a single search in between: the offsets are gone, the single list is back
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_STATE"):
        cur.read_match_offsets()
    ref_dbs, d = checker(20)
    assert single["frame"] == 3 and np.array_equal(cur.read_matches(), ref_dbs["votes"].search(d, rig["w"]["query"][2], MC.params())["matches"])


def test_stale_registration_is_a_state_error():
    w = MC.world()
    prm = dev_params(MC.params())
    with vxba.LoopRegistration() as reg, vxba.LoopSearch(reg) as a, vxba.LoopSearch(reg) as b:
        loc, occ, rows = w["sessions"]["four"][0]
        a.describe(loc, occ, prm); a.add(reg.add_cloud(rows))
        reg.clear()
        cid = reg.add_cloud(rows)
        b.describe(loc, occ, prm)
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_STATE"):
            b.search_multi([b, a], [-1, -1], cid, prm)
        a.clear()
        assert [r["frame"] for r in b.search_multi([b, a], [-1, -1], cid, prm)] == [-1, -1]


# ---- the policy on real handles against the same policy on the numpy stand-ins -------------------------------------------------------------
def run_policy(ts, **hooks):
    prm = vxba.LoopSearchParams(skip_near_num=ts["params"].skip_near_num)
    v6 = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
    recs = []
    with multisession.MultiSession(params=prm, jud_default=0.3, prev_halt=3, **hooks) as ms:
        ms.import_session([((loc, occ), rows, k) for k, (loc, occ, rows) in enumerate(ts["first"])], ts["first_poses"], v6)
        for k, (loc, occ, rows) in enumerate(ts["second"]):
            ms.push_scan(ts["second_poses"][k], v6)
            recs.append(ms.push_keyframe((loc, occ), ms.reg.add_cloud(rows), jour_step=8.0 if k else 0.0))
        edges = ms.edges.to_arrays()
        poses = [s.poses.copy() for s in ms.sessions]
    return recs, edges, poses


def test_policy_on_the_device_equals_the_policy_on_the_checkers():
    ts = MC.two_sessions()
    got, ge, gp = run_policy(ts)
    want, we, wp = run_policy(ts, search_cls=MR.RefLoopSearch, reg_cls=MR.RefLoopRegistration, graph_cls=MR.PG.RefPoseGraph)
    keys = ("id", "frame", "tried", "accept", "ord_bl", "kind", "push", "step", "node_i", "node_j", "relc_count")
    for g, w in zip(got, want):
        assert (g["isGraph"], g["isOpt"], g["match_num"], g["ids"], g["stepsizes"]) == (w["isGraph"], w["isOpt"], w["match_num"], w["ids"], w["stepsizes"])
        assert [{k: d.get(k) for k in keys} for d in g["sessions"]] == [{k: d.get(k) for k in keys} for d in w["sessions"]]
    assert want[0]["isGraph"] and sum(r["match_num"] for r in want) >= 4 and sum(r["isOpt"] for r in want) >= 2      # first contact, then a drift past 0.25 m
    assert np.array_equal(ge["pairs"], we["pairs"]) and np.array_equal(ge["ids"], we["ids"]) and np.array_equal(ge["ptr"], we["ptr"])
    worst = max(max(LR.pose_diff(a, b)) for x, y in zip(gp, wp) for a, b in zip(x, y))
    print(f"policy on the device: {sum(r['match_num'] for r in got)} edges, poses within {worst:.3e} of the run on the checkers")
    assert worst <= POSE_CONTRACT[0]
