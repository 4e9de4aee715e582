"""The loop search on the GPU (vxba_loopsearch_*, vxba.LoopSearch, hba.loop_search / loop_closure) against the numpy checker
tests/_loopsearch_ref.py, on the inputs of tests/_loopsearch_cases.py.

Counts, orders, corner indices, cells, match lists, votes, hypothesis indices, useful counts and scores are compared for EQUALITY:
tests/test_loopsearch_cpu.py (test_honesty_*) shows on the CPU that on every input used here no integer and no verdict changes when its
real-valued argument moves by 1e-9 relative, and that every distance against 3.0 and every gate of the score keeps 1e-6.  Triangles and
centres: 1e-12 relative.  Poses: the project's standing contract (1e-7 m, 1e-7 rad).

Largest deviations measured on the MI355X (this file, printed by test_zz_report): poses 3.7e-14 m / 6.4e-16 rad from the
checker's (numpy.linalg.svd), triangles and centres bit-equal; hba.loop_closure's edge 7.3e-16 m / 1.2e-16 rad from the one loop_registration makes
of the checker's candidate, the optimised poses within 1.4e-14.
"""
import functools

import numpy as np
import pytest

from tests import _loopreg_ref as LR
from tests import _loopsearch_cases as K
from tests import _loopsearch_ref as S
from voxel_slam_amd import hba, vxba

pytestmark = pytest.mark.gpu

POSE_CONTRACT = (1e-7, 1e-7)        # [m], [rad]: tests/test_gpu_loopreg.py
WORST = dict(pose_m=0.0, pose_rad=0.0, triangle_rel=0.0, centre_abs=0.0)


def dev_params(p):
    return vxba.LoopSearchParams(**{f: getattr(p, f) for f in ("descriptor_near_num", "descriptor_min_len", "descriptor_max_len", "std_side_resolution", "skip_near_num",
                                                                "candidate_num", "rough_dis_threshold", "similarity_threshold", "icp_threshold", "normal_threshold", "dis_threshold")})


@functools.lru_cache(maxsize=None)
def scenario(name):
    if name == "revisit":
        sc = K.session_scenario(True)
    elif name == "no_revisit":
        sc = K.session_scenario(False)
    else:
        sc = K.scenarios()[name]
    return sc, K.run_checker(sc)


@pytest.fixture(scope="module")
def reg():
    with vxba.LoopRegistration() as r:
        yield r


def run_device(reg, sc, on_add=None):
    """The scenario through the library: dict(described, searches, matches, stats per search)."""
    prm = dev_params(sc["params"][0])
    out = dict(described=[], searches=[], matches=[])
    with vxba.LoopSearch(reg) as ls:
        for loc, occ, rows in sc["frames"]:
            ls.describe(loc, occ, prm)
            out["described"].append(ls.read_descriptors())
            cid = reg.add_cloud(rows)
            if on_add is not None:
                on_add(ls, cid)
            else:
                ls.add(cid)
        loc, occ, rows = sc["query"]
        ls.describe(loc, occ, prm)
        out["described"].append(ls.read_descriptors())
        cur = reg.add_cloud(rows)
        for p in sc["params"]:
            out["searches"].append(ls.search(cur, dev_params(p)))
            out["matches"].append(ls.read_matches())
    return out


def check_described(got, want):
    nd = want["triangle"].shape[0]
    assert got["triangle"].shape[0] == nd
    assert np.array_equal(got["corners"], want["corners"])
    assert np.array_equal((got["triangle"] + 0.5).astype(np.int64), want["cell"])
    if nd:
        rel = np.abs(got["triangle"] - want["triangle"]) / np.abs(want["triangle"])
        cab = np.abs(got["centre"] - want["centre"]) / max(1.0, np.abs(want["centre"]).max())
        WORST["triangle_rel"] = max(WORST["triangle_rel"], float(rel.max())); WORST["centre_abs"] = max(WORST["centre_abs"], float(cab.max()))
        assert rel.max() <= 1e-12 and cab.max() <= 1e-12


def check_search(got, matches, want):
    assert np.array_equal(matches, want["matches"])
    assert got["frame"] == want["frame"]
    assert len(got["candidates"]) == len(want["candidates"])
    for g, w in zip(got["candidates"], want["candidates"]):
        for k in ("frame", "votes", "pairs", "hypotheses", "best", "max_vote", "useful"):
            assert g[k] == w[k], (k, g, w)
        assert g["score"] == w["score"]                      # equal useful counts over the same cloud: the same quotient
        dt, dr = LR.pose_diff(g["pose"], w["pose"])
        print(f"candidate frame {g['frame']}: pairs {g['pairs']}, max vote {g['max_vote']}, pose differs from the checker's by {dt:.3e} m, {dr:.3e} rad")
        WORST["pose_m"] = max(WORST["pose_m"], dt); WORST["pose_rad"] = max(WORST["pose_rad"], dr)
        assert dt <= POSE_CONTRACT[0] and dr <= POSE_CONTRACT[1]
    if want["frame"] >= 0:
        assert got["score"] == want["score"]
        dt, dr = LR.pose_diff(got["pose"], want["pose"])
        assert dt <= POSE_CONTRACT[0] and dr <= POSE_CONTRACT[1]


# ---- describe ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n0", "n1", "n2", "n3", "n7", "n15", "n100", "square", "equilateral", "collinear", "close_pair"])
def test_describe(reg, name):
    loc, occ, prm = K.describe_cases()[name]
    want = S.describe(loc, occ, prm)
    with vxba.LoopSearch(reg) as ls:
        n = ls.describe(loc, occ, dev_params(prm))
        got = ls.read_descriptors()
        assert n == ls.num_descriptors(-2) == want["triangle"].shape[0]
        check_described(got, want)
    expect = dict(n0=0, n1=0, n2=0, n3=1, square=1, equilateral=1)
    if name in expect:
        assert n == expect[name]
    if name == "collinear":            # the triple (0, 1, 2) is the near-collinear one
        assert not any(sorted(c) == [0, 1, 2] for c in got["corners"].tolist()) and n > 0
    if name == "close_pair":           # no triangle holds both corners of the pair closer than min_len
        assert not any({0, 1} <= set(c) for c in got["corners"].tolist()) and n > 0


def test_default_params_are_the_references():
    assert vxba.LoopSearchParams.library_defaults() == vxba.LoopSearchParams()
    assert dev_params(S.Params()) == vxba.LoopSearchParams()


# ---- add / query / vote / verify -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_cell_three_frames", "cell_boundary", "skip", "similarity", "votes", "verify_49", "verify_50", "verify_51", "verify_101", "max_vote_3",
                                  "max_vote_4", "equal_votes"])
def test_scenario(reg, name):
    sc, ref = scenario(name)
    dev = run_device(reg, sc)
    for g, w in zip(dev["described"], ref["described"]):
        check_described(g, w)
    for g, m, w in zip(dev["searches"], dev["matches"], ref["searches"]):
        check_search(g, m, w)
    s = ref["searches"]
    # what each scenario is there for, stated on the checker's result (the device equals it)
    if name == "one_cell_three_frames":
        assert s[0]["matches"].tolist() == [[0, 0, 0], [0, 1, 0], [0, 2, 0]]
    if name == "cell_boundary":
        assert s[0]["matches"].tolist() == [[0, 0, 0], [1, 0, 1]]
    if name == "skip":
        assert s[0]["matches"][:, 1].tolist() == [0, 1] and s[1]["matches"][:, 1].tolist() == [0, 1, 2, 3]
    if name == "similarity":
        assert s[0]["matches"].tolist() == [[0, 0, 0]]
    if name == "votes":
        assert [c["frame"] for c in s[0]["candidates"]] == [3, 0] and [c["frame"] for c in s[1]["candidates"]] == [3, 0, 2]
        assert [c["votes"] for c in s[1]["candidates"]] == [6, 5, 5]
    if name.startswith("verify_"):
        M = int(name.split("_")[1])
        c = s[0]["candidates"][0]
        assert c["pairs"] == M and c["hypotheses"] == M // (M // 50 + 1) and c["max_vote"] == M
    if name == "max_vote_3":
        assert s[0]["candidates"][0]["max_vote"] == 3 and s[0]["candidates"][0]["score"] == -1.0 and s[0]["frame"] == -1
    if name == "max_vote_4":
        assert s[0]["candidates"][0]["max_vote"] == 4 and s[0]["frame"] == 0
    if name == "equal_votes":
        assert s[0]["candidates"][0]["max_vote"] == 4 and s[0]["candidates"][0]["best"] == 0 and list(s[0]["candidates"][0]["hyp_votes"]) == [4] * 8


# ---- search, end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def revisit_run(reg):
    """The revisit session through the library, keyframe by keyframe: describe -> search -> add.  Keeps the handle open for the tests that go on."""
    sc, ref = scenario("revisit")
    prm = dev_params(sc["params"][0])
    ls = vxba.LoopSearch(reg)
    log = []
    frames = list(sc["frames"]) + [sc["query"]]
    clouds = []
    for k, (loc, occ, rows) in enumerate(frames):
        nd = ls.describe(loc, occ, prm)
        cid = reg.add_cloud(rows); clouds.append(cid)
        r = ls.search(cid, prm)
        before = ls.stats()
        if k < len(frames) - 1:
            ls.add(cid)
        log.append(dict(nd=nd, result=r, bytes_added=ls.stats()["record_bytes"] - before["record_bytes"]))
    yield dict(ls=ls, log=log, clouds=clouds, sc=sc, ref=ref, prm=prm)
    ls.close()


def test_revisit_session_finds_the_revisited_keyframe(revisit_run):
    sc, ref, log = revisit_run["sc"], revisit_run["ref"], revisit_run["log"]
    for k, e in enumerate(log[:-1]):
        assert e["result"]["frame"] == -1, k                 # nothing to find before the revisit (the checker: tests/test_loopsearch_cpu.py)
        assert e["nd"] == ref["described"][k]["triangle"].shape[0]
    check_search(log[-1]["result"], revisit_run["ls"].read_matches(), ref["searches"][0])
    assert log[-1]["result"]["frame"] == 3
    dt, dr = LR.pose_diff(log[-1]["result"]["pose"], K.true_relative(sc["R"], sc["p"], 3, K.N_KEYFRAMES - 1))
    assert dt < 0.5 and dr < 0.1                               # inside the ICP's first gates


def test_session_without_a_revisit_finds_nothing(reg):
    sc, ref = scenario("no_revisit")
    dev = run_device(reg, sc)
    assert ref["searches"][0]["frame"] == -1
    check_search(dev["searches"][0], dev["matches"][0], ref["searches"][0])


def test_structure_launches_and_bytes(reg, revisit_run):
    log = revisit_run["log"]
    a, b = log[5]["result"], log[-1]["result"]               # against 5 frames and against 24
    assert (a["launches"], a["host_syncs"]) == (b["launches"], b["host_syncs"]) == (9, 2)
    assert len(b["candidates"]) > 1
    one = run_device(reg, scenario("verify_49")[0])["searches"][0]
    assert len(one["candidates"]) == 1 and (one["launches"], one["host_syncs"]) == (9, 2)
    per = [e["bytes_added"] / e["nd"] for e in log[:-1]]
    assert min(per) == max(per) > 0                            # device bytes added by add: proportional to the keyframe's descriptors


def test_loop_closure_pushes_the_edge_registration_makes_of_the_checkers_candidates(reg, revisit_run):
    sc, ref, ls = revisit_run["sc"], revisit_run["ref"], revisit_run["ls"]
    cur = K.N_KEYFRAMES - 1
    poses = K.pose_records(sc["R"], sc["p"])
    poses[:, 10] += 0.01 * np.arange(K.N_KEYFRAMES)           # odometry drift
    v6 = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
    want = ref["searches"][0]
    cands = [(want["frame"], revisit_run["clouds"][want["frame"]])]
    r_want = hba.loop_registration(revisit_run["clouds"][cur], cands, want["pose"].reshape(1, 12), cur, reg=reg, score_threshold=sc["params"][0].icp_threshold)
    g_want = hba.loop_graph(poses, r_want["edges"], v6)
    loc, occ, _ = sc["query"]
    got = hba.loop_closure((loc, occ), revisit_run["clouds"][cur], cur, poses, v6, ls, reg, params=revisit_run["prm"], add=False)
    assert got["candidates"] == cands
    assert len(got["edges"]) == len(r_want["edges"]) == 1
    e, w = got["edges"][0], r_want["edges"][0]
    assert (e["i"], e["j"]) == (w["i"], w["j"]) == (3, cur)
    dt, dr = LR.pose_diff(LR.pose_of(e["rot"], e["tra"]), LR.pose_of(w["rot"], w["tra"]))
    assert dt <= POSE_CONTRACT[0] and dr <= POSE_CONTRACT[1]
    worst = max(max(LR.pose_diff(a, b)) for a, b in zip(got["poses"], g_want["poses"]))
    print(f"loop_closure: edge differs by {dt:.3e} m, {dr:.3e} rad; optimised poses by at most {worst:.3e}")
    assert worst <= POSE_CONTRACT[0]
    assert max(LR.pose_diff(got["poses"][cur], poses[cur])) > 1e-3      # the graph moved the revisiting keyframe


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_handle_and_database_as_they_were(reg):
    sc, ref = scenario("verify_49")
    prm = dev_params(sc["params"][0])
    with vxba.LoopSearch(reg) as ls:
        loc, occ, rows = sc["frames"][0]
        ls.describe(loc, occ, prm); ls.add(reg.add_cloud(rows))
        loc, occ, rows = sc["query"]
        ls.describe(loc, occ, prm)
        cur = reg.add_cloud(rows)
        base = ls.search(cur, prm); st = ls.stats(); nd = ls.num_descriptors(-2)

        def same():
            assert ls.stats()["frames"] == st["frames"] and ls.stats()["descriptors"] == st["descriptors"] and ls.stats()["record_bytes"] == st["record_bytes"]
            assert ls.num_descriptors(-2) == nd
            again = ls.search(cur, prm)
            assert again["frame"] == base["frame"] and again["score"] == base["score"] and np.array_equal(again["pose"], base["pose"])

        bad = loc.copy(); bad[4, 1] = np.nan
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            ls.describe(bad, occ, prm)
        same()
        bad[4, 1] = np.inf
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            ls.describe(bad, occ, prm)
        same()
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            ls.describe(loc, np.ones((loc.shape[0], 65), dtype=bool), prm)          # more than 64 bits' worth of occupancy
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            ls.describe(loc, [1 << 64] * loc.shape[0], prm)
        same()
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            ls.describe(loc, occ, vxba.LoopSearchParams(descriptor_min_len=0.3, std_side_resolution=0.2))      # cells below 2
        same()
        for cid in (-1, reg.num_clouds()):
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
                ls.search(cid, prm)
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
                ls.add(cid)
            same()


def test_zz_report():
    print("largest deviations of this run:", {k: float(f"{v:.3e}") for k, v in WORST.items()})
