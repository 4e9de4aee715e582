"""Deterministic inputs of the multi-session loop-search tests: several databases under ONE current set.

Built from the pieces of tests/_loopsearch_cases.py (corner triples with descriptor_near_num = 3: one triple, one descriptor).  The query keyframe is
the union of the queries of three of its scenarios -- ``votes`` (six triples), ``verify_101`` (101 triples) and ``skip`` (one triple) -- each in an
anchor range of its own, so that no triple comes near another; the sessions hold the scenarios' frames.  tests/test_multisession_cpu.py checks the
union for honesty as tests/test_loopsearch_cpu.py checks the scenarios: no integer and no verdict of the checker moves under a relative
perturbation of 1e-9, every verify distance and score gate keeps 1e-6.
"""
import functools

import numpy as np

from tests import _loopsearch_cases as K
from tests import _loopsearch_ref as S

WHERE_VOTES = list(range(0, 6))             # anchors at y = 0, 100
WHERE_VERIFY = list(range(200, 301))        # y = 1100 .. 1600
WHERE_SKIP = [400]                          # y = 1900
S0 = (6.2503, 8.0507, 10.2504)
O3 = np.array([K.FULL] * 3, np.uint64)


def params(**kw):
    return K.triple_params(**kw)


def _cat(parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@functools.lru_cache(maxsize=None)
def world():
    """dict(query (locations, occupancy, plane rows), sessions: name -> list of frames (locations, occupancy, plane rows), two_corners)."""
    cloud = K.small_cloud(3)
    cloud_m = K.move_cloud(cloud, *K.M1)
    sh = K.distinct_shapes(6, 60)
    qv, fv = K._moved(sh, 61, lambda k: K.M1, where=WHERE_VOTES)

    def part(ks):
        idx = np.concatenate([np.arange(3 * k, 3 * k + 3) for k in ks])
        return fv[0][idx], fv[1][idx], cloud_m
    q101, f101 = K._moved(K.distinct_shapes(101, 171), 181, lambda k: K.M1, where=WHERE_VERIFY)
    qs = K.triples_keyframe([S0], 45, where=WHERE_SKIP, occ=O3)
    loc, occ = _cat([qv, q101, qs])
    centres = loc.reshape(-1, 3, 3).mean(axis=1)
    d = np.linalg.norm(centres[:, None] - centres[None], axis=2) + 1e9 * np.eye(centres.shape[0])
    assert d.min() > 40.0, d.min()           # the triples of the union stay triples under descriptor_near_num = 3
    sessions = dict(
        votes=[part(range(0, 5)), part(range(0, 4)), part(range(1, 6)), part(range(0, 6))],       # votes 5, 4, 5, 6
        verify=[f101 + (cloud_m,)],                                                                 # 101 pairs: skip_len 3
        four=[part(range(0, 4))],                                                                   # no frame reaches 5 votes
        skip=[K.triples_keyframe([S0], 40 + k, where=WHERE_SKIP, occ=O3) + (cloud,) for k in range(4)],
        empty=[],
    )
    two = (np.array([[0.0, 0, 0], [8.0, 1.0, 0.5]]), np.array([0xFFF, 0xFFF0], np.uint64), cloud)
    return dict(query=(loc, occ, cloud), sessions=sessions, two_corners=two)


# name -> (sessions searched, skip_near_num per session, frames the current handle holds, or the index in the list of the session that IS the current
# handle, Params of the call).  Session "skip" holds frames 0..3: with 6 frames in the current handle and skip 3, frame 3 is at distance 3 (out) and
# frame 2 at 4 (in); with skip 2 frame 3 comes in as well.
ALL = -100                                  # a skip under which every frame is eligible whatever the current handle holds
CASES = {
    "one": (["votes"], [ALL], 0, params()),
    "two": (["votes", "verify"], [ALL, ALL], 2, params()),
    "three_cur_among": (["verify", "votes", "four"], [-1, -1, -1], ("index", 1), params()),
    "empty_among_full": (["empty", "votes", "empty", "verify"], [-1, ALL, 0, -4], 3, params()),
    "four_next_to_votes": (["four", "votes"], [ALL, ALL], 1, params()),
    "skip_equal_and_one_more": (["skip", "skip", "votes"], [3, 2, ALL], 6, params()),
    "negative_skip": (["skip", "votes", "verify"], [ALL, -7, -2], 9, params()),
    "shorter_current": (["votes", "skip"], [-1, -2], 1, params()),        # 1 - f > -1: frames 0, 1 of four; 1 - f > -2: frames 0, 1, 2
    "candidate_num_1": (["votes", "verify", "skip"], [ALL, ALL, ALL], 1, params(candidate_num=1)),
    "candidate_num_2": (["votes", "verify", "skip"], [ALL, ALL, ALL], 1, params(candidate_num=2)),
    "sixteen": (["votes", "verify", "four", "skip", "empty"] * 3 + ["votes"], [ALL, -1, -1, 1, -1, 2, -3, 0, 3, 4, ALL, -1, 5, -1, 2, 0], 4, params()),
}


def describe_all(prm, perturb=0.0):
    """The checker's databases of every session and its descriptors of the query."""
    w = world()
    dbs = {}
    for name, frames in w["sessions"].items():
        db = S.Database()
        for loc, occ, rows in frames:
            db.add(S.describe(loc, occ, prm, perturb), rows)
        dbs[name] = db
    return dbs, S.describe(w["query"][0], w["query"][1], prm, perturb)


def cur_frames(case, dbs):
    names, _, cur, _ = CASES[case]
    return dbs[names[cur[1]]].num_frames if isinstance(cur, tuple) else int(cur)


# ---- two drives over one world, for the policy on real handles and for scripts/run_multisession.py ----
def two_sessions(n_first=12, n_second=8):
    """Two drives over one world (tests/_loopsearch_cases.session, no revisit): the first imported, the second -- the same corridor a little to the
    side, with odometry drift -- streamed.  One scan per keyframe."""
    a = K.session(seed=5, revisit=False, n_keyframes=n_first)
    w = K.world(5, 190, 4.0 * (n_first + 1))
    R, p = K.keyframe_poses(False, n_second)
    p = p + np.array([1.0, 0.4, 0.05]); R = np.array([K.rot_z(0.03) @ r for r in R])
    rng = np.random.default_rng(77)
    b = [K.observe(w, R[k], p[k], rng) for k in range(n_second)]
    drift = np.zeros_like(p); drift[:, 1] = 0.06 * np.arange(n_second)
    return dict(first=a["keyframes"], first_poses=K.pose_records(a["R"], a["p"]), second=b, second_poses=K.pose_records(R, p + drift), second_truth=K.pose_records(R, p),
                params=a["params"])
