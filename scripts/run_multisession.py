"""Loop closure across two sessions (voxel_slam_amd.multisession over vxba_loopsearch_search_multi), next to the same policy on the numpy checkers.

    python scripts/run_multisession.py [--out profiles/multisession] [--first 12] [--second 8] [--profile]

Two drives over one synthetic world (tests/_multisession_cases.two_sessions): the first is imported as an earlier session, the second -- the same
corridor a little to the side, with odometry drift -- is streamed keyframe by keyframe through MultiSession.  Per keyframe: the sessions that
answered, what the policy did with each (kind, drift, push), ids and stepsizes, and whether the graph was optimised; at the end the loop edges and the
position error of every scan of the second drive against the truth before and after
(scans pushed after the last optimisation keep their odometry pose).  Every line is printed for the device run and for the run on the stand-ins
(tests/_multisession_ref.py) side by side.
--profile: one search_multi over S = 1, 4, 16 sessions of the first drive's size against S calls of vxba_loopsearch_search on the same handles, one
after the other (the only route without search_multi); wall clock around calls that end in a host synchronisation, the two alternating, median of 9
after a warm-up call of each, with the launch and synchronisation counts.  Records, not bars: multisession.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (its HIP runtime must enter the process before libvxba.so, as in tests/conftest.py)
except Exception:
    pass

import numpy as np  # noqa: E402

from tests import _multisession_cases as MC  # noqa: E402
from tests import _multisession_ref as MR  # noqa: E402
from voxel_slam_amd import multisession, vxba  # noqa: E402

V6 = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])


def stream(ts, **hooks):
    prm = vxba.LoopSearchParams(skip_near_num=ts["params"].skip_near_num)
    log = []
    with multisession.MultiSession(params=prm, jud_default=0.3, prev_halt=3, **hooks) as ms:
        ms.import_session([((loc, occ), rows, k) for k, (loc, occ, rows) in enumerate(ts["first"])], ts["first_poses"], V6)
        for k, (loc, occ, rows) in enumerate(ts["second"]):
            ms.push_scan(ts["second_poses"][k], V6)
            r = ms.push_keyframe((loc, occ), ms.reg.add_cloud(rows), jour_step=8.0 if k else 0.0)
            log.append(dict(keyframe=k, answered=[dict(session=d["id"], frame=d["frame"], score=d["score"], kind=d.get("kind"), drift_p=d.get("drift_p"), push=d.get("push", False))
                                                  for d in r["sessions"]], ids=r["ids"], stepsizes=r["stepsizes"], graph_rebuilt=r["isGraph"], optimised=r["isOpt"]))
        e = ms.edges.to_arrays()
        err = lambda P: [float(x) for x in np.linalg.norm(P[:, 9:] - ts["second_truth"][:, 9:], axis=1)]      # per scan of the second drive
        return dict(per_keyframe=log, edges=dict(pairs=e["pairs"].tolist(), ids=e["ids"].tolist()), ids=ms.ids, stepsizes=ms.stepsizes,
                    position_error_before_m=err(ts["second_poses"]), position_error_after_m=err(ms.current.poses))


def median_ms(fns, reps=9):
    """Wall milliseconds of every function of ``fns`` (each ends in a host synchronisation), alternating, median of ``reps`` after one warm-up each."""
    for f in fns:
        f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            t[k].append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(x)) for x in t]


def profile(ts, sizes=(1, 4, 16)):
    prm = vxba.LoopSearchParams(skip_near_num=-1000)               # every frame of every session is eligible
    loc, occ, rows = ts["second"][3]
    out = []
    with vxba.LoopRegistration() as reg:
        clouds = [reg.add_cloud(r) for _, _, r in ts["first"]]
        cur_cloud = reg.add_cloud(rows)
        handles = []
        for _ in range(max(sizes)):
            ls = vxba.LoopSearch(reg)
            for (l, o, _), cid in zip(ts["first"], clouds):
                ls.describe(l, o, prm)
                ls.add(cid)
            ls.describe(loc, occ, prm)                              # the single search reads each handle's own current set
            handles.append(ls)
        for S in sizes:
            dbs = handles[:S]
            multi = lambda: handles[0].search_multi(dbs, [-1000] * S, cur_cloud, prm)
            serial = lambda: [h.search(cur_cloud, prm) for h in dbs]
            t_multi, t_serial = median_ms([multi, serial])
            s, m = serial(), multi()                                # the multi search last: read_matches below is its list
            assert all(a["frame"] == b["frame"] and a["score"] == b["score"] and a["pose"].tobytes() == b["pose"].tobytes() for a, b in zip(m, s))
            out.append(dict(sessions=S, frames_per_session=len(clouds), descriptors_per_session=handles[0].num_descriptors(-1), matches=int(handles[0].read_matches().shape[0]),
                            search_multi_ms=t_multi, search_multi_launches=m[0]["launches"], search_multi_host_syncs=m[0]["host_syncs"],
                            sequential_ms=t_serial, sequential_launches=sum(r["launches"] for r in s), sequential_host_syncs=sum(r["host_syncs"] for r in s),
                            found=[r["frame"] for r in m]))
        for ls in handles:
            ls.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for multisession.json")
    ap.add_argument("--first", type=int, default=12)
    ap.add_argument("--second", type=int, default=8)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    ts = MC.two_sessions(a.first, a.second)
    dev = stream(ts)
    ref = stream(ts, search_cls=MR.RefLoopSearch, reg_cls=MR.RefLoopRegistration, graph_cls=MR.PG.RefPoseGraph)
    for d, r in zip(dev["per_keyframe"], ref["per_keyframe"]):
        print("device ", json.dumps(d, default=float))
        print("checker", json.dumps(r, default=float))
    for name, x in (("device ", dev), ("checker", ref)):
        print(name, json.dumps({k: v for k, v in x.items() if k != "per_keyframe"}, default=float))
    res = dict(first=a.first, second=a.second, device=dev, checker=ref)
    if a.profile:
        res["search"] = profile(ts)
        for row in res["search"]:
            print("search ", json.dumps(row, default=float))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "multisession.json"), "w") as fh:
            json.dump(res, fh, indent=1, default=float)


if __name__ == "__main__":
    main()
