"""The loop-closure chain from corners to a rebuilt map, timed (vxba_loopsearch_*, hba.loop_closure -> vxba_map_loop_update), next to the numpy checker.

    python scripts/run_loop_search.py [--out profiles/loopsearch] [--keyframes 41] [--radius 25] [--profile]

A corridor revisit like scripts/run_loop_icp.py's, but nothing is handed in: every keyframe's corners go through describe -> search -> add, and the
last keyframe, which revisits keyframe 3 from another heading, has to find it.  The found frame and hypothesis go through the score gate, the ICP and
the pose graph (hba.loop_closure), and the optimised poses rebuild the local map from the keyframes' plane centres (LocalMap.loop_update).
Per keyframe: wall milliseconds of describe, search and add (host synchronisation included) and of the vectorised checker on the same input; the
rows at database sizes 5 and 25 and at the end of the session go into loop_search.json with the launch and synchronisation counts.
--profile: the same session once more in a child process under `rocprofv3 --kernel-trace --stats`, its per-kernel table copied next to the JSON.
Records, not bars."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (its HIP runtime must enter the process before libvxba.so, as in tests/conftest.py)
except Exception:
    pass

import numpy as np  # noqa: E402

from tests import _loopreg_ref as LR  # noqa: E402
from tests import _loopsearch_cases as K  # noqa: E402
from tests import _loopsearch_ref as S  # noqa: E402
from voxel_slam_amd import hba, vxba  # noqa: E402


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def run(a, with_checker=True):
    ses = K.session(5, True, n_keyframes=a.keyframes, radius=a.radius, n_landmarks=int(190 * (a.keyframes + 1) / 26 * 1.25), skip_near_num=a.skip)
    prm_ref = ses["params"]
    prm = vxba.LoopSearchParams(skip_near_num=a.skip)
    kfs = ses["keyframes"]
    cur = len(kfs) - 1
    rows_out = []
    db = S.Database()
    with vxba.LoopRegistration() as reg, vxba.LoopSearch(reg) as ls:
        ls.describe(*kfs[0][:2], prm); ls.search(reg.add_cloud(kfs[0][2]), prm)          # first-call costs (module load, allocations) stay out of the rows
        clouds = []
        for k, (loc, occ, rows) in enumerate(kfs):
            cid = reg.add_cloud(rows); clouds.append(cid)
            nd, t_desc = ms(lambda: ls.describe(loc, occ, prm))
            row = dict(keyframe=k, corners=int(loc.shape[0]), descriptors=int(nd), database=ls.num_descriptors(-1), describe_ms=t_desc)
            if k < cur:
                r, row["search_ms"] = ms(lambda: ls.search(cid, prm))
                row.update(matches=int(ls.read_matches().shape[0]), candidates=len(r["candidates"]), frame=r["frame"], launches=r["launches"], host_syncs=r["host_syncs"])
                _, row["add_ms"] = ms(lambda: ls.add(cid))
            if with_checker:
                d, row["checker_describe_ms"] = ms(lambda: S.describe(loc, occ, prm_ref))
                rr, row["checker_search_ms"] = ms(lambda: db.search(d, rows, prm_ref))
                _, row["checker_add_ms"] = ms(lambda: db.add(d, rows))
                row["checker_frame"] = rr["frame"]
            rows_out.append(row)
        # the last keyframe: corners -> loop edge -> pose graph -> rebuilt map
        poses = K.pose_records(ses["R"], ses["p"])
        poses[:, 10] += 0.01 * np.arange(len(kfs))                                         # odometry drift
        v6 = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
        loc, occ, _ = kfs[cur]
        ls.describe(loc, occ, prm)
        _, t_revisit = ms(lambda: ls.search(clouds[cur], prm))                              # the one search of the session with matches to order and candidates to verify
        out, t_chain = ms(lambda: hba.loop_closure((loc, occ), clouds[cur], cur, poses, v6, ls, reg, params=prm, add=True))
        f = out["search"]
        rows_out[-1].update(search_ms=t_revisit, matches=int(ls.read_matches().shape[0]), candidates=len(f["candidates"]), frame=f["frame"], launches=f["launches"],
                            host_syncs=f["host_syncs"])
        chain = dict(found_frame=f["frame"], score=f["score"], candidates=[{k: c[k] for k in ("frame", "pairs", "hypotheses", "best", "max_vote", "useful", "score")} for c in f["candidates"]],
                     edges=len(out["edges"]), chain_ms=t_chain)
        if f["frame"] >= 0:
            dt, dr = LR.pose_diff(f["pose"], K.true_relative(ses["R"], ses["p"], f["frame"], cur))
            chain.update(hypothesis_error_m=dt, hypothesis_error_rad=dr)
        if out["edges"]:
            e = out["edges"][0]
            dt, dr = LR.pose_diff(LR.pose_of(e["rot"], e["tra"]), K.true_relative(ses["R"], ses["p"], e["i"], e["j"]))
            chain.update(edge=(e["i"], e["j"]), edge_error_m=dt, edge_error_rad=dr)
            gt = K.pose_records(ses["R"], ses["p"])
            chain.update(end_point_error_before_m=float(np.linalg.norm(poses[cur, 9:] - gt[cur, 9:])), end_point_error_after_m=float(np.linalg.norm(out["poses"][cur, 9:] - gt[cur, 9:])))
            m = vxba.LocalMap(win_size=10)
            world = []
            for k, (_, _, rows) in enumerate(kfs):
                Rk = out["poses"][k, :9].reshape(3, 3).T
                world.append(rows[:, :3].astype(np.float64) @ Rk.T + out["poses"][k, 9:])
            _, t_map = ms(lambda: m.loop_update(world))
            chain.update(map_rebuild_ms=t_map, map=m.counts())
            m.close()
        st = ls.stats()
    pick = {n: next((r for r in rows_out if r["keyframe"] == n), None) for n in (5, 25)}
    return dict(keyframes=len(kfs), radius=a.radius, skip_near_num=a.skip, at_5_frames=pick[5], at_25_frames=pick[25], last_search_before_revisit=rows_out[-2], revisit=rows_out[-1], chain=chain,
                database=dict(frames=st["frames"], descriptors=st["descriptors"], record_bytes=st["record_bytes"], table_bytes=st["table_bytes"]), per_keyframe=rows_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for loop_search.json (and kernel_stats.csv with --profile)")
    ap.add_argument("--keyframes", type=int, default=41)
    ap.add_argument("--radius", type=float, default=25.0)
    ap.add_argument("--skip", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:                                             # under the profiler: the device work only
        run(a, with_checker=False)
        return
    res = run(a)
    if a.profile:
        with tempfile.TemporaryDirectory() as td:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--child", "--keyframes", str(a.keyframes),
                   "--radius", str(a.radius), "--skip", str(a.skip)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            found = sorted(glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True))
            res["profile"] = dict(returncode=p.returncode, stats_file=os.path.basename(found[0]) if found else None)
            if found and a.out:
                os.makedirs(a.out, exist_ok=True)
                shutil.copy(found[0], os.path.join(a.out, "kernel_stats.csv"))
            elif not found:
                res["profile"]["stderr_tail"] = p.stderr[-600:]
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "loop_search.json"), "w") as fh:
            json.dump(res, fh, indent=1, default=float)
    short = {k: v for k, v in res.items() if k != "per_keyframe"}
    print(json.dumps(short, default=float))


if __name__ == "__main__":
    main()
