"""A saved session end to end and timed (voxel_slam_amd/sessionio.py, vxba.SavedSession, MultiSession.import_saved / global_map), next to the numpy
checker.

    python scripts/run_session_reload.py [--profile] [--out profiles/session/session.json] [--reps 9]

1. A synthetic session (synth.make_corner_revisit_stream: one scene seen several times) is saved in the reference's formats, reloaded with
   MultiSession.import_saved -- scans to the device once, keyframes, descriptor clouds, corners and plane clouds made there -- and a second visit is
   streamed through the keyframe builder: its keyframe closes a loop into the RELOADED session, the graph is optimised and the global map is built
   from the optimised poses, over the reloaded session and the running one (its keyframe clouds in an HbaSession, attach_hba).  File I/O, reload (merge, filter, windows) and map are timed separately; the keyframes, the descriptor clouds and the map
   are compared with the checker's (tests/_session_ref.py), bit for bit.
2. --profile: a session of 200 scans x 20 000 points (20 keyframes of 10 scans) through load_scans / build_keyframes / window_cloud, the device time
   per stage of build_keyframes from events recorded on the handle's stream, wall clock around the calls; one global map over a 500-keyframe set of
   the size of ``bench.py --config cfg5`` (500 x 20 000 points); the launches and host waits of build_keyframes at K = 2, 20 and 200.  Warm-up first,
   then the median of --reps.  First measurements, not bars.
"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (its HIP runtime must enter the process before libvxba.so, as in tests/conftest.py)
except Exception:
    torch = None

import numpy as np  # noqa: E402

from tests import _session_ref as S  # noqa: E402
from voxel_slam_amd import multisession, sessionio, synth, vxba  # noqa: E402

WIN, VOXEL, ACSIZE, MGSIZE = 3, 1.0, 1, 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def reload_demo(workdir):
    stream = synth.make_corner_revisit_stream(5, WIN, seed=55)
    first, live = stream[:4 * WIN], stream[4 * WIN:]
    n = len(first)
    states = np.concatenate([np.stack([x[0] for x in first]), np.zeros((n, 12))], axis=1)
    d = os.path.join(workdir, "first")
    _, t_save = timed(lambda: sessionio.save_session(d, [x[2] for x in first], 0.1 * np.arange(n), states, np.stack([x[1] for x in first]), min_scans=1))
    src, t_read = timed(lambda: sessionio.read_session(d))
    scans, _, st, v6 = src
    poses = np.ascontiguousarray(st[:, :12])
    prm = vxba.LoopSearchParams(skip_near_num=-1)
    with multisession.MultiSession(params=prm, jud_default=0.3) as ms, vxba.CornerExtractor() as ce, vxba.KeyframeBuilder(WIN, VOXEL) as kb, vxba.SavedSession() as probe, \
            contextlib.closing(vxba.HbaSession()) as hb:
        sid, t_import = timed(lambda: ms.import_saved(src, win_size=WIN, voxel_size=VOXEL, acsize=ACSIZE, mgsize=MGSIZE, corners=ce))
        # the stages of the reload on a handle of their own (import_saved runs them interleaved with the corner extraction)
        _, t_load = timed(lambda: probe.load_scans(scans, poses))
        K, t_build = timed(lambda: probe.build_keyframes(WIN, VOXEL))
        nw = vxba.SavedSession.num_windows(K, ACSIZE, MGSIZE)
        _, t_win = timed(lambda: [probe.window_cloud(w, ACSIZE, MGSIZE) for w in range(nw)])
        (wins, clouds, ids, x0), t_chk = timed(lambda: S.descriptor_frames(scans, poses, WIN, VOXEL, ACSIZE, MGSIZE))
        got = probe.read_keyframes()
        same_kf = len(got) == len(clouds) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, clouds))
        probe.window_cloud(nw - 1, ACSIZE, MGSIZE)
        same_win = bool(np.array_equal(bits(probe.read_window()), bits(wins[-1][0])))
        rec = None
        ms.attach_hba(hb)                       # the running session's keyframe clouds, device to device: it takes part in the map through them
        live_clouds = []
        for pose, v, pts, var in live:
            ms.push_scan(pose, v)
            if kb.push_scan(pose, v, pts, var):
                info, ptrs = kb.info(), kb.device_ptrs()
                ce.extract_device(info["n_full"], ptrs["full"])
                c = ce.read()
                rec = ms.push_keyframe((c["locations"], c["occupancy"]), ms.reg.add_keyframe_device(info["n_full"], ptrs["full"]))
                hb.add_keyframes_device([info["n_full"]], ptrs["full"])
                live_clouds.append(kb.read()[0])
        s0, s1 = ms.sessions[sid], ms.current
        gm, t_map = timed(lambda: ms.global_map())
        ref, t_map_chk = timed(lambda: S.globalmap([(clouds, s0.x0, sid), (live_clouds, s1.x0, ms.cur_id)], 5000000))
        same_map = bool(np.array_equal(bits(gm["xyzi"]), bits(ref["xyzi"])))
        path = ms.global_path()
        found = rec["found"][sid] if rec else dict(frame=-1, score=0.0)
        out = dict(scans=n, points=int(sum(s.shape[0] for s in scans)), keyframes=int(K), windows=int(nw), keyframe_points=[int(c.shape[0]) for c in clouds],
                   found_frame=int(found["frame"]), score=float(found["score"]), edges_pushed=int(rec["match_num"]) if rec else 0, optimised=bool(rec and rec["isOpt"]),
                   map_points=int(gm["xyzi"].shape[0]), path_points=int(path.shape[0]), keyframes_match_checker=bool(same_kf), window_matches_checker=same_win,
                   map_matches_checker=same_map,
                   ms=dict(save_files=t_save, read_files=t_read, import_saved_first_call=t_import, load_scans=t_load, build_keyframes=t_build, windows=t_win, global_map=t_map,
                           checker_chain_cpu=t_chk, checker_map_cpu=t_map_chk))
    print("reload: " + json.dumps(out))
    if not (same_kf and same_win and same_map) or out["found_frame"] < 0 or out["edges_pushed"] != 1:
        raise SystemExit("the reloaded session did not close the loop, or the device and the checker disagree")
    return out


def big_session(n_scans, pts, seed=3):
    """Scans of a scene a few tens of metres wide seen from a slowly moving sensor: ~10 points per occupied 0.1 m voxel after the merge of 10."""
    rng = np.random.default_rng(seed)
    world = (rng.integers(-150, 150, size=(pts, 3)) * 0.1).astype(np.float32)
    scans, Rs, ps = [], [], []
    for k in range(n_scans):
        R = synth.rodrigues(np.deg2rad(np.array([0.0, 0.0, 0.2 * k]))); p = np.array([0.05 * k, 0.01 * k, 0.0])
        w = world + rng.uniform(0.0, 0.1, size=world.shape).astype(np.float32)
        scans.append(np.ascontiguousarray(((w.astype(np.float64) - p) @ R).astype(np.float32)))
        Rs.append(R); ps.append(p)
    return scans, synth.pack_poses(np.stack(Rs), np.stack(ps))


def profile(reps):
    med = lambda v: float(np.median(v))
    scans, poses = big_session(200, 20_000)
    xyz = np.ascontiguousarray(np.concatenate(scans)); ptr = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    out = {}
    with vxba.SavedSession() as s:
        s.set_profiling(True)
        loads, builds, stages, wins = [], [], [], []
        for r in range(reps + 2):
            _, tl = timed(lambda: s.load_scans(xyz, poses, scan_ptr=ptr))
            K, tb = timed(lambda: s.build_keyframes(10, 1.0))
            st = s.stage_times()
            nw = vxba.SavedSession.num_windows(K, 10, 5)
            _, tw = timed(lambda: [s.window_cloud(w, 10, 5) for w in range(nw)])
            if r >= 2:
                loads.append(tl); builds.append(tb); stages.append(st); wins.append(tw / max(nw, 1))
        k = s.keyframes()
        stats = s.stats()
        wc = s.window_cloud(0, 10, 5)
        out["reload"] = dict(scans=200, points=int(ptr[-1]), keyframes=int(K), keyframe_points=int(k["kf_ptr"][-1]), windows=int(nw), window_points=int(wc["n"]),
                             load_scans_wall_ms=med(loads), build_keyframes_wall_ms=med(builds), build_stage_ms={n: med([x[n] for x in stages]) for n in stages[0]},
                             window_cloud_wall_ms=med(wins), reps=reps)
    counts = {}
    for K in (2, 20, 200):
        sc, ps = big_session(10 * K, 500, seed=K)
        with vxba.SavedSession() as s:
            s.load_scans(sc, ps)
            assert s.build_keyframes(10, 1.0) == K
            st = s.stats()
            counts[str(K)] = dict(launches=st["launches"], host_waits=st["host_waits"])
    out["build_counts"] = counts
    # one global map over a session of the size of bench.py --config cfg5: 500 keyframes of 20 000 points
    rng = np.random.default_rng(5)
    Kf, n = 500, 20_000
    hb = vxba.HbaSession()
    try:
        for b in range(0, Kf, 50):
            hb.add_keyframes([(rng.uniform(-20, 20, size=(n, 3))).astype(np.float32) for _ in range(50)])
        d, cptr = hb.device_clouds()
        kp = synth.pack_poses(np.stack([synth.rodrigues(np.deg2rad(np.array([0.0, 0.0, 0.3 * k]))) for k in range(Kf)]), np.stack([np.array([0.5 * k, 0.0, 0.0]) for k in range(Kf)]))
        sets = [dict(d_xyz=d, cloud_ptr=cptr, poses=kp, id=0)]
        res = {}
        for name, interval in (("interval_5e6", 5_000_000), ("interval_1e5", 100_000)):
            t = []
            for r in range(reps + 2):
                g, ms_ = timed(lambda: vxba.global_map(sets, interval))
                if r >= 2:
                    t.append(ms_)
            res[name] = dict(points_out=int(g["xyzi"].shape[0]), chunks=int(g["chunk_ptr"].size - 1), wall_ms=med(t))
        out["global_map"] = dict(keyframes=Kf, points=Kf * n, **res, note="wall clock of the whole call, the copy of the map to the host included", reps=reps)
    finally:
        hb.close()
    print("profile: " + json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session", "session.json"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        res = dict(reload=reload_demo(td))
    if a.profile:
        res["profile"] = profile(a.reps)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
