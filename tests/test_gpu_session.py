"""vxba_session_* and vxba_globalmap on the device against the numpy checker (tests/_session_ref.py), bit for bit, and against
vxba.down_sampling_voxel per keyframe; MultiSession.import_saved against import_session fed with the checker chain's frames.
tests/test_session_cpu.py asserts that the inputs of tests/_session_cases.py contain what they claim."""
import numpy as np
import pytest

from tests import _session_cases as SC
from tests import _session_ref as S

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_clouds(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w))


def loaded(case):
    from voxel_slam_amd import vxba
    s = vxba.SavedSession()
    s.load_scans(case["scans"], case["poses"])
    return s


@pytest.fixture(scope="module")
def main_ref():
    c = SC.main_case()
    clouds, ids, x0 = S.build_keyframes(c["scans"], c["poses"], c["win_size"], c["voxel_size"])
    merged, _, _ = S.merge_scans(c["scans"], c["poses"], c["win_size"])
    return dict(case=c, clouds=clouds, ids=ids, x0=x0, merged=merged)


@pytest.fixture(scope="module")
def window_ref():
    c = SC.window_case()
    clouds, ids, x0 = S.build_keyframes(c["scans"], c["poses"], c["win_size"], c["voxel_size"])
    return dict(case=c, clouds=clouds, ids=ids, x0=x0)


def test_build_keyframes_bit_for_bit(main_ref):
    from voxel_slam_amd import vxba
    c = main_ref["case"]
    with loaded(c) as s:
        assert s.num_scans() == 7 and s.build_keyframes(c["win_size"], c["voxel_size"]) == 2      # two keyframes, the seventh scan dropped
        k = s.keyframes()
        got = s.read_keyframes()
        assert k["ids"].tolist() == main_ref["ids"].tolist() == [2, 5] and np.array_equal(k["poses"], main_ref["x0"])
        assert k["kf_ptr"].tolist() == [0, got[0].shape[0], got[0].shape[0] + got[1].shape[0]]
        same_clouds(got, main_ref["clouds"])
        for g, m in zip(got, main_ref["merged"]):                                                   # ... and the stand-alone filter on that keyframe's merged cloud alone
            alone = vxba.down_sampling_voxel(m, c["voxel_size"] / 10)
            assert alone.shape == g.shape and np.array_equal(bits(alone), bits(g))
        st = s.stats()
        assert st["points"] == sum(x.shape[0] for x in c["scans"]) and st["keyframes"] == 2 and st["host_waits"] == 1
        # below 0.001 the filter returns the merged clouds untouched
        assert s.build_keyframes(c["win_size"], 0.005) == 2
        same_clouds(s.read_keyframes(), main_ref["merged"])


def test_fewer_scans_than_a_window_is_no_keyframe_and_no_error(main_ref):
    c = main_ref["case"]
    from voxel_slam_amd import vxba
    with vxba.SavedSession() as s:
        s.load_scans(c["scans"][:2], c["poses"][:2])
        assert s.build_keyframes(3, 1.0) == 0 and s.keyframes()["kf_ptr"].tolist() == [0] and s.read_keyframes() == [] and s.device_ptr() == 0
        s.load_scans([], np.zeros((0, 12)))
        assert s.build_keyframes(3, 1.0) == 0
        # a group of empty scans: one keyframe without a point
        s.load_scans([np.zeros((0, 3), np.float32)] * 3, c["poses"][:3])
        assert s.build_keyframes(3, 1.0) == 1 and s.keyframes()["kf_ptr"].tolist() == [0, 0] and s.keyframes()["ids"].tolist() == [2]


def test_refused_input_leaves_the_handle_as_it_was(main_ref):
    from voxel_slam_amd import vxba
    c = main_ref["case"]
    with loaded(c) as s:
        s.build_keyframes(c["win_size"], c["voxel_size"])

        def unchanged():
            assert s.num_scans() == 7 and s.num_keyframes() == 2
            same_clouds(s.read_keyframes(), main_ref["clouds"])
            assert np.array_equal(s.keyframes()["poses"], main_ref["x0"])

        xyz = np.concatenate(c["scans"]); ptr = np.concatenate([[0], np.cumsum([x.shape[0] for x in c["scans"]])])
        bad_ptr = ptr.copy(); bad_ptr[3] = bad_ptr[2] - 1
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*scan_ptr decreases at scan 2"):
            s.load_scans(xyz, c["poses"], scan_ptr=bad_ptr)
        unchanged()
        bad_pose = c["poses"].copy(); bad_pose[4, 10] = np.nan
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*pose of scan 4 is not finite"):
            s.load_scans(c["scans"], bad_pose)
        unchanged()
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*pose of scan 4 is not finite"):
            s.set_scan_poses(bad_pose)
        unchanged()
    # a point beyond the voxel range, or one that is not finite, is met by the build: error code, message, no keyframe made; the handle goes on working
    for bad_value in (2.0e5, np.nan):                          # 2e6 voxels of 0.1 m
        far = [x.copy() for x in c["scans"]]
        far[4][7, 1] = bad_value
        with vxba.SavedSession() as s2:
            s2.load_scans(far, c["poses"])
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*2\\^20 voxels"):
                s2.build_keyframes(c["win_size"], c["voxel_size"])
            assert s2.num_keyframes() == 0 and s2.num_scans() == 7 and s2.read_keyframes() == []
            s2.load_scans(c["scans"], c["poses"])
            assert s2.build_keyframes(c["win_size"], c["voxel_size"]) == 2
            same_clouds(s2.read_keyframes(), main_ref["clouds"])


def test_refused_build_keeps_the_previous_keyframes(main_ref):
    """load_scans replaces the scans and drops the keyframes, so the only build that can fail while keyframes exist is one whose points turn
    unacceptable under a different voxel size: 2^20 voxels of the new, smaller size no longer reach them."""
    from voxel_slam_amd import vxba
    c = main_ref["case"]
    scans = [x.copy() for x in c["scans"]]
    scans[0][5] = [2000.0, 0.0, 0.0]                           # fine at 0.1 m voxels (index 20000); out of range at 0.0011 m (1.8e6)
    with vxba.SavedSession() as s:
        s.load_scans(scans, c["poses"])
        assert s.build_keyframes(3, 1.0) == 2
        keep, k0 = s.read_keyframes(), s.keyframes()
        same_clouds(keep, S.build_keyframes(scans, c["poses"], 3, 1.0)[0])
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG.*2\\^20 voxels"):
            s.build_keyframes(3, 0.011)
        k1 = s.keyframes()
        same_clouds(s.read_keyframes(), keep)
        assert all(np.array_equal(k0[n], k1[n]) for n in k0) and s.num_keyframes() == 2
        w = s.window_cloud(0, 1, 1)                              # and they still serve
        assert w["n"] == keep[0].shape[0] and w["frame_id"] == 2


def test_launches_and_waits_do_not_depend_on_the_number_of_keyframes(main_ref):
    counts = {}
    for name, c in (("K2", main_ref["case"]), ("K12", SC.many_case())):
        with loaded(c) as s:
            K = s.build_keyframes(c["win_size"], c["voxel_size"])
            st = s.stats()
            counts[name] = (st["launches"], st["host_waits"])
            assert K == {"K2": 2, "K12": 12}[name]
            if name == "K12":
                same_clouds(s.read_keyframes(), S.build_keyframes(c["scans"], c["poses"], c["win_size"], c["voxel_size"])[0])
    assert counts["K2"] == counts["K12"] == (8, 1)


def test_windows_and_corners_from_the_device_cloud(window_ref):
    from voxel_slam_amd import vxba
    c = window_ref["case"]
    assert vxba.SavedSession.num_windows(5, 3, 1) == 2 and vxba.SavedSession.num_windows(3, 3, 1) == 0
    with loaded(c) as s, vxba.CornerExtractor() as ce:
        assert s.build_keyframes(c["win_size"], c["voxel_size"]) == 5
        same_clouds(s.read_keyframes(), window_ref["clouds"])
        with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
            s.window_cloud(2, 3, 1)
        for w, i in enumerate(S.windows(5, 3, 1)):
            want, fid = S.window_cloud(window_ref["clouds"], window_ref["x0"], window_ref["ids"], i, 3)
            wc = s.window_cloud(w, 3, 1)
            got = s.read_window()
            assert wc["n"] == want.shape[0] and wc["frame_id"] == fid == window_ref["ids"][i + 2] and np.array_equal(bits(got), bits(want))
            st = s.stats()
            assert (st["launches"], st["host_waits"]) == (1, 1)
            n_dev = ce.extract_device(wc["n"], wc["d_xyz"])
            dev = ce.read()
            n_host = ce.extract(got.astype(np.float64))
            host = ce.read()
            assert n_dev == n_host and np.array_equal(dev["occupancy"], host["occupancy"]) and np.array_equal(dev["locations"], host["locations"])


def test_corners_of_a_reloaded_scene_from_the_device_pointer():
    """The same on a cloud that HAS corners (the synthetic scene of the corner tests), so that the comparison above is not one of two empty sets."""
    from voxel_slam_amd import synth, vxba
    stream = synth.make_corner_revisit_stream(2, 3, seed=55)
    scans = [np.asarray(p, dtype=np.float32) for _, _, p, _ in stream]
    poses = np.stack([x[0] for x in stream])
    with vxba.SavedSession() as s, vxba.CornerExtractor() as ce:
        s.load_scans(scans, poses)
        assert s.build_keyframes(3, 1.0) == 2
        wc = s.window_cloud(0, 1, 1)
        got = s.read_window()
        want, fid = S.window_cloud(s.read_keyframes(), s.keyframes()["poses"], s.keyframes()["ids"], 0, 1)
        assert fid == wc["frame_id"] == 2 and np.array_equal(bits(got), bits(want))
        n_dev = ce.extract_device(wc["n"], wc["d_xyz"]); dev = ce.read()
        n_host = ce.extract(got.astype(np.float64)); host = ce.read()
        assert n_dev == n_host > 0 and np.array_equal(dev["occupancy"], host["occupancy"]) and np.array_equal(dev["locations"], host["locations"])


def test_set_scan_poses_moves_x0_windows_and_the_map(window_ref):
    from voxel_slam_amd import vxba
    c = window_ref["case"]
    new = SC.moved_poses(c["poses"])
    with loaded(c) as s:
        s.build_keyframes(c["win_size"], c["voxel_size"])
        s.window_cloud(0, 3, 1)
        before = s.read_window()
        s.set_scan_poses(new)
        k = s.keyframes()
        assert np.array_equal(k["poses"], new[k["ids"]]) and not np.array_equal(k["poses"], window_ref["x0"])
        same_clouds(s.read_keyframes(), window_ref["clouds"])                     # the clouds stay in their keyframes' frames
        want, _ = S.window_cloud(window_ref["clouds"], new[k["ids"]], k["ids"], 0, 3)
        s.window_cloud(0, 3, 1)
        got = s.read_window()
        assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(before))
        g = vxba.global_map([s.map_set(6)], 10 ** 6)
        ref = S.globalmap([(window_ref["clouds"], new[k["ids"]], 6)], 10 ** 6)
        assert np.array_equal(bits(g["xyzi"]), bits(ref["xyzi"])) and g["chunk_ptr"].tolist() == ref["chunk_ptr"].tolist()


def test_globalmap_over_saved_and_running_sets(main_ref, window_ref):
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(41)
    run_clouds = [SC.cloud(n, rng) for n in (33, 0, 58, 21)]                      # the running session: an HbaSession, one keyframe empty
    run_poses = SC.poses_for(4, 9)
    a, b = loaded(main_ref["case"]), loaded(window_ref["case"])
    hb = vxba.HbaSession()
    try:
        a.build_keyframes(3, 1.0); b.build_keyframes(3, 1.0)
        hb.add_keyframes(run_clouds)
        d, ptr = hb.device_clouds()
        assert ptr.tolist() == [0, 33, 33, 91, 112] and d
        sets = [b.map_set(1), a.map_set(0), dict(d_xyz=d, cloud_ptr=ptr, poses=run_poses, id=2)]
        ref_sets = [(window_ref["clouds"], window_ref["x0"], 1), (main_ref["clouds"], main_ref["x0"], 0), (run_clouds, run_poses, 2)]
        for interval in (40, 10 ** 6):
            ref = S.globalmap(ref_sets, interval)
            g = vxba.global_map(sets, interval)
            assert g["xyzi"].shape == ref["xyzi"].shape and np.array_equal(bits(g["xyzi"][:, :3]), bits(ref["xyzi"][:, :3]))
            assert np.array_equal(g["xyzi"][:, 3], ref["xyzi"][:, 3]) and set(g["xyzi"][:, 3].tolist()) == {0.0, 1.0, 2.0}
            assert g["chunk_ptr"].tolist() == ref["chunk_ptr"].tolist()
        ref = S.globalmap(ref_sets, 40)
        assert ref["jump"] == 3 and len(ref["chunk_ptr"]) > 3                     # every third point, several chunks
        n = ref["xyzi"].shape[0]
        out = np.full((n, 4), -1.0, dtype=np.float32)
        rc, need, _ = vxba._globalmap_call(sets, 40, out, n - 1)
        assert rc == 1 and need == n and np.all(out == -1.0)                      # VXBA_ERR_ARG, the exact count, nothing written
        rc, need, chunks = vxba._globalmap_call(sets, 40, out, n)
        assert rc == 0 and need == n and np.array_equal(bits(out), bits(ref["xyzi"])) and chunks.tolist() == ref["chunk_ptr"].tolist()
        assert vxba.global_map([], 40)["xyzi"].shape == (0, 4)
    finally:
        a.close(); b.close(); hb.close()


# ---- end to end: save, reload, close a loop into the reloaded session ----
def save_revisit(tmp_path, n_visits=4, n_live=1):
    from voxel_slam_amd import sessionio, synth
    stream = synth.make_corner_revisit_stream(n_visits + n_live, 3, seed=55)
    saved, live = stream[:3 * n_visits], stream[3 * n_visits:]
    n = len(saved)
    states = np.concatenate([np.stack([x[0] for x in saved]), np.zeros((n, 12))], axis=1)
    d = str(tmp_path / "first")
    assert sessionio.save_session(d, [x[2] for x in saved], 0.1 * np.arange(n), states, np.stack([x[1] for x in saved]), min_scans=1)
    return d, live


def live_keyframe(ms, ce, live):
    """The second visit's scans through the keyframe builder into the running session of ``ms``; returns push_keyframe's record."""
    from voxel_slam_amd import vxba
    with vxba.KeyframeBuilder(3, 1.0) as kb:
        for pose, v6, pts, var in live:
            ms.push_scan(pose, v6)
            if kb.push_scan(pose, v6, pts, var):
                info, ptrs = kb.info(), kb.device_ptrs()
                ce.extract_device(info["n_full"], ptrs["full"])
                c = ce.read()
                return ms.push_keyframe((c["locations"], c["occupancy"]), ms.reg.add_keyframe_device(info["n_full"], ptrs["full"]))
    raise AssertionError("no keyframe")


def test_import_saved_equals_import_session_on_the_checker_chain(tmp_path):
    from voxel_slam_amd import multisession, sessionio, vxba
    d, live = save_revisit(tmp_path)
    prm = vxba.LoopSearchParams(skip_near_num=-1)
    with multisession.MultiSession(params=prm, jud_default=0.3) as a, multisession.MultiSession(params=prm, jud_default=0.3) as b, vxba.CornerExtractor() as ce:
        sid = a.import_saved(d, win_size=3, voxel_size=1.0, acsize=1, mgsize=1, corners=ce)
        scans, t, states, v6 = sessionio.read_session(d)
        poses = np.ascontiguousarray(states[:, :12])
        wins, clouds, ids, x0 = S.descriptor_frames(scans, poses, 3, 1.0, 1, 1)
        frames = []
        for cloud, fid in wins:
            ce.extract(cloud.astype(np.float64))
            c = ce.read()
            frames.append(((c["locations"], c["occupancy"]), b.reg.add_keyframe(cloud.astype(np.float64)), fid))
        assert b.import_session(frames, poses, v6, keyframes=ids) == sid == 0
        sa, sb = a.sessions[0], b.sessions[0]
        assert sa.search.num_frames() == sb.search.num_frames() == 3 and sa.scan_index == sb.scan_index == [2, 5, 8] and sa.skip == sb.skip == -13
        assert [sa.search.num_descriptors(k) for k in range(3)] == [sb.search.num_descriptors(k) for k in range(3)] and sa.search.num_descriptors() > 0
        assert [k for k, _ in sa.keyframes] == [k for k, _ in sb.keyframes] == [2, 5, 8, 11] and np.array_equal(sa.x0, sb.x0) and np.array_equal(sa.x0, x0)
        assert [a.reg.cloud_size(i) for i in sa.cloud_ids] == [b.reg.cloud_size(i) for i in sb.cloud_ids]
        ra, rb = live_keyframe(a, ce, live), live_keyframe(b, ce, live)
        assert [(f["frame"], f["score"]) for f in ra["found"]] == [(f["frame"], f["score"]) for f in rb["found"]]
        assert all(np.array_equal(x["pose"], y["pose"]) for x, y in zip(ra["found"], rb["found"]))
        print(f"reloaded session: found {[(f['frame'], round(f['score'], 3)) for f in ra['found']]}, edges pushed {ra['match_num']}")
        assert ra["found"][0]["frame"] >= 0 and ra["match_num"] == rb["match_num"] == 1 and ra["isGraph"] and rb["isGraph"]
        ea, eb = a.edges.to_arrays(), b.edges.to_arrays()
        assert all(np.array_equal(ea[k], eb[k]) for k in ea) and ea["pairs"].tolist() == [[0, 1]]
        # the optimisation reached the reloaded session's device side, and the map is built from it
        ka = sa.saved.keyframes()
        assert np.array_equal(ka["poses"], sa.x0) and np.array_equal(sa.x0, sa.poses[[2, 5, 8, 11]])
        g = a.global_map()
        ref = S.globalmap([(clouds, sa.x0, 0)], 5000000)
        assert np.array_equal(bits(g["xyzi"]), bits(ref["xyzi"]))
        gp = a.global_path()
        assert gp.shape == (12 + 3, 4) and gp[:12, 3].tolist() == [0.0] * 12 and np.array_equal(gp[12:, :3], a.sessions[1].poses[:, 9:].astype(np.float32))


def test_running_session_joins_the_map_through_its_hba_session(tmp_path):
    """MultiSession.global_map over a reloaded session and the RUNNING one (attach_hba), in every state the running session goes through: no keyframe
    yet; keyframes before any optimisation; the keyframe that optimises; a keyframe after it that does not.  A keyframe has a pose from its creation
    on (upstream: Keyframe(xc)), so the map never waits for an optimisation."""
    from voxel_slam_amd import multisession, sessionio, vxba
    d, live = save_revisit(tmp_path, n_visits=3, n_live=4)
    scans, _, states, _ = sessionio.read_session(d)
    clouds, ids, _ = S.build_keyframes(scans, np.ascontiguousarray(states[:, :12]), 3, 1.0)
    prm = vxba.LoopSearchParams(skip_near_num=-1)
    hb = vxba.HbaSession()
    try:
        with multisession.MultiSession(params=prm, jud_default=0.3) as ms, vxba.CornerExtractor() as ce, vxba.KeyframeBuilder(3, 1.0) as kb:
            assert ms.import_saved(d, win_size=3, voxel_size=1.0, acsize=1, mgsize=1, corners=ce) == 0
            old, run = ms.sessions[0], ms.sessions[1]
            ms.attach_hba(hb)
            run_clouds = []

            def held():
                """global_map() -- ids=None: every session with clouds on the device -- against the checker over both sessions' CURRENT poses."""
                assert run.x0.shape[0] == len(run.keyframes) == len(run_clouds) and np.array_equal(run.x0, run.poses[[k for k, _ in run.keyframes]].reshape(-1, 12))
                g = ms.global_map()
                ref = S.globalmap([(clouds, old.poses[ids], 0), (run_clouds, run.x0, 1)], 5000000)
                assert g["xyzi"].shape == ref["xyzi"].shape and np.array_equal(bits(g["xyzi"]), bits(ref["xyzi"])) and g["chunk_ptr"].tolist() == ref["chunk_ptr"].tolist()
                return g

            assert set(held()["xyzi"][:, 3].tolist()) == {0.0}                  # attached, no keyframe yet: the reloaded session alone, as before
            recs = []
            for k, (pose, v6, pts, var) in enumerate(live):
                ms.push_scan(pose, v6)
                if not kb.push_scan(pose, v6, pts, var):
                    continue
                info, ptrs = kb.info(), kb.device_ptrs()
                ce.extract_device(info["n_full"], ptrs["full"])
                c = ce.read()
                recs.append(ms.push_keyframe((c["locations"], c["occupancy"]), ms.reg.add_keyframe_device(info["n_full"], ptrs["full"])))
                hb.add_keyframes_device([info["n_full"]], ptrs["full"])
                run_clouds.append(kb.read()[0])
                g = held()
                assert set(g["xyzi"][:, 3].tolist()) == {0.0, 1.0}
            opt = [bool(r["isOpt"]) for r in recs]
            print("running session: " + "; ".join(f"found {r['found'][0]['frame']} score {r['found'][0]['score']:.3f} pushed {r['match_num']} optimised {o}" for r, o in zip(recs, opt)))
            # the first contact optimises, once: keyframes came before it (the search had not answered yet) and after it (the session is then
            # connected over a zero journey: an IEEE division, never pushed), and the map held at every one of them
            assert len(recs) == 4 and not opt[0] and opt.count(True) == 1 and 0 < opt.index(True) < 3 and [r["optimised"] is not None for r in recs] == opt
            assert recs[0]["match_num"] == 0 and recs[opt.index(True)]["match_num"] == 1 and recs[opt.index(True)]["isGraph"]
            assert [k for k, _ in run.keyframes] == [2, 5, 8, 11]
            assert np.array_equal(old.saved.keyframes()["poses"], old.poses[ids])
            # a session whose HbaSession holds another number of keyframes is refused by name, not mapped wrongly
            hb.add_keyframes([run_clouds[0]])
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_STATE.*session 1 has 4 keyframes, its HbaSession 5"):
                ms.global_map()
    finally:
        hb.close()


def test_import_saved_with_a_descriptor_window_that_holds_no_point():
    """Three empty scans make an empty keyframe, and at acsize 1 an empty descriptor window: (0, no address) goes through the corner extraction and
    the plane-cloud builder and makes a frame without descriptors, as upstream's loop would; the other windows are what they are without it."""
    from voxel_slam_amd import multisession, synth, vxba
    stream = synth.make_corner_revisit_stream(4, 3, seed=55)
    poses = np.stack([x[0] for x in stream]); v6 = np.stack([x[1] for x in stream])
    full = [np.asarray(x[2], dtype=np.float32) for x in stream]
    holed = [np.zeros((0, 3), np.float32) if 3 <= k < 6 else s for k, s in enumerate(full)]
    states = np.concatenate([poses, np.zeros((12, 12))], axis=1)
    prm = vxba.LoopSearchParams(skip_near_num=-1)
    with multisession.MultiSession(params=prm) as a, multisession.MultiSession(params=prm) as b, vxba.CornerExtractor() as ce:
        a.import_saved((holed, None, states, v6), win_size=3, voxel_size=1.0, acsize=1, mgsize=1, corners=ce)
        b.import_saved((full, None, states, v6), win_size=3, voxel_size=1.0, acsize=1, mgsize=1, corners=ce)
        sa, sb = a.sessions[0], b.sessions[0]
        assert sa.saved.keyframes()["kf_ptr"][1] == sa.saved.keyframes()["kf_ptr"][2] and sa.saved.window_cloud(1, 1, 1) == dict(n=0, d_xyz=0, frame_id=5)
        assert sa.search.num_frames() == sb.search.num_frames() == 3 and sa.scan_index == sb.scan_index == [2, 5, 8]
        na, nb = [sa.search.num_descriptors(k) for k in range(3)], [sb.search.num_descriptors(k) for k in range(3)]
        assert na[1] == 0 and nb[1] > 0 and na[0] == nb[0] > 0 and na[2] == nb[2] > 0
        assert a.reg.cloud_size(sa.cloud_ids[1]) == 0 and [a.reg.cloud_size(sa.cloud_ids[k]) for k in (0, 2)] == [b.reg.cloud_size(sb.cloud_ids[k]) for k in (0, 2)]
        clouds, ids, x0 = S.build_keyframes(holed, poses, 3, 1.0)
        assert clouds[1].shape == (0, 3)
        assert np.array_equal(bits(a.global_map()["xyzi"]), bits(S.globalmap([(clouds, x0, 0)], 5000000)["xyzi"]))
