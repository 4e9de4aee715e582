"""The loop hand-back on the device (vxba_kfarchive_*, vxba_map_loop_update_device, vxba_map_scan_device, voxel_slam_amd/handback.py) against the
numpy checker tests/_handback_ref.py -- for EQUALITY: both sides do the same IEEE operations in the same order without contraction -- and the device
route into the local map against the existing host route (which tests/test_gpu_map_fix.py pins to the reference's golden) fed the checker's clouds.
tests/test_handback_cpu.py asserts what the inputs used here contain and that the criteria reject four degraded checkers."""
import ctypes as C

import numpy as np
import pytest

from tests import _handback_ref as H

pytestmark = pytest.mark.gpu

INIT = 5
RADIUS = 10.0


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


_hip = None


def dev_read(addr, shape, dtype=np.float64):
    """A copy of device memory (the producing call has waited for its stream)."""
    global _hip
    out = np.zeros(shape, dtype=dtype)
    if out.size == 0:
        return out
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert addr and _hip.hipMemcpy(out.ctypes.data, addr, out.nbytes, 2) == 0
    return out


def fill_gpu(ar, kfs):
    for kid, pose, jour, down in kfs:
        ar.add(kid, pose, jour, down)
    return ar


def same_map_loop(got, want):
    """dict of KeyframeArchive.map_loop against (cloud_ptr, points, variances (N, 3, 3)) of the checker; the device's 3 x 3 are column-major."""
    cptr, P, V = want
    assert got["cloud_ptr"].tolist() == cptr.tolist()
    N = int(cptr[-1])
    if N == 0:
        assert got["pnt_world"] == 0 and got["var"] == 0
        return
    assert dev_read(got["pnt_world"], (N, 3)).tobytes() == P.tobytes()
    assert np.transpose(dev_read(got["var"], (N, 9)).reshape(N, 3, 3), (0, 2, 1)).tobytes() == np.ascontiguousarray(V).tobytes()


# ---- the archive ----
def test_archive_host_and_device_routes_read_growth_and_clear(vx):
    import torch
    kfs = H.make_keyframes(9) + [(100 + j, H.pose_rec(np.eye(3), [j, 0, 0]), 9.0 + j, np.random.default_rng(j).normal(size=(3000 + 1500 * j, 6)).astype(np.float32)) for j in range(4)]
    with vx.KeyframeArchive() as a, vx.KeyframeArchive() as b:
        caps = set()
        for kid, pose, jour, down in kfs:
            a.add(kid, pose, jour, down)
            t = torch.tensor(down, device="cuda"); torch.cuda.synchronize()
            b.add_device(kid, pose, jour, down.shape[0], t.data_ptr() if down.shape[0] else 0)
            assert b.stats()["bytes_h2d"] == 0 and a.stats()["bytes_h2d"] == down.nbytes      # the device route stages nothing through the host
            caps.add(a.device_ptrs()["xyzv"])
        assert len(caps) >= 3                                            # no store, then blocks at different addresses: the store moved as it grew ...
        for x in (a, b):                                                 # ... and every earlier keyframe is still what went in
            assert len(x) == len(kfs) and x.ids().tolist() == [k[0] for k in kfs] and not x.exist().any()
            for k, (kid, pose, jour, down) in enumerate(kfs):
                i = x.info(k)
                assert (i["id"], i["jour"], i["n"], i["exist"]) == (kid, jour, down.shape[0], 0) and np.array_equal(i["pose"], pose)
                assert x.read(k).tobytes() == down.tobytes()
            dp = x.device_ptrs()
            assert dp["cloud_ptr"].tolist() == np.concatenate([[0], np.cumsum([k[3].shape[0] for k in kfs])]).tolist()
            assert dev_read(dp["xyzv"], (int(dp["cloud_ptr"][-1]), 6), np.float32).tobytes() == np.concatenate([k[3] for k in kfs]).tobytes()
        # after clear, a second session in the same handle equals a fresh handle
        a.arm_history(INIT)
        a.clear()
        assert len(a) == 0 and a.history_size() == 0 and a.load_near([0, 0, 0])["k"] == -1
        second = H.make_keyframes(6, seed=2)
        fill_gpu(a, second)
        with vx.KeyframeArchive() as fresh:
            fill_gpu(fresh, second)
            want = H.fill(H.Archive(), second).map_loop(INIT, True)
            same_map_loop(a.map_loop(INIT, True), want); same_map_loop(fresh.map_loop(INIT, True), want)
            assert [a.info(k)["id"] for k in range(6)] == [fresh.info(k)["id"] for k in range(6)]


# ---- map_loop ----
@pytest.mark.parametrize("cumulative", [True, False])
@pytest.mark.parametrize("K", [0, 1, 4, 5, 6, 9])
def test_map_loop_equals_the_checker(vx, K, cumulative):
    """Keyframes of 0, 1, 63, 64, 65, 255, 256, 257 points (an empty one inside the range), coordinates of both signs, poses tens of metres out."""
    kfs = H.make_keyframes(K, seed=H.MAP_LOOP_SEED[K])
    sizes = [k[3].shape[0] for k in kfs[-INIT:]]
    with vx.KeyframeArchive() as a:
        fill_gpu(a, kfs)
        same_map_loop(a.map_loop(INIT, cumulative), H.fill(H.Archive(), kfs).map_loop(INIT, cumulative))
        assert a.stats()["launches"] == (1 if sum(sizes) else 0)


def test_map_loop_with_buffered_scans_carries_their_full_variances_unrotated(vx):
    import torch
    rng = np.random.default_rng(5)
    kfs = H.make_keyframes(6, seed=3)
    pend = []
    for n in (257, 0, 64):
        A = rng.normal(size=(n, 3, 3)) * 0.01
        pend.append((H.pose_rec(H.rodrigues(rng.normal(size=3)), rng.normal(size=3) * 30), rng.normal(size=(n, 3)) * 5, A @ np.transpose(A, (0, 2, 1)) + rng.normal(size=(n, 3, 3)) * 1e-6))
    tens = [(torch.tensor(np.ascontiguousarray(b), device="cuda"), torch.tensor(np.ascontiguousarray(np.transpose(v, (0, 2, 1))).reshape(-1, 9), device="cuda")) for _, b, v in pend]
    torch.cuda.synchronize()
    with vx.KeyframeArchive() as a:
        fill_gpu(a, kfs)
        got = a.map_loop(INIT, True, [(p[0], p[1].shape[0], t[0].data_ptr() if p[1].shape[0] else 0, t[1].data_ptr() if p[1].shape[0] else 0) for p, t in zip(pend, tens)])
        same_map_loop(got, H.fill(H.Archive(), kfs).map_loop(INIT, True, pend))
        assert (a.stats()["launches"], a.stats()["host_waits"]) == (1, 1) and got["cloud_ptr"].shape[0] == INIT + 3 + 1
        # a NULL variance array is zeros
        got = a.map_loop(INIT, False, [(pend[0][0], 257, tens[0][0].data_ptr(), 0)])
        same_map_loop(got, H.fill(H.Archive(), kfs).map_loop(INIT, False, [(pend[0][0], pend[0][1], None)]))


# ---- load_near along a scripted path ----
def test_load_near_along_the_scripted_path(vx):
    kfs, steps = H.make_history()
    ref = H.fill(H.Archive(), kfs)
    with vx.KeyframeArchive() as a:
        fill_gpu(a, kfs)
        assert a.load_near(steps[0][0], RADIUS)["k"] == -1 and a.stats()["launches"] == 0          # not armed
        a.arm_history(INIT); ref.arm_history(INIT)
        assert a.history_size() == ref.history_kfsize == 8 and a.exist().tolist() == ref.exist().tolist()
        loaded = []
        for p, what in steps:
            k, pts = ref.load_near(p, RADIUS)
            r = a.load_near(p, RADIUS)
            loaded.append(r["k"])
            assert r["k"] == k, what
            assert a.history_size() == ref.history_kfsize and a.exist().tolist() == ref.exist().tolist(), what
            if k >= 0:
                assert r["n"] == pts.shape[0] and dev_read(r["pnt_world"], pts.shape).tobytes() == pts.tobytes(), what
                assert (a.stats()["launches"], a.stats()["host_waits"]) == ((1, 1) if r["n"] else (0, 0))
            else:
                assert r["n"] == 0 and r["pnt_world"] == 0 and a.stats()["launches"] == 0
        assert loaded == [2, 3, 1, -1, 7, 0]
        # set_poses after arming: the search still reads the snapshot, the transform reads the new x0
        moved = np.array([k[1] for k in kfs]); moved[:, 9:] += 1000.0
        a.set_poses(moved); ref.set_poses(moved)
        k, pts = ref.load_near([16.0, 0.5, 1.0], RADIUS)
        r = a.load_near([16.0, 0.5, 1.0], RADIUS)
        assert r["k"] == k == 4 and dev_read(r["pnt_world"], pts.shape).tobytes() == pts.tobytes() and pts[:, 0].min() > 900
        # re-arming after the move snapshots the new positions: nothing near the old ones any more
        a.arm_history(INIT); ref.arm_history(INIT)
        assert a.load_near([16.0, 0.5, 1.0], RADIUS)["k"] == ref.load_near([16.0, 0.5, 1.0], RADIUS)[0] == -1 and a.history_size() == 8
    with vx.KeyframeArchive() as few:                                   # K <= init_num: nothing is armed
        fill_gpu(few, kfs[:INIT]); few.arm_history(INIT)
        assert few.history_size() == 0 and few.load_near(steps[0][0], RADIUS)["k"] == -1 and not few.exist().any()


# ---- the map ----
def _map_case():
    from tests.test_gpu_map_fix import _golden_module
    G = _golden_module()
    inp = G.inputs()
    xyz, fp = inp["xyz"], inp["fp"]
    kfs = []
    for k in range(7):                                                  # seven keyframes: five for map_loop, two of history
        body = xyz[fp[k]:fp[k + 1]][::2].astype(np.float32)
        d = np.abs(np.random.default_rng(100 + k).normal(0, 1e-4, (body.shape[0], 3))).astype(np.float32)
        kfs.append((k, G.corrected(inp["poses_gt"][k], inp["dR"], inp["dp"]), float(k), np.concatenate([body, d], axis=1)))
    return G, inp, kfs


def test_loop_update_device_and_keyframe_loading_equal_the_host_routes(vx):
    from tests.test_gpu_map_fix import _used_map, same_tables
    G, inp, kfs = _map_case()
    (a, win), (b, _) = _used_map(vx, G, inp), _used_map(vx, G, inp)
    poses = np.stack([G.corrected(inp["poses_in"][k], inp["dR"], inp["dp"]) for k in win])
    ref = H.fill(H.Archive(), kfs)
    with vx.KeyframeArchive() as ar:
        fill_gpu(ar, kfs)
        for cumulative in (True, False):
            ml = ar.map_loop(INIT, cumulative)
            a.loop_update_device(ml["cloud_ptr"], ml["pnt_world"], ml["var"], poses)
            clouds, cvars = ref.clouds(*ref.map_loop(INIT, cumulative))
            b.loop_update(clouds, cvars, poses, None)
            la = a.leaves()
            assert la["node_id"].size > 500 and (la["pcr_fix"][:, 9] > 0).sum() > 300 and la["has_sw"].sum() > 100
            same_tables(la, b.leaves())
            assert a.counts() == b.counts() and a.fix_pool()["cursor"] == b.fix_pool()["cursor"]
        # keyframe_loading against cut_voxel_fix with the checker's points
        ar.arm_history(INIT); ref.arm_history(INIT)
        p_curr = kfs[1][1][9:12] + np.array([0.3, -0.2, 0.1])
        d2 = ref.distances(p_curr).astype(np.float64)
        assert (np.abs(d2 - RADIUS * RADIUS) >= 1e-3).all() and abs(d2[0] - d2[1]) > 1e-3
        for step in range(3):                                           # two history keyframes, then nothing left
            r = ar.load_near(p_curr, RADIUS)
            k, pts = ref.load_near(p_curr, RADIUS)
            assert r["k"] == k == (1, 0, -1)[step]
            if k >= 0:
                a.cut_voxel_fix_device(r["n"], r["pnt_world"], None, 3.0 + step)
                b.cut_voxel_fix(pts, None, 3.0 + step)
            same_tables(a.leaves(), b.leaves())
        assert a.counts() == b.counts()
    a.close(); b.close()


# ---- scan_device ----
def test_scan_device_hands_the_marginalised_scan_to_the_keyframe_builder(vx):
    from tests.test_oracle_octree import PRM
    from voxel_slam_amd import synth
    S, win, pts = 4, 3, 12000
    xyz, fp, poses_gt, _ = synth.make_scans(win_size=S, pts_per_scan=pts, seed=synth.MASTER_SEED + 977)
    m, f, ge = vx.LocalMap(win_size=win, **PRM), vx.LidarFactor(win), vx.LioEstimator(PRM["voxel_size"], PRM["max_layer"])
    with pytest.raises(vx.VxbaError, match="VXBA_ERR_STATE"):
        m.scan_device(0)                                                # an empty slot
    cov = np.eye(15) * 1e-4
    host, xs = [], []
    kb_dev, kb_host = vx.KeyframeBuilder(2, 1.0), vx.KeyframeBuilder(2, 1.0)
    pushed = 0
    for k in range(S):
        state = np.concatenate([poses_gt[k], np.zeros(9), [0, 0, -9.8]])
        ge.var_init(xyz[fp[k]:fp[k + 1]].astype(np.float32))
        _, var_w = ge.pvec_update(state, cov)
        host.append((ge.read_points()[0], var_w))
        xs.append(poses_gt[k].copy())
        f.clear()
        m.cut_voxel_lio(len(xs) - 1, ge)
        m.recut(len(xs), np.stack(xs), f)
        if len(xs) == win:
            out = vx.Lidar_BA_Optimizer().damping_iter(np.stack(xs), f, max_iter=3)
            m.margi(win, out["poses"], f)
            sd = m.scan_device(0)                                       # ScanPose(x_buf[0], pvec_buf[0]) before the slot is reused
            pnt, var_w = host[0]
            assert sd["n"] == pnt.shape[0] and dev_read(sd["pnt_body"], pnt.shape).tobytes() == pnt.tobytes()
            assert np.transpose(dev_read(sd["var_world"], (sd["n"], 9)).reshape(-1, 3, 3), (0, 2, 1)).tobytes() == np.ascontiguousarray(var_w).tobytes()
            v6 = 1e-4 * np.ones(6)
            e1 = kb_dev.push_scan_device(out["poses"][0], v6, sd["n"], sd["pnt_body"], sd["var_world"])
            e2 = kb_host.push_scan(out["poses"][0], v6, pnt, var_w)
            assert e1 == e2
            pushed += 1
            m.slide(1)
            xs = [p for p in out["poses"][1:]]; host = host[1:]
    assert pushed == 2 and e1 and kb_dev.num_scans() == kb_host.num_scans() == 2
    i1, i2 = kb_dev.info(), kb_host.info()
    assert (i1["id"], i1["jour"], i1["n_full"], i1["n_down"]) == (i2["id"], i2["jour"], i2["n_full"], i2["n_down"]) and np.array_equal(i1["pose"], i2["pose"]) and i1["n_down"] > 100
    (f1, d1), (f2, d2) = kb_dev.read(), kb_host.read()
    assert f1.tobytes() == f2.tobytes() and d1.tobytes() == d2.tobytes()
    assert kb_dev.scan_poses()[0].tobytes() == kb_host.scan_poses()[0].tobytes()
    m.clear()
    with pytest.raises(vx.VxbaError, match="VXBA_ERR_STATE"):
        m.scan_device(0)                                                # forgotten by the clear
    for h in (kb_dev, kb_host, m, ge):
        h.close()


# ---- LoopHandback end to end ----
@pytest.mark.parametrize("n_pending", [0, 2])
def test_loop_handback_end_to_end(vx, n_pending):
    import torch
    from tests import _keyframe_ref as K
    from tests.test_gpu_map_fix import same_tables
    from tests.test_oracle_octree import PRM
    from voxel_slam_amd import handback, hba, synth
    st = synth.make_scanpose_stream(27, 500, 3, stationary=False, empty_scan=-1)
    scans = list(st)
    rk = K.KeyframeRef(3, 1.0)
    ref = H.Archive()
    for s in scans:
        if rk.push_scan(*s):
            kf = rk.keyframe
            ref.add(kf["id"], kf["pose"], kf["jour"], kf["down"])
    assert len(ref.kf) >= 7
    hb = handback.LoopHandback(init_num=INIT, radius=RADIUS)
    kb, ses = vx.KeyframeBuilder(3, 1.0), vx.HbaSession()
    with vx.LoopRegistration() as reg:
        got = hba.keyframe_stream(kb, reg, ses, scans, archive=hb)
    ar = hb.archive
    assert len(ar) == len(ref.kf) == len(got) and ar.ids().tolist() == [k["id"] for k in ref.kf]
    for k, kf in enumerate(ref.kf):
        assert ar.read(k).tobytes() == kf["cloud"].tobytes() and np.array_equal(ar.info(k)["pose"], kf["x0"]) and ar.info(k)["jour"] == kf["jour"]
    # a synthetic optimisation: the later scan poses are rotated and shifted, growing along the stream
    before, _ = kb.scan_poses()
    after = before.copy()
    for i in range(len(after)):
        w = i / len(after)
        dR = H.rodrigues(np.array([0.002, -0.001, 0.02]) * w)
        after[i, :9] = (dR @ before[i, :9].reshape(3, 3).T).T.reshape(9)
        after[i, 9:] = dR @ before[i, 9:] + np.array([0.05, -0.03, 0.01]) * w
    dx = hb.on_optimised(after, before)
    want_dx = H.loop_delta(before[-1], after[-1])
    assert np.array(dx[0]).tobytes() == np.array(want_dx[0]).tobytes() and np.array(dx[1]).tobytes() == np.array(want_dx[1]).tobytes() and hb.loop_detect == 1
    ref.set_poses(after[[k["id"] for k in ref.kf]]); ref.arm_history(INIT)
    assert ar.history_size() == ref.history_kfsize == len(ref.kf) - INIT and ar.exist().tolist() == ref.exist().tolist()
    # two maps that hold the last two scans of the stream in their window
    a, b = vx.LocalMap(win_size=3, **PRM), vx.LocalMap(win_size=3, **PRM)
    states = []
    for i, s in enumerate(scans[-2:]):
        pose, _, pts, var = s
        for m in (a, b):
            m.cut_voxel(i, pts, var.reshape(-1, 3, 3), H.world_cloud_vec(pose, pts))
        states.append(np.concatenate([pose, [0.3 + i, -0.2, 0.1], 0.01 * np.ones(6), [0.1, -0.2, -9.8]]))
    states = np.array(states)
    f = vx.LidarFactor(3)
    for m in (a, b):
        f.clear(); m.recut(2, states[:, :12], f)
    x_curr = states[-1].copy(); x_curr[12:15] = [1.0, 2.0, -0.5]
    rng = np.random.default_rng(8)
    pend_host, pend_dev, keep = [], [], []
    for j in range(n_pending):
        n = (130, 65)[j]
        body = rng.uniform(-1.4, 1.4, size=(n, 3)); A = rng.normal(size=(n, 3, 3)) * 0.01
        var = A @ np.transpose(A, (0, 2, 1)) + 1e-6 * np.eye(3)
        pose = scans[-3 - j][0]
        tb = torch.tensor(body, device="cuda"); tv = torch.tensor(np.ascontiguousarray(np.transpose(var, (0, 2, 1))).reshape(-1, 9), device="cuda")
        keep += [tb, tv]
        pend_host.append((pose, body, var)); pend_dev.append((pose, n, tb.data_ptr(), tv.data_ptr()))
    torch.cuda.synchronize()
    out = hb.loop_update(a, states, x_curr, 1, pending=pend_dev)
    want = H.loop_update(want_dx, after, states, x_curr, 1, pending_poses=[p[0] for p in pend_host])
    assert out["g_update"] == want["g_update"] == 2 and hb.loop_detect == 0
    for key in ("states", "x_curr", "path"):
        assert np.asarray(out[key]).tobytes() == np.asarray(want[key]).tobytes(), key
    assert out["path"].shape[0] == len(after) + n_pending + 2
    clouds, cvars = ref.clouds(*ref.map_loop(INIT, True, [(q, p[1], p[2]) for q, p in zip(want["pending_poses"], pend_host)]))
    b.loop_update(clouds, cvars, want["states"][:, :12], None)
    la = a.leaves()
    assert la["node_id"].size > 20 and (la["pcr_fix"][:, 9] > 0).sum() > 10 and la["has_sw"].sum() > 5
    same_tables(la, b.leaves())
    for step in range(3):                                               # three keyframe_loading steps as the sensor goes on
        p_curr = out["x_curr"][9:12] + 0.05 * step
        d2 = ref.distances(p_curr).astype(np.float64)
        assert (np.abs(d2 - RADIUS * RADIUS) >= 1e-3).all()
        k = hb.keyframe_loading(p_curr, 4.0 + step, a)
        kr, pts = ref.load_near(p_curr, RADIUS)
        assert k == kr and (k >= 0) == (step < len(ref.kf) - INIT)
        if kr >= 0:
            b.cut_voxel_fix(pts, None, 4.0 + step)
        same_tables(a.leaves(), b.leaves())
        assert ar.history_size() == ref.history_kfsize
    assert a.counts() == b.counts()
    for h in (a, b, kb, ses, hb):
        h.close()


# ---- refusals leave everything as it was ----
def test_refusals_leave_everything_as_it_was(vx):
    from tests.test_gpu_map_fix import _used_map, same_tables
    G, inp, kfs = _map_case()
    bad = kfs[0][1].copy(); bad[4] = np.nan
    with vx.KeyframeArchive() as ar:
        fill_gpu(ar, kfs)
        want = H.fill(H.Archive(), kfs).map_loop(INIT, True)
        with pytest.raises(vx.VxbaError, match="VXBA_ERR_ARG"):
            ar.add(99, bad, 0.0, kfs[0][3])
        x0 = np.array([k[1] for k in kfs]); x0[3, 10] = np.inf
        with pytest.raises(vx.VxbaError, match="VXBA_ERR_ARG"):
            ar.set_poses(x0)
        with pytest.raises(vx.VxbaError, match="VXBA_ERR_ARG"):
            ar.load_near([0.0, np.nan, 0.0])
        assert len(ar) == len(kfs) and all(np.array_equal(ar.info(k)["pose"], kfs[k][1]) for k in range(len(kfs)))
        ml = ar.map_loop(INIT, True)
        same_map_loop(ml, want)
        m, win = _used_map(vx, G, inp)
        before, counts = m.leaves(), m.counts()
        poses = np.stack([G.corrected(inp["poses_in"][k], inp["dR"], inp["dp"]) for k in win])
        other = vx.LioEstimator(2.0 * inp["kw"]["voxel_size"], inp["kw"]["max_layer"])
        with pytest.raises(vx.VxbaError, match="VXBA_ERR_ARG"):
            m.loop_update_device(ml["cloud_ptr"], ml["pnt_world"], ml["var"], poses, est=other)
        same_tables(before, m.leaves())
        assert m.counts() == counts and m.scan_device(0)["n"] > 0
        with pytest.raises(vx.VxbaError, match="VXBA_ERR_ARG"):
            m.scan_device(G.WIN)
        other.close(); m.close()


# ---- launches and waits ----
def test_launches_and_waits_do_not_depend_on_keyframes_or_points(vx):
    seen = set()
    for K in (1, 9):
        for n in (64, 257):
            with vx.KeyframeArchive() as ar:
                fill_gpu(ar, H.make_keyframes(K, seed=1, sizes=(n,)))
                for cumulative in (True, False):
                    ar.map_loop(INIT, cumulative)
                    seen.add((ar.stats()["launches"], ar.stats()["host_waits"], ar.stats()["bytes_d2h"]))
    assert seen == {(1, 1, 0)}
