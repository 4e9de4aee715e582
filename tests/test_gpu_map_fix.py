"""Fixed points in the device-resident local map (vxba_map_cut_voxel_fix / vxba_map_clear / vxba_map_loop_update, csrc/vxba_map.hip): what
keyframe_loading (voxelslam.cpp:1189-1228) and loop_update (:1101-1186) do to `surf_map`.  The pin is tests/golden/map_fix/*.npz, generated from the
reference's own cut_voxel / allocate_fix / recut by tests/golden/map_fix/make_golden_map_fix.py; the other tests need no checker."""
import importlib.util
import os

import numpy as np
import pytest

from tests.test_oracle_octree import PRM, point_vars, to_world

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden_module():
    spec = importlib.util.spec_from_file_location("tests._make_golden_map_fix", os.path.join(HERE, "golden", "map_fix", "make_golden_map_fix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-300))


def same_tables(a, b, skip=()):
    for key, va in a.items():
        if key not in skip and isinstance(va, np.ndarray):
            assert np.array_equal(va, b[key]), key


# ------------------------------------------------------------------------------------------------------------------------------------------
# the pin
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_device_map_with_loaded_keyframes_reproduces_the_reference_golden(vx):
    """The scenario of make_golden_map_fix.py on the device map, stage by stage against the leaf tables of the reference: identical leaves, flags
    and counts everywhere; pcr_fix / pcr_add BIT-IDENTICAL after the keyframe clouds (no BA result in the map yet) and pcr_fix / pcrs_local after the
    loop update (identical inputs); rounding-level agreement where the two sides' own BA results have entered."""
    G = _golden_module()
    g = G.load_fixture()
    inp = G.inputs()
    assert np.array_equal(inp["poses_in"], g["poses_in"])
    m, f = vx.LocalMap(win_size=G.WIN, **inp["kw"]), vx.LidarFactor(G.WIN)
    opt = vx.Lidar_BA_Optimizer()
    seen = []
    stats = {}

    def on_stage(tag, lm):
        lv = m.leaves()
        t = lambda key: g[f"{tag}_{key}"]
        assert np.array_equal(lv["node_id"], t("node_id")), tag
        for key in ("layer", "isexist", "is_plane", "has_sw", "in_slide", "last_num", "n_point_fix"):
            assert np.array_equal(np.asarray(lv[key]).astype(np.int64), t(key).astype(np.int64)), (tag, key)
        assert np.array_equal(lv["n_points"], t("n_points")), tag
        assert np.array_equal(lv["pcr_add"][:, 9], t("pcr_add")[:, 9]) and np.array_equal(lv["pcr_fix"][:, 9], t("pcr_fix")[:, 9]), tag
        r_add, r_fix = rel(lv["pcr_add"], t("pcr_add")), rel(lv["pcr_fix"], t("pcr_fix"))
        print(f"{tag}: {lv['node_id'].size} leaves, rel(pcr_add) {r_add:.3e}, rel(pcr_fix) {r_fix:.3e}")
        if tag == "fix0":
            assert np.array_equal(lv["pcr_fix"], t("pcr_fix")) and np.array_equal(lv["pcr_add"], t("pcr_add"))
            assert not lv["has_sw"].any() and not lv["in_slide"].any() and m.counts()["slide"] == 0
        if tag == "loop":
            assert np.array_equal(lv["pcr_fix"], t("pcr_fix")) and np.array_equal(lv["pcrs_local"], t("pcrs_local"))
            ca = lv["cov_add"][lv["has_sw"]][:, G.TRIU[0], G.TRIU[1]]
            r_cov = rel(ca, t("cov_add_triu"))
            print(f"loop: rel(cov_add) {r_cov:.3e}")
            assert r_cov < 1e-9
            kids = lv["layer"] > 0
            stats["loop_planes"] = int(lv["is_plane"].sum())
            stats["loop_kids_cov"] = int((kids & (np.abs(lv["cov_add"]).sum(axis=(1, 2)) > 0)).sum())
        assert r_add < 1e-9 and r_fix < 1e-9, (tag, r_add, r_fix)
        if tag != "kf5":
            pl = lv["is_plane"]
            vb2 = np.sum((t("pcr_add")[pl, 6:9] / t("pcr_add")[pl, 9:10]) ** 2, axis=1, keepdims=True)
            d = np.abs(lv["eig_val"][pl] - t("eig_val")[pl]) / (vb2 + 1.0)
            print(f"{tag}: eigenvalues of {int(pl.sum())} planes, max |diff| / (|v|^2 + 1) = {d.max() if d.size else 0.0:.3e}")
            assert np.all(d <= 1e-12), tag
        if lm is not None:
            assert np.array_equal(lm["trace"][:, 6:], t("trace")[:, 6:]), tag
            from voxel_slam_amd import synth
            et, er = synth.pose_errors(lm["poses"], t("poses"))
            print(f"{tag}: poses {et:.2e} m {er:.2e} rad")
            assert et < 1e-7 and er < 1e-7, (tag, et, er)
        stats[tag] = lv["node_id"].size
        stats[tag + "_kids_fix"] = int(((lv["layer"] > 0) & (lv["pcr_fix"][:, 9] > 0)).sum())
        seen.append(tag)

    def on_factor(k):
        lv = m.leaves()
        fac = lv["opt_state"] >= 0
        assert np.array_equal(np.sort(lv["node_id"][fac]), g[f"w{k}_factor_ids"]) and f.size() == int(fac.sum())
        stats.setdefault("first_factor_with_fix", int((fac & (lv["pcr_fix"][:, 9] > 0)).sum()))

    G.scenario(m, f, lambda ff, xs: opt.damping_iter(xs, ff, max_iter=3), inp, on_stage, on_factor, fixed=dict(kf_poses=g["kf_poses"], loop_poses=g["loop_poses"]))
    assert seen == ["fix0", "w5", "kf5", "w6", "w7", "w8", "loop"]
    # the case is not an empty one
    assert stats["first_factor_with_fix"] > 50 and stats["w8_kids_fix"] > 100 and stats["kf5"] > stats["w5"] and stats["loop_planes"] > 100
    assert stats["loop_kids_fix"] > 100 and stats["loop_kids_cov"] > 100
    fp = m.fix_pool()
    assert 0 < fp["cursor"] <= fp["capacity"]


# ------------------------------------------------------------------------------------------------------------------------------------------
# loop_update against its parts, and its two modes against each other
# ------------------------------------------------------------------------------------------------------------------------------------------
def _used_map(vx, G, inp, upto=7):
    """A map with loaded keyframes that has been through windows of scans 3 .. upto - 1 (poses as given, no BA: what enters the map is the same from
    handle to handle).  Returns (map, scan indices left in the window)."""
    xyz, fp, var = inp["xyz"], inp["fp"], inp["var"]
    m, f = vx.LocalMap(win_size=G.WIN, **inp["kw"]), vx.LidarFactor(G.WIN)
    for k in range(3):
        s = slice(fp[k], fp[k + 1])
        m.cut_voxel_fix(to_world(inp["poses_gt"][k], xyz[s])[::2], None, float(k))
    win = []
    for k in range(3, upto):
        s = slice(fp[k], fp[k + 1])
        win.append(k)
        xs = np.stack([inp["poses_in"][j] for j in win])
        f.clear()
        m.cut_voxel(len(win) - 1, xyz[s], var[s], to_world(xs[-1], xyz[s]))
        m.recut(len(win), xs, f)
        if len(win) == G.WIN:
            f.evaluate_only_residual(xs)
            m.margi(len(win), xs, f)
            m.slide(1)
            win = win[1:]
    return m, win


def _loop_inputs(G, inp, win):
    xyz, fp, var = inp["xyz"], inp["fp"], inp["var"]
    kf = [G.corrected(inp["poses_gt"][k], inp["dR"], inp["dp"]) for k in range(5)]
    clouds = [np.ascontiguousarray(to_world(kf[k], xyz[fp[k]:fp[k + 1]])[::2]) for k in range(5)]
    cvars = [G.keyframe_vars(k, c.shape[0]) for k, c in enumerate(clouds)]
    poses = np.stack([G.corrected(inp["poses_in"][k], inp["dR"], inp["dp"]) for k in win])
    scans = [(xyz[fp[k]:fp[k + 1]], var[fp[k]:fp[k + 1]]) for k in win]
    return clouds, cvars, poses, scans


def test_loop_update_is_clear_plus_its_parts_and_clear_forgets_everything(vx):
    G = _golden_module()
    inp = G.inputs()
    (a, win), (b, _) = _used_map(vx, G, inp), _used_map(vx, G, inp)
    clouds, cvars, poses, scans = _loop_inputs(G, inp, win)
    assert a.counts()["mp0"] != 0 and a.counts()["roots"] > 100
    a.loop_update(clouds, cvars, poses, scans)
    # by hand on a second used handle
    b.clear()
    c0 = b.counts()
    assert (c0["roots"], c0["slide"], c0["leaves"], c0["mp0"]) == (0, 0, 0, 0) and b.fix_pool()["cursor"] == 0 and b.leaves()["node_id"].size == 0
    f = vx.LidarFactor(G.WIN)
    for c, v in zip(clouds, cvars):
        b.cut_voxel_fix(c, v, 0.0)
    for i, (pnt, v) in enumerate(scans):
        b.cut_voxel(i, pnt, v, to_world(poses[i], pnt))       # (the same association as the device's unfused product)
    b.recut(len(scans), poses, f)
    la, lb = a.leaves(), b.leaves()
    assert la["node_id"].size > 500 and la["is_plane"].sum() > 100 and (la["pcr_fix"][:, 9] > 0).sum() > 300
    # multi_recut also fills the factor (opt_state); every root of this map with a leaf that can split is in the slide map, so the trees agree
    same_tables(la, lb, skip=("opt_state",))
    assert a.counts() == b.counts()
    # a fresh handle
    c = vx.LocalMap(win_size=G.WIN, **inp["kw"])
    c.loop_update(clouds, cvars, poses, scans)
    same_tables(la, c.leaves())
    assert a.counts() == c.counts()


def test_loop_update_on_the_resident_scans_equals_the_host_array_mode(vx):
    G = _golden_module()
    inp = G.inputs()
    (a, win), (b, _) = _used_map(vx, G, inp), _used_map(vx, G, inp)
    assert a.counts()["mp0"] == 2 and len(win) == 2
    clouds, cvars, poses, scans = _loop_inputs(G, inp, win)
    a.loop_update(clouds, cvars, poses, None)         # the ring slots' own scans, slot i <- old slot mp[i]
    b.loop_update(clouds, cvars, poses, scans)
    la = a.leaves()
    assert la["has_sw"].sum() > 300 and la["n_points"][:, :2].sum() > 1000
    same_tables(la, b.leaves())
    assert a.counts() == b.counts() and a.counts()["mp0"] == 0
    # and the window goes on from there: the next scan against both
    k = win[-1] + 1
    s = slice(inp["fp"][k], inp["fp"][k + 1])
    xs = np.concatenate([poses, G.corrected(inp["poses_in"][k], inp["dR"], inp["dp"])[None]])
    for m in (a, b):
        f = vx.LidarFactor(G.WIN)
        m.cut_voxel(2, inp["xyz"][s], inp["var"][s], to_world(xs[2], inp["xyz"][s]))
        assert m.recut(3, xs, f) > 50
    same_tables(a.leaves(), b.leaves())


# ------------------------------------------------------------------------------------------------------------------------------------------
# release, pool growth, arguments
# ------------------------------------------------------------------------------------------------------------------------------------------
def _box(rng, n, lo):
    return rng.uniform(0.05, 2.95, (n, 3)) + np.asarray(lo, dtype=np.float64)


def test_release_ages_loaded_roots_by_the_journey_they_were_given(vx):
    rng = np.random.default_rng(5)
    m = vx.LocalMap(win_size=3, thread_num=1, **PRM)
    old, young, scan = _box(rng, 3000, (0, 0, 0)), _box(rng, 3000, (10, 0, 0)), _box(rng, 3000, (20, 0, 0))
    m.cut_voxel_fix(old, None, 0.0)
    m.cut_voxel_fix(young, None, 10.0)
    m.cut_voxel_fix(old[:500] + 1e-3, None, 650.0)          # an existing root is not re-stamped
    pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    m.cut_voxel(0, scan, point_vars(3000, 2), scan)
    c0, b0, p0 = m.counts(), m.device_bytes(), m.fix_pool()
    assert c0["roots"] == 81 and c0["slide"] == 27 and p0["cursor"] >= 6500
    assert b0["fix_pool"] == p0["capacity"] * 96
    r = m.release(700.0, 700)
    c1, b1 = m.counts(), m.device_bytes()
    assert r["roots"] == 27 and c1["roots"] == 54 and c1["slide"] == 27
    lv = m.leaves()
    x = (lv["node_id"] >> np.uint64(48)).astype(np.int64) - 32768
    assert set(np.unique(x).tolist()) == {10, 11, 12, 20, 21, 22}
    assert int(lv["pcr_fix"][:, 9].sum()) == 3000 and int(lv["n_point_fix"].sum()) == 3000
    assert b1["nodes"] < b0["nodes"] and b1["total"] < b0["total"] and m.fix_pool()["cursor"] < p0["cursor"]
    r = m.release(710.0, 700)                               # now the roots loaded at journey 10; the slide map's stay whatever their stamp
    assert r["roots"] == 27 and m.counts()["roots"] == 27 and m.counts()["slide"] == 27


def _sequential_cluster(pts):
    c = [0.0] * 10
    for x, y, z in pts.tolist():      # PointCluster::push (tools.hpp:326-331), one rounding per operation
        c[9] += 1.0
        c[0] += x * x; c[1] += x * y; c[2] += x * z; c[3] += y * y; c[4] += y * z; c[5] += z * z
        c[6] += x; c[7] += y; c[8] += z
    return np.array(c)


@pytest.mark.parametrize("compact_at", [None, 2000])
def test_a_leaf_fed_by_successive_calls_keeps_its_points_in_call_order(vx, monkeypatch, compact_at):
    """One leaf outgrows its region of the fix-point pool four times (and, with the threshold lowered, the pool is compacted between the calls); the split
    that follows hands every point to a child by fix_divide, in stored order: the children's pcr_fix must be numpy's sequential sums per octant."""
    if compact_at:
        monkeypatch.setenv("VXBA_MAP_FIX_COMPACT_AT", str(compact_at))
    kw = dict(PRM); kw["max_layer"] = 1; kw["max_points"] = 60
    m = vx.LocalMap(win_size=3, thread_num=1, **kw)
    rng = np.random.default_rng(9)
    lo = np.array([3.0, 2.0, 0.0])
    calls = [rng.uniform(0.02, 0.98, (n, 3)) + lo for n in (100, 200, 400, 800, 1500)]
    other = rng.uniform(0.02, 0.98, (700, 3)) + np.array([7.0, 2.0, 0.0])     # a second leaf, so that regions interleave in the pool
    vs = [point_vars(c.shape[0], 20 + i) for i, c in enumerate(calls)]
    for i, c in enumerate(calls):
        m.cut_voxel_fix(c, vs[i], 0.0)
        m.cut_voxel_fix(other[100 * i:100 * (i + 1)], None, 0.0)
    allp = np.concatenate(calls)
    lv = m.leaves()
    assert lv["node_id"].size == 2 and sorted(lv["n_point_fix"].tolist()) == [500, 3000]
    big = int(np.argmax(lv["n_point_fix"]))
    assert np.array_equal(lv["pcr_fix"][big], _sequential_cluster(allp)) and np.array_equal(lv["pcr_add"][big], lv["pcr_fix"][big])
    assert not np.any(lv["cov_add"])                                            # push_fix_NOVAR
    fp = m.fix_pool()
    assert fp["cursor"] >= 3500 and (fp["compactions"] >= 1 if compact_at else fp["compactions"] == 0), fp
    # a window scan into the same voxel makes it split
    scan = rng.uniform(0.02, 0.98, (300, 3)) + lo
    f = vx.LidarFactor(3)
    pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    m.cut_voxel(0, scan, point_vars(300, 3), scan)
    m.recut(1, pose[None], f)
    lv = m.leaves()
    kids = np.nonzero((lv["layer"] == 1) & ((lv["node_id"] >> np.uint64(48)) == np.uint64(32768 + 3)))[0]
    assert kids.size == 8
    octant = 4 * (allp[:, 0] > lo[0] + 0.5) + 2 * (allp[:, 1] > lo[1] + 0.5) + (allp[:, 2] > lo[2] + 0.5)
    for j in kids:
        o = int((lv["node_id"][j] >> np.uint64(7 + 6)) & np.uint64(7))
        assert np.array_equal(lv["pcr_fix"][j], _sequential_cluster(allp[octant == o])), o
        assert np.any(lv["cov_add"][j])                                         # push_fix: the stored variances reached the child


def test_arguments_and_the_device_form(vx):
    import torch
    rng = np.random.default_rng(3)
    pts = _box(rng, 4000, (1, 1, 0))
    a, b, c = (vx.LocalMap(win_size=3, **PRM) for _ in range(3))
    a.cut_voxel_fix(pts, None, 2.0)
    b.cut_voxel_fix(pts, np.zeros((4000, 3, 3)), 2.0)                          # var = NULL is an array of zeros
    same_tables(a.leaves(), b.leaves())
    before = a.leaves()
    a.cut_voxel_fix(np.zeros((0, 3)), None, 0.0)                                # n = 0: a no-op
    same_tables(before, a.leaves())
    with pytest.raises(vx.VxbaError):
        a.cut_voxel_fix(pts + 1e6, None, 0.0)                                   # outside the +-32768 voxel range, as vxba_map_cut_voxel answers
    var = point_vars(4000, 4)
    a.cut_voxel_fix(pts[::-1], var, 3.0)
    tp = torch.tensor(np.ascontiguousarray(pts), device="cuda")
    tq = torch.tensor(np.ascontiguousarray(pts[::-1]), device="cuda")
    tv = torch.tensor(np.ascontiguousarray(np.transpose(var, (0, 2, 1))).reshape(-1, 9), device="cuda")
    torch.cuda.synchronize()
    c.cut_voxel_fix_device(4000, tp.data_ptr(), None, 2.0)
    c.cut_voxel_fix_device(4000, tq.data_ptr(), tv.data_ptr(), 3.0)
    same_tables(a.leaves(), c.leaves())
    assert a.counts() == c.counts() and a.leaves()["n_point_fix"].sum() == 8000


# ------------------------------------------------------------------------------------------------------------------------------------------
# the odometry's plane map follows a loop update
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_odometry_matches_against_the_rebuilt_map_only(vx):
    """loop_update(..., est) clears the odometry's plane map with the tree.  A used pair (map + odometry, planes exported before the loop closed) and a
    fresh pair go through the same loop update and the same next scan cycle; lio_state_estimation of the scan after must then be the same on both --
    a plane left over from before the loop update would be matched by the used pair only."""
    G = _golden_module()
    inp = G.inputs()
    xyz, fp, var = inp["xyz"], inp["fp"], inp["var"]
    a, win = _used_map(vx, G, inp)
    ea, eb = (vx.LioEstimator(inp["kw"]["voxel_size"], inp["kw"]["max_layer"]) for _ in range(2))
    assert a.export_planes(ea) > 100 and ea.map_size()[0] > 0
    b = vx.LocalMap(win_size=G.WIN, **inp["kw"])
    clouds, cvars, poses, scans = _loop_inputs(G, inp, win)
    a.loop_update(clouds, cvars, poses, None, est=ea)
    b.loop_update(clouds, cvars, poses, scans, est=eb)
    assert ea.map_size() == (0, 0)
    k = win[-1] + 1
    s = slice(fp[k], fp[k + 1])
    xs = np.concatenate([poses, G.corrected(inp["poses_in"][k], inp["dR"], inp["dp"])[None]])
    for m, e in ((a, ea), (b, eb)):
        f = vx.LidarFactor(G.WIN)
        m.cut_voxel(2, xyz[s], var[s], to_world(xs[2], xyz[s]))
        assert m.recut(3, xs, f) > 50
        f.evaluate_only_residual(xs)
        m.margi(3, xs, f)
        m.slide(1)
        assert m.export_planes(e) > 100
    same_tables(a.leaves(), b.leaves())
    assert ea.map_size() == eb.map_size() and ea.map_size()[1] > 0
    k += 1
    s = slice(fp[k], fp[k + 1])
    prior = np.concatenate([G.corrected(inp["poses_in"][k], inp["dR"], inp["dp"]), np.zeros(9), [0, 0, -9.8]])
    cov = np.eye(15) * 1e-4
    out = []
    for e in (ea, eb):
        e.var_init(xyz[s].astype(np.float32))
        out.append(e.lio_state_estimation(prior, cov))
    assert out[0]["match_num"] == out[1]["match_num"] > 100 and out[0]["iterations"] == out[1]["iterations"]
    assert np.array_equal(out[0]["state"], out[1]["state"]) and np.array_equal(out[0]["cov"], out[1]["cov"])
