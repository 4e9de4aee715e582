"""One grow-only device workspace per handle (csrc/vxba_dev.hpp: vxu::Arena), carved anew by every call: what fresh allocations cannot get wrong and a
shared workspace can -- stale contents of a larger earlier call, a regrow in the middle of a handle's life, a refused call that leaves its work behind.
Every entry point that carves one runs the point counts COUNTS in that order on ONE handle: 3000 -> 20000 crosses the growth, 20000 -> 65 and 3000 -> 1
reuse the block at a smaller size; after the largest call one call is refused and the next must be right again.  Each result is held to the checker its
neighbouring test uses, in the same way.  The second half does the same for the per-scan path: the local map (two arenas, several carvings per call), the
odometry's staging and the leased workspace of the stand-alone entry points (vxu::Lease)."""
import numpy as np
import pytest

from tests import _init_ref as IR
from tests import _keyframe_ref as KR
from tests import _loopreg_ref as LR
from tests import _oracle as O
from tests.test_gpu_keyframe import same_keyframe
from tests.test_gpu_loopreg import NORMAL_BOUND

pytestmark = pytest.mark.gpu

COUNTS = (3000, 1, 65, 20000, 65)
REFUSE_AFTER = 3          # ... the 20000-point call: the refused call and the 65-point one after it find the most left behind


def _cloud32(rng, n):
    """Gaussian points of a few voxels' spread, a tenth of them on voxel faces (tests/test_gpu_lio.py::test_down_sampling_voxel_is_bit_identical)."""
    xyz = (rng.normal(size=(n, 3)) * 2).astype(np.float32)
    xyz[: n // 10] = np.round(xyz[: n // 10] / 0.5) * 0.5
    if n > 10:
        xyz[5] = xyz[9]
    return xyz


def test_down_sampling_on_the_per_device_scratch():
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(8300)
    for k, n in enumerate(COUNTS):
        xyz = _cloud32(rng, n)
        assert np.array_equal(vxba.down_sampling_voxel(xyz, 0.5), O.down_sampling_voxel(xyz, 0.5)), (k, n)
        pts, sel = vxba.down_sampling_close(xyz, 0.5)
        want_p, want_s = IR.down_sampling_close(xyz, 0.5)
        assert np.array_equal(sel, want_s) and np.array_equal(pts, want_p), (k, n)
        if k == REFUSE_AFTER:
            bad = _cloud32(rng, 3000); bad[7] = (3e6, 0, 0)
            with pytest.raises(vxba.VxbaError):
                vxba.down_sampling_voxel(bad, 0.5)
            with pytest.raises(vxba.VxbaError):
                vxba.down_sampling_close(bad, 0.5)


def _planes(rng, n):
    """n points on a slightly rough plane, about fifty to a 1 m voxel (65 and fewer: inside one voxel), in random order."""
    half = max(1, int(round(np.sqrt(n / 50.0) / 2)))
    xy = rng.uniform(-half, half, size=(n, 2)) if n > 100 else rng.uniform(0.05, 0.95, size=(n, 2))
    z = 0.3 + 0.05 * xy[:, 0] - 0.03 * xy[:, 1] + rng.normal(0, 0.005, n)
    return np.ascontiguousarray(np.concatenate([xy, z[:, None]], axis=1))


def test_loopreg_add_keyframe_on_one_handle():
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(8301)
    with vxba.LoopRegistration() as r:
        for k, n in enumerate(COUNTS):
            c = _planes(rng, n)
            got = r.read_cloud(r.add_keyframe(c))
            want = LR.plane_cloud(c)
            rows, lam = want["rows"], want["lam"]
            assert got.shape == rows.shape and (got.shape[0] > 0) == (n >= 65), (k, n, got.shape, rows.shape)
            assert np.array_equal(LR.voxel_coords(got[:, :3].astype(np.float64), 1.0), want["coords"]), (k, n)
            assert np.all(np.abs(got[:, :3] - rows[:, :3]) <= np.spacing(np.abs(rows[:, :3]))), (k, n)
            well = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
            assert np.all(np.abs(got[well, 3:].astype(np.float64) - rows[well, 3:].astype(np.float64)) <= NORMAL_BOUND), (k, n)
            if k == REFUSE_AFTER:
                bad = _planes(rng, 3000); bad[7, 0] = 2.0 ** 20 + 0.5
                before = r.num_clouds()
                with pytest.raises(vxba.VxbaError, match="beyond 2\\^20 voxels"):
                    r.add_keyframe(bad)
                assert r.num_clouds() == before


def test_keyframe_builder_on_one_handle():
    """win_size 2 and a metre between pushes: every push that completes a window emits, a keyframe of two scans of the count's size."""
    from voxel_slam_amd import vxba
    rng = np.random.default_rng(8302)
    b, r = vxba.KeyframeBuilder(2, 1.0), KR.KeyframeRef(2, 1.0)
    v6 = np.full(6, 1e-4)
    step = 0

    def pose():
        nonlocal step
        step += 1
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, float(step), 0.25, 0], dtype=np.float64)

    for k, n in enumerate(COUNTS):
        first, second = rng.uniform(-1, 1, size=(n, 3)), rng.uniform(-1, 1, size=(n, 3))
        P = pose()
        assert not b.push_scan(P, v6, first) and not r.push_scan(P, v6, first)
        if k == REFUSE_AFTER:
            bad = second.copy(); bad[n // 2, 1] = np.inf
            with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
                b.push_scan(pose(), v6, bad)
            assert b.num_buffered() == 1 and b.num_scans() == 2 * k + 1
        P = pose()
        assert b.push_scan(P, v6, second) and r.push_scan(P, v6, second), (k, n)
        same_keyframe(b, r.keyframe)
        assert b.info()["n_full"] == 2 * n and 0 < b.info()["n_down"] <= 2 * n
    b.close()


# ---- the per-scan path: the local map's two workspaces, the odometry's staging, the leased workspace of the stand-alone entry points ----

MAP_SEED = 8311           # chosen on the oracle alone, for either thread_num: its factor holds 125 voxels after the 20000-point scan, 127 after the 65-point
MAP_TAIL = 3              # one behind it, and 150 leaves lie below layer 0 from the 20000-point scan on; three more scans of 3000 let the window slide on


@pytest.mark.parametrize("thread_num", [5, 1])
def test_local_map_on_one_handle(thread_num):
    """cut_voxel -> recut, and from the full window on damping_iter -> margi -> slide, with scans of COUNTS points (win_size 3: the window is
    full at the third scan).  Under the default thread_num 5 the scans of 1 and 65 points touch fewer roots than threads and return after the descent:
    their carving is used, the shared resolve / iota / sort is not.  Under thread_num 1 every scan is pushed, so the sort runs at 1 and 65 points too.
    There a window holds a frame of 65 points beside one of 20000: the BA of such a window is ill-posed (its steps are decimetres long), the two
    optimisers' last digits grow into 1e-6 m, and a map that went on from its own poses could sort a point into another octant than the oracle's.  The
    subject is the map: the poses are held to the interface's contract of 1e-4 (tests/test_gpu_map.py) and both maps go on from the oracle's."""
    from tests.test_gpu_map import by_id, same_structure
    from tests.test_oracle_octree import PRM, point_vars, to_world
    from voxel_slam_amd import synth, vxba
    counts = COUNTS + (3000,) * MAP_TAIL
    xyz, fp, poses_gt, _ = synth.make_scans(win_size=len(counts), pts_per_scan=20000, seed=MAP_SEED)
    var = point_vars(xyz.shape[0], MAP_SEED)
    rng = np.random.default_rng(MAP_SEED)
    win = 3
    mo, mg = O.LocalMapOracle(win_size=win, thread_num=thread_num, **PRM), vxba.LocalMap(win_size=win, thread_num=thread_num, **PRM)
    fo, fg = O.Oracle(win), vxba.LidarFactor(win)
    other = vxba.LidarFactor(win + 1)
    xo, xg = [], []
    win_count = 0
    pushed, deep = {}, 0

    def same(stage):
        a, b = by_id(mo.leaves()), mg.leaves()
        same_structure(a, b, stage)
        assert np.array_equal(a["pcrs_local"], b["pcrs_local"]), stage
        return a

    for k, n in enumerate(counts):
        pose = poses_gt[k].copy(); pose[9:12] += rng.normal(0, 0.01, 3)
        s = slice(fp[k], fp[k] + n)
        win_count += 1
        for m, f, xb in ((mo, fo, xo), (mg, fg, xg)):
            xb.append(pose.copy())
            f.clear()
            m.cut_voxel(win_count - 1, xyz[s], var[s], to_world(xb[-1], xyz[s]))
        same(("cut_voxel", k, n))
        mo.recut(win_count, np.stack(xo), fo)
        npush = mg.recut(win_count, np.stack(xg), fg)
        a = same(("recut", k, n))
        assert fo.size() == fg.size() == npush, (k, n, fo.size(), fg.size(), npush)
        pushed[k] = npush
        deep = max(deep, int((a["layer"] > 0).sum()))
        if win_count < win:
            continue
        po, pg = np.stack(xo), np.stack(xg)
        if npush > 0:       # (the first full window holds 3000 + 1 + 65 points: no voxel passes the plane test yet)
            po = fo.damping_iter(po, max_iter=3, thd_num=2)["poses"]
            pg = vxba.Lidar_BA_Optimizer().damping_iter(pg, fg, max_iter=3)["poses"]
            et, er = synth.pose_errors(pg, po)
            print(f"window at scan {k} ({n} points), thread_num {thread_num}: poses {et:.2e} m, {er:.2e} rad from the oracle's")
            bound = 1e-7 if thread_num == 5 else 1e-4
            assert et < bound and er < bound, (k, n, et, er)
            if thread_num == 1:
                pg = po
        mo.margi(win_count, po, fo); mg.margi(win_count, pg, fg)
        mo.slide(1); mg.slide(1)
        xo[:] = [p for p in po[1:]]; xg[:] = [p for p in pg[1:]]
        win_count -= 1
        same(("margi", k, n))
        assert mo.counts() == mg.counts(), (k, n)
        if k == REFUSE_AFTER:
            with pytest.raises(vxba.VxbaError):
                mg.recut(win_count, np.stack(xg), other)
    assert pushed[REFUSE_AFTER] > 0 and pushed[REFUSE_AFTER + 1] > 0 and deep > 0, (pushed, deep)


def test_lio_map_update_on_one_handle():
    """COUNTS plane records a call, upserted and then half of them removed; after each call the record counts and a sweep of one fixed 2000-point
    scan against an oracle map rebuilt from the surviving leaves (tests/test_gpu_lio.py)."""
    from tests.test_gpu_lio import check_sweep
    from voxel_slam_amd import synth, vxba
    pm = synth.make_plane_map(n_roots=5000, extent=10, seed=8320)
    sc = synth.make_lio_scan(pm, n_points=2000, seed=8321)
    order = np.random.default_rng(8322).permutation(len(pm.layer))
    assert len(order) >= sum(COUNTS)
    g = vxba.LioEstimator(pm.voxel_size, pm.max_layer); g.var_init(sc.xyz)
    pnt, var = g.read_points()
    alive = np.zeros(len(order), dtype=bool)
    sent = np.zeros(len(order), dtype=bool)
    matched = 0

    def held(stage):
        nonlocal matched
        assert g.map_size() == (np.unique(pm.loc[sent], axis=0).shape[0], int(pm.is_plane[sent].sum())), stage      # records are never given back
        keep = np.nonzero(alive)[0]
        o = O.LioOracle(pm.voxel_size, pm.max_layer)
        if keep.size:
            o.map_update(pm.loc[keep], pm.layer[keep], pm.path[keep], pm.center[keep], pm.normal[keep], pm.plane_var[keep], pm.radius[keep])
        o.set_points(pnt, var)
        ro, rg = o.sweep(sc.state_init, sc.cov, want_points=True), g.sweep(sc.state_init, sc.cov, want_points=True)
        assert np.array_equal(ro["plane_of_point"] >= 0, rg["plane_of_point"] >= 0), stage
        m = ro["plane_of_point"] >= 0
        assert np.allclose(ro["sigma_of_point"][m], rg["sigma_of_point"][m], rtol=1e-11), stage
        if ro["match_num"]:
            check_sweep(rg, ro)
        matched = max(matched, int(ro["match_num"]))

    off = 0
    for k, n in enumerate(COUNTS):
        idx = order[off:off + n]; off += n
        g.map_update(pm.loc[idx], pm.layer[idx], pm.path[idx], pm.center[idx], pm.normal[idx], pm.plane_var[idx], pm.radius[idx], pm.is_plane[idx])
        sent[idx] = True; alive[idx] = pm.is_plane[idx] == 1
        held(("upsert", k, n))
        drop = idx[::2]
        g.map_update(pm.loc[drop], pm.layer[drop], pm.path[drop], pm.center[drop], pm.normal[drop], pm.plane_var[drop], pm.radius[drop], np.zeros(drop.size, dtype=np.int32))
        alive[drop] = False
        held(("remove", k, n))
    assert matched > 100


def _patches(seed, cells, lo, hi):
    """`cells` planar patches (0.4 m across, 2 cm rough) of 12 to 19 points with centres in [lo, hi)^3: the points, the cell offsets, the generator."""
    rng = np.random.default_rng(seed)
    per = rng.integers(12, 20, size=cells)
    cell_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    k = np.repeat(np.arange(cells), per)
    nrm = rng.normal(size=(cells, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = np.cross(nrm, np.array([0.31, 0.52, 0.79])); a /= np.linalg.norm(a, axis=1, keepdims=True); b = np.cross(nrm, a)
    ctr = rng.uniform(lo, hi, size=(cells, 3))
    world = ctr[k] + rng.uniform(-0.2, 0.2, (k.size, 1)) * a[k] + rng.uniform(-0.2, 0.2, (k.size, 1)) * b[k] + rng.normal(0, 0.02, (k.size, 1)) * nrm[k]
    return np.ascontiguousarray(world), cell_ptr, rng


def test_stand_alone_entry_points_on_the_leased_workspace():
    """build_clusters, plane_fit, cov_add_build and plane_update at COUNTS rows a call, with the flow and the bounds of
    tests/test_gpu_lio.py::test_plane_records_built_on_the_gpu_match_oracle: the GPU's clusters, eigen-decomposition and cov_add go into its plane_update.
    Two pools of cells, the oracle runs each once.  `near` is of the neighbour's kind: +-6 m around the sensor, covariances from var_init + pvec_update.
    cov_add's per-entry bound (rtol 1e-12 of every entry, and of its mirror image) is held on `pos`.  An entry of sum Bf_var = sum [B V B^T, B V; V B^T, V]
    adds products of coordinates and covariance entries, and with 20000 cells instead of the neighbour's few thousand some entries of `near` cancel so far
    that the oracle itself, summing a cell's points in another order, moves them by up to 6e-12 of themselves and is off its own mirror image by as much.
    In `pos` every coordinate and every covariance entry is positive, so every term of every entry is: at most 19 terms and a few roundings each keep
    any order of evaluation, fused or not, within 1e-14 of the entry, and a miss of the bound is the code's, not the conditioning's."""
    from voxel_slam_amd import vxba
    cells = max(COUNTS)
    world, cell_ptr, _ = _patches(8330, cells, -6.0, 6.0)
    o = O.LioOracle(); o.var_init(world.astype(np.float32))
    world, var = o.pvec_update(np.concatenate([np.eye(3).reshape(9), np.zeros(15)]), np.eye(15) * 1e-6)
    cl_o = O.build_clusters(world, cell_ptr)
    ev_o, U_o = O.plane_fit(cl_o)
    ca_o = O.cov_add_build(world, var, cell_ptr)
    pl_o = O.plane_update(cl_o, ev_o, U_o, ca_o)
    pos_w, pos_ptr, rng = _patches(8332, cells, 2.0, 12.0)
    A = rng.uniform(1e-3, 1e-2, size=(pos_w.shape[0], 3, 3))
    pos_v = A @ np.transpose(A, (0, 2, 1))
    pos_v = np.ascontiguousarray((pos_v + np.transpose(pos_v, (0, 2, 1))) / 2)
    assert pos_w.min() > 0 and pos_v.min() > 0
    pos_o = O.cov_add_build(pos_w, pos_v, pos_ptr)
    for step, n in enumerate(COUNTS):
        ptr, npt = cell_ptr[:n + 1], int(cell_ptr[n])
        cl_g = vxba.build_clusters(world[:npt], ptr)
        assert np.array_equal(cl_g, cl_o[:n]), (step, n)
        ev_g, U_g = vxba.plane_fit(cl_g)
        assert np.allclose(ev_g, ev_o[:n], rtol=1e-9, atol=1e-13), (step, n)
        pos_g = vxba.cov_add_build(pos_w[:int(pos_ptr[n])], pos_v[:int(pos_ptr[n])], pos_ptr[:n + 1])
        print(f"cov_add_build {n} cells: entries within {float((np.abs(pos_g - pos_o[:n]) / pos_o[:n]).max()):.2e} of the oracle's")
        assert np.allclose(pos_g, pos_o[:n], rtol=1e-12, atol=1e-22) and np.allclose(pos_g, np.transpose(pos_g, (0, 2, 1)), rtol=1e-12, atol=1e-22), (step, n)
        ca_g = vxba.cov_add_build(world[:npt], var[:npt], ptr)
        pl_g = vxba.plane_update(cl_g, ev_g, U_g, ca_g)
        sgn = np.sign(np.sum(pl_g["normal"] * pl_o["normal"][:n], axis=1))
        print(f"plane_update {n} rows: normals within {float(np.abs(pl_g['normal'] * sgn[:, None] - pl_o['normal'][:n]).max()):.2e}, "
              f"{int((pl_g['radius'] != pl_o['radius'][:n]).sum())} radii differ")
        assert np.all(np.abs(sgn) == 1) and np.allclose(pl_g["normal"] * sgn[:, None], pl_o["normal"][:n], atol=1e-9), (step, n)
        assert np.allclose(pl_g["center"], pl_o["center"][:n], rtol=1e-15) and np.array_equal(pl_g["radius"], pl_o["radius"][:n]), (step, n)
        S = np.ones((n, 6)); S[:, :3] = sgn[:, None]
        pv_g = pl_g["plane_var"] * S[:, :, None] * S[:, None, :]
        scale = np.abs(pl_o["plane_var"][:n]).max(axis=(1, 2), keepdims=True)
        assert np.all(np.abs(pv_g - pl_o["plane_var"][:n]) <= 1e-7 * scale), (step, n)       # 1/(lambda_0 - lambda_k) amplifies the eigen-solvers' 1e-13
