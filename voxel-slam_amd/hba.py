"""One window of the hierarchical / global BA (reference: ``HBA_add_edge``, voxelslam.cpp:2320-2430) on top of the C ABI:
repeat { re-voxelise the window's scans at the current poses (OctreeGBA::cut_voxel + recut -> vxba_voxelize_push), run
Lidar_BA_Optimizer::damping_iter with up to 4 iterations } with the reference's convergence schedule (coarse voxel
parameters first, the odometry's finer ones for the last round), then turn the off-diagonal 6x6 blocks of the final Hessian
into pose-graph edge weights.  Host orchestration only -- the per-round work (hashing, octree, plane tests, sweeps, solve)
runs on the GPU; this file is the harness-level mirror used by the tests and as an integration example (config 5's bottom
level: windows of 10 keyframes on the MFMA path; the top level's ~100 submap poses go through the same calls on the wide-window
path, VXBA_MAX_WIN < W <= VXBA_MAX_WIN_WIDE).

The top-down half (``topDownProcess``, voxelslam.cpp:2231-2317) is ``top_down``: the edges of both levels, the odometry chain and a prior on the
first keyframe in one pose graph, optimised on the GPU by ``vxba.PoseGraph``; ``global_ba`` runs both halves, ``loop_graph`` is the same graph with
loop edges instead of BA edges (``build_graph``, :1741-1802)."""
from __future__ import annotations

import numpy as np

from . import vxba


def window_refine(xyz_local, frame_ptr, poses, coarse: "vxba.VoxelizeParams", fine: "vxba.VoxelizeParams", max_iter: int = 10, up: int = 4,
                  device: int = 0, factor_cls=None, optimizer=None, voxelize=None, factor=None):
    """Returns dict(poses, hess, rounds, n_voxels, resis).  ``factor_cls`` / ``optimizer`` / ``voxelize`` let the tests run the
    same schedule on the CPU oracle (defaults: the GPU path).  ``factor``: a LidarFactor of the right win_size to reuse (cleared
    before every round) instead of creating one per round -- what a long-running mapper does (the reference constructs a
    LidarFactor per round, voxelslam.cpp:2378; here that would be a dozen device allocations each time)."""
    W = poses.shape[0]
    xs = np.ascontiguousarray(poses, dtype=np.float64).copy()
    converge_flag, converge_thre = 0, 0.05
    hess = None
    log = []
    for it in range(max_iter):
        params = fine if (converge_flag == 1 or it == max_iter - 1) else coarse          # voxelslam.cpp:2362-2372
        if voxelize is None:
            if factor is not None:
                f = factor
                f.clear()
            else:
                f = vxba.LidarFactor(W, device=device) if factor_cls is None else factor_cls(W)
            n_vox = f.voxelize_push(xyz_local, frame_ptr, xs, params, want_ids=False)
        else:
            f, n_vox = voxelize(xyz_local, frame_ptr, xs, params)
        opt = vxba.Lidar_BA_Optimizer() if optimizer is None else optimizer
        if optimizer is None and int(n_vox) == 0:
            # no factor voxel (too few points for any plane): upstream's damping_iter then runs on an all-zero system -- zero step, poses unchanged,
            # *hess zero, residuals 0 and 0 / 0 -- and the schedule goes on; the GPU entry point refuses an empty factor, so that outcome is written here
            out = dict(poses=xs, hess=np.zeros((6 * W, 6 * W)), resis=(0.0, float("nan")), is_converge=False)
        else:
            out = opt.damping_iter(xs, f, max_iter=up)
        xs = out["poses"]
        hess = out["hess"]
        r0, r1 = out["resis"]
        log.append(dict(round=it, n_voxels=int(n_vox), resis=(float(r0), float(r1)), converged=bool(out["is_converge"]), fine=params is fine))
        if factor is None and hasattr(f, "close"):
            f.close()
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.float64(abs(r0 - r1)) / np.float64(r0)          # 0 / 0 for a window without factor voxels: NaN, the test below is false (as upstream)
        if (rel < converge_thre and out["is_converge"]) or (it == max_iter - 2 and converge_flag == 0):   # :2387-2398
            converge_thre = 0.01
            if converge_flag == 0:
                converge_flag = 1
            elif converge_flag == 1:
                break
    return dict(poses=xs, hess=hess, rounds=log)


def edges_from_hessian(poses, hess, min_abs: float = 1e-6):
    """Pose-graph edges of a refined window (voxelslam.cpp:2405-2427): for every frame pair whose six Hessian entries
    hess(6i+k, 6j+k) all exceed ``min_abs`` in magnitude, the relative pose and the weights v6 = 1 / |hess(6i+k, 6j+k)|."""
    W = poses.shape[0]
    R = poses[:, :9].reshape(W, 3, 3).transpose(0, 2, 1)
    p = poses[:, 9:12]
    out = []
    for i in range(W - 1):
        for j in range(i + 1, W):
            hc = np.abs(np.array([hess[6 * i + k, 6 * j + k] for k in range(6)]))
            if np.any(hc < min_abs):
                continue
            out.append(dict(i=i, j=j, rot=R[i].T @ R[j], tra=R[i].T @ (p[j] - p[i]), v6=1.0 / hc))
    return out


def merge_submap(clouds, poses, voxel_size: float, downsample=None, device: int = 0):
    """Tail of ``HBA_add_edge`` (voxelslam.cpp:2430-2450): the window's scans expressed in the FIRST frame's coordinates
    (dR = R0^T Ri, dp = R0^T (pi - p0)), stored as float like ``PointType``, then ``down_sampling_voxel(pl, voxel_size / 8)``."""
    W = poses.shape[0]
    R = poses[:, :9].reshape(W, 3, 3).transpose(0, 2, 1)
    p = poses[:, 9:12]
    parts = []
    for i in range(W):
        dR = R[0].T @ R[i]; dp = R[0].T @ (p[i] - p[0])
        parts.append((np.asarray(clouds[i], dtype=np.float64) @ dR.T + dp).astype(np.float32))
    pl = np.ascontiguousarray(np.concatenate(parts))
    ds = (lambda x, s: vxba.down_sampling_voxel(x, s, device=device)) if downsample is None else downsample
    return ds(pl, voxel_size / 8)


def windows(K: int, wdsize: int, mgsize: int, tail: bool = True):
    """[(first keyframe, keyframe count)] of one bottom-up pass: the numpy-free twin of ``vxba_hba_num_windows`` / ``vxba_hba_window`` (include/vxba.h) --
    full windows of ``wdsize`` keyframes at stride ``mgsize`` (thd_globalmapping runs one whenever localID holds wdsize keyframes and pops mgsize,
    voxelslam.cpp:2536-2541, 2571-2574) and, with ``tail``, the CLOSING window of upstream's last iteration (total_ba == 1, :2519-2523: no size test) over
    the keyframes left behind the last pop, [S mgsize, K)."""
    S = (K - wdsize) // mgsize + 1 if K >= wdsize else 0
    out = [(w * mgsize, wdsize) for w in range(S)]
    if tail and S * mgsize < K:
        out.append((S * mgsize, K - S * mgsize))
    return out


def hierarchical_ba(clouds, poses, coarse: "vxba.VoxelizeParams", fine: "vxba.VoxelizeParams", wdsize: int = 10, mgsize: int = 5, top_max_iter: int = 1,
                    device: int = 0, optimizer=None, voxelize=None, downsample=None, tail: bool = True):
    """Bottom-up pass of the global mapping thread (``thd_globalmapping``, voxelslam.cpp:2485-2595) over one session: the windows of ``windows(K, wdsize,
    mgsize, tail)``, each refined by one round of ``HBA_add_edge`` (max_iter = 1: the odometry's voxel parameters straight away, :2362-2372) and merged
    into a submap anchored at its first keyframe; then one ``HBA_add_edge`` over all submap poses (the top level, up to VXBA_MAX_WIN_WIDE of them) with
    ``top_max_iter`` rounds.  A closing window of ONE keyframe is not refined (its only pose is the gauge; its cloud is the submap).  Returns the
    pose-graph edges of both levels (``top_down`` consumes them) and the refined submap poses.
    ``clouds``: list of (n_i, 3) arrays in keyframe coordinates; ``poses``: (K, 12).  The keyword hooks run the same schedule on the
    CPU oracle in the tests."""
    K = poses.shape[0]
    sub_clouds, sub_ids, edges1 = [], [], []
    factors = {}                                                  # one factor per window size (the closing window has its own)
    for base, cnt in windows(K, wdsize, mgsize, tail):
        ids = list(range(base, base + cnt))
        if cnt >= 2:
            xyz = np.ascontiguousarray(np.concatenate([np.asarray(clouds[i], dtype=np.float64) for i in ids]))
            fp = np.concatenate([[0], np.cumsum([len(clouds[i]) for i in ids])]).astype(np.int64)
            if voxelize is None and cnt not in factors:
                factors[cnt] = vxba.LidarFactor(cnt, device=device)
            r = window_refine(xyz, fp, poses[ids], coarse, fine, max_iter=1, device=device, optimizer=optimizer, voxelize=None if voxelize is None else voxelize(cnt),
                              factor=factors.get(cnt))
            for e in edges_from_hessian(r["poses"], r["hess"]):
                edges1.append(dict(e, i=ids[e["i"]], j=ids[e["j"]]))
            refined = r["poses"]
        else:
            refined = poses[ids]
        sub_clouds.append(merge_submap([clouds[i] for i in ids], refined, fine.voxel_size, downsample=downsample, device=device))
        sub_ids.append(base)
    for f in factors.values():
        f.close()
    S = len(sub_ids)
    top_xyz = np.ascontiguousarray(np.concatenate(sub_clouds).astype(np.float64))
    top_fp = np.concatenate([[0], np.cumsum([len(c) for c in sub_clouds])]).astype(np.int64)
    if S >= 2:
        top = window_refine(top_xyz, top_fp, poses[sub_ids], coarse, fine, max_iter=top_max_iter, device=device, optimizer=optimizer,
                            voxelize=None if voxelize is None else voxelize(S))
        edges2 = [dict(e, i=sub_ids[e["i"]], j=sub_ids[e["j"]]) for e in edges_from_hessian(top["poses"], top["hess"])]
    else:
        top, edges2 = dict(poses=np.array(poses[sub_ids], dtype=np.float64), rounds=[]), []
    return dict(edges1=edges1, edges2=edges2, submap_ids=sub_ids, submap_poses=top["poses"], submap_sizes=[len(c) for c in sub_clouds], top_rounds=top["rounds"])


PRIOR_V6 = 1e-9      # variances of the prior on the first keyframe (voxelslam.cpp:1777-1782)


def chain_edges(poses, odom_v6):
    """The odometry chain of ``build_graph`` (voxelslam.cpp:1759-1766): edge k-1 -> k with the relative pose of the INPUT poses and the variances
    ``odom_v6[k-1]`` (ScanPose::v6 of keyframe k-1; one 6-vector is broadcast).  Returns (edge_ij (K-1, 2), edge_data (K-1, 18))."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    K = poses.shape[0]
    R = poses[:, :9].reshape(K, 3, 3).transpose(0, 2, 1)
    p = poses[:, 9:12]
    v6 = np.broadcast_to(np.asarray(odom_v6, dtype=np.float64).reshape(-1, 6), (K - 1, 6))
    ij = np.stack([np.arange(K - 1), np.arange(1, K)], axis=1).astype(np.int32)
    data = np.zeros((K - 1, 18))
    RiT = R[:-1].transpose(0, 2, 1)
    data[:, :9] = (RiT @ R[1:]).reshape(K - 1, 9)
    data[:, 9:12] = np.einsum("kab,kb->ka", RiT, p[1:] - p[:-1])
    data[:, 12:] = v6
    return ij, data


def _solve_graph(poses, groups, options, device, graph_cls):
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    g = vxba.PoseGraph(device=device) if graph_cls is None else graph_cls()
    try:
        g.set_poses(poses)
        g.add_priors([0], poses[:1], np.full((1, 6), PRIOR_V6))
        for ij, data in groups:
            if len(ij):
                g.add_edges(ij, data)
        out = g.optimize(options) if options is not None else g.optimize()
    finally:
        g.close()
    return out


def _as_arrays(edges):
    return edges if isinstance(edges, tuple) else vxba.pack_edges(edges)


def top_down(poses, odom_v6, edges1, edges2, options: "vxba.PgoOptions | None" = None, device: int = 0, graph_cls=None):
    """The pose graph of ``topDownProcess`` for one session: odometry chain (``chain_edges``), a prior on keyframe 0 at 1e-9 (:1777-1782), then the
    edges of the bottom and of the top level (:2247-2277) -- lists of edge dicts as ``hierarchical_ba`` returns them, or (edge_ij, edge_data) array
    pairs as ``vxba_hba_pass`` fills them.  Optimised by ``vxba.PoseGraph`` (where the reference calls ISAM2: one update + five more).  Returns
    dict(poses (K, 12), report, launches, host_syncs).  ``graph_cls``: a stand-in with the same methods (the tests run the checker through it)."""
    return _solve_graph(poses, [chain_edges(poses, odom_v6), _as_arrays(edges1), _as_arrays(edges2)], options, device, graph_cls)


def loop_graph(poses, loop_edges, default_v6, options: "vxba.PgoOptions | None" = None, device: int = 0, graph_cls=None):
    """The graph ``build_graph`` makes after a loop closure (lpedge_enable = 1) with every factor under one default variance vector (the commented
    alternative of :1764; the reference's own chain uses the per-keyframe v6 -- pass those through ``top_down`` with empty BA edges instead): chain +
    prior + loop edges.  ``loop_edges``: dicts (i, j, rot, tra[, v6]) or an (edge_ij, edge_data) pair.  Returns what ``top_down`` returns; its poses
    are what ``vxba_map_loop_update`` takes."""
    v6 = np.asarray(default_v6, dtype=np.float64).reshape(6)
    if isinstance(loop_edges, tuple):
        lp = loop_edges
    else:
        lp = vxba.pack_edges([dict(e, v6=e.get("v6", v6)) for e in loop_edges])
    return _solve_graph(poses, [chain_edges(poses, v6), lp], options, device, graph_cls)


def loop_drift(pose_target, pose_cur, tra):
    """``drift_p`` of voxelslam.cpp:2004: how far the registered edge puts the current keyframe from where odometry has it,
    |R_t tra + p_t - p_c| -- the caller's drift-to-distance test (:2013, :2044) decides whether the edge is pushed."""
    a = np.asarray(pose_target, dtype=np.float64).reshape(12); b = np.asarray(pose_cur, dtype=np.float64).reshape(12)
    return float(np.linalg.norm(a[:9].reshape(3, 3).T @ np.asarray(tra, dtype=np.float64).reshape(3) + a[9:] - b[9:]))


def loop_registration(cloud_cur, candidates, guesses, cur_index, reg: "vxba.LoopRegistration | None" = None, params: "vxba.PlaneCloudParams | None" = None,
                      score_threshold: float = 0.15, normal_threshold: float = 0.2, dis_threshold: float = 0.5, options: "vxba.IcpOptions | None" = None,
                      device: int = 0, reg_cls=None):
    """From place-recognition candidates to loop edges (voxelslam.cpp:1987-2066 without the descriptor search): every candidate's guess is scored
    (plane_geometric_verify) in one call, those above ``score_threshold`` (config icp_threshold_, BTC.cpp:32) go through icp_normal in one call,
    and every accepted pair becomes an edge dict (i = target keyframe, j = ``cur_index``, rot, tra) -- what ``lp_edges.push`` / ``add_edge``
    receive (:2061-2066) and ``loop_graph`` takes.

    ``cloud_cur`` and the clouds of ``candidates`` -- a sequence of (keyframe index, cloud) -- are (n, 3) keyframe clouds in their own frames (their
    plane clouds are built) or ids of plane clouds ``reg`` already holds; ``guesses`` (B, 12) map current-frame coordinates into each candidate's
    frame.  Returns dict(edges, report (B, 8; zero rows for candidates the score turned away), poses (B, 12), score, useful, tried, accept, ids).
    ``reg_cls``: a stand-in with LoopRegistration's methods (the tests run the checker through it)."""
    own = reg is None
    if own:
        reg = vxba.LoopRegistration(device=device) if reg_cls is None else reg_cls()
    try:
        lookup = lambda c: int(c) if np.isscalar(c) else reg.add_keyframe(c, params)
        src = lookup(cloud_cur)
        tars = [lookup(c) for _, c in candidates]
        B = len(tars)
        guesses = np.asarray(guesses, dtype=np.float64).reshape(B, 12)
        pairs = np.array([[src, t] for t in tars], dtype=np.int32).reshape(B, 2)
        sc, useful = reg.score(pairs, guesses, normal_threshold, dis_threshold)
        tried = sc > score_threshold
        poses = guesses.copy(); report = np.zeros((B, 8))
        if tried.any():
            r = reg.icp(pairs[tried], guesses[tried], options)
            poses[tried] = r["poses"]; report[tried] = r["report"]
        accept = report[:, 0] > 0
        edges = []
        for b in np.nonzero(accept)[0]:
            edges.append(dict(i=int(candidates[b][0]), j=int(cur_index), rot=poses[b, :9].reshape(3, 3).T.copy(), tra=poses[b, 9:].copy()))
        return dict(edges=edges, report=report, poses=poses, score=sc, useful=useful, tried=tried, accept=accept, ids=dict(cur=src, candidates=tars))
    finally:
        if own:
            reg.close()


def loop_search(corners_cur, cloud_cur, search: "vxba.LoopSearch", params: "vxba.LoopSearchParams | None" = None, frame_keyframes=None, detail: bool = False):
    """Place recognition for one keyframe (voxelslam.cpp:1980-1989: GenerateBtcDescs' last step + SearchLoop): ``corners_cur`` = (locations (n, 3),
    occupancy words) of the keyframe's corners (None: ``search.describe`` has been called already), ``cloud_cur`` the id of its plane cloud in the
    registration handle ``search`` is attached to.  Returns (candidates, guesses) in the form ``loop_registration`` takes: candidates a list of
    (keyframe index, plane-cloud id) -- the one frame SearchLoop returns, or empty -- and guesses (B, 12).  ``frame_keyframes``: frame -> keyframe
    index where they differ (default: the frame number).  ``detail``: the dict of ``LoopSearch.search`` as a third value.  Adds nothing to the
    database: ``search.add(cloud_cur)`` afterwards (voxelslam.cpp:2081)."""
    if corners_cur is not None:
        search.describe(corners_cur[0], corners_cur[1], params)
    r = search.search(cloud_cur, params)
    cands, guesses = [], np.zeros((0, 12))
    if r["frame"] >= 0:
        f = r["frame"]
        cands = [(int(frame_keyframes[f]) if frame_keyframes is not None else f, search.cloud_ids[f])]
        guesses = r["pose"].reshape(1, 12).copy()
    return (cands, guesses, r) if detail else (cands, guesses)


def loop_closure(corners_cur, cloud_cur, cur_index, poses, default_v6, search: "vxba.LoopSearch", reg: "vxba.LoopRegistration", params: "vxba.LoopSearchParams | None" = None,
                 icp_options: "vxba.IcpOptions | None" = None, pgo_options: "vxba.PgoOptions | None" = None, frame_keyframes=None, add: bool = True, device: int = 0):
    """From one keyframe's corners and plane cloud to the poses ``vxba_map_loop_update`` takes (voxelslam.cpp:1980-2081 + build_graph): ``loop_search``,
    then ``loop_registration`` of what it found (score gate, icp_normal), then ``loop_graph`` over ``poses`` (K, 12; keyframe ``cur_index`` is the
    current one) with the accepted edge.  ``add``: the keyframe's descriptors join the database afterwards, found or not.  Returns dict(candidates,
    guesses, search, registration (None when nothing was found), edges, poses (the optimised ones, or the input when no edge was accepted), graph)."""
    p = params if params is not None else vxba.LoopSearchParams()
    cands, guesses, found = loop_search(corners_cur, cloud_cur, search, params, frame_keyframes, detail=True)
    regis, edges, graph = None, [], None
    if cands:
        regis = loop_registration(cloud_cur, cands, guesses, cur_index, reg=reg, score_threshold=p.icp_threshold, normal_threshold=p.normal_threshold,
                                  dis_threshold=p.dis_threshold, options=icp_options)
        edges = regis["edges"]
    if edges:
        graph = loop_graph(poses, edges, default_v6, options=pgo_options, device=device)
    if add:
        search.add(cloud_cur)
    out = graph["poses"] if graph is not None else np.asarray(poses, dtype=np.float64).reshape(-1, 12).copy()
    return dict(candidates=cands, guesses=guesses, search=found, registration=regis, edges=edges, poses=out, graph=graph)


def rotate_velocities(poses_before, poses_after, velocities):
    """``ScanPose::set_state`` (loop_refine.hpp:36-43): a keyframe's velocity turns with its pose, v <- (R_new R_old^T) v."""
    a = np.asarray(poses_before, dtype=np.float64).reshape(-1, 12)[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    b = np.asarray(poses_after, dtype=np.float64).reshape(-1, 12)[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
    return np.einsum("kab,kb->ka", b @ a.transpose(0, 2, 1), np.asarray(velocities, dtype=np.float64).reshape(-1, 3))


def global_ba(clouds, poses, odom_v6, coarse: "vxba.VoxelizeParams", fine: "vxba.VoxelizeParams", wdsize: int = 10, mgsize: int = 5, top_max_iter: int = 1,
              device: int = 0, options: "vxba.PgoOptions | None" = None, tail: bool = True):
    """Both halves of the global BA over one session: ``hierarchical_ba`` (bottom-up: the edges) and ``top_down`` (the refined keyframe poses).
    Returns the bottom-up result with ``poses`` and ``pgo_report`` added."""
    up = hierarchical_ba(clouds, poses, coarse, fine, wdsize=wdsize, mgsize=mgsize, top_max_iter=top_max_iter, device=device, tail=tail)
    down = top_down(poses, odom_v6, up["edges1"], up["edges2"], options=options, device=device)
    return dict(up, poses=down["poses"], pgo_report=down["report"])


def keyframe_stream(builder: "vxba.KeyframeBuilder", reg: "vxba.LoopRegistration", session: "vxba.HbaSession", scans, params: "vxba.PlaneCloudParams | None" = None,
                    corners: "vxba.CornerExtractor | None" = None, corner_params: "vxba.CornerParams | None" = None, archive=None):
    """The hand-over between local mapping and the back end (the front half of thd_loop_closure, voxelslam.cpp:1898-1977): every ``(pose, v6, body
    points, covariances)`` of ``scans`` goes into the keyframe builder; each keyframe it emits hands its ``full`` cloud to the registration handle
    (the plane cloud of the loop chain) and the xyz of its ``down`` cloud to the hierarchical-BA session, device to device -- no cloud crosses PCIe.
    Returns one ``(id, pose, jour)`` per keyframe; keyframe k is plane cloud k of ``reg`` and keyframe k of ``session`` when both started empty.
    With ``corners`` (a ``vxba.CornerExtractor``) the ``full`` cloud also goes through the corner extraction (GenerateSTDescs without generate_std),
    device to device, and every tuple gets a fourth item ``(locations, occupancy)`` -- what ``loop_closure(corners_cur=...)`` takes.
    With ``archive`` (a ``vxba.KeyframeArchive`` or a ``handback.LoopHandback``) every keyframe's whole ``down`` cloud -- the variances included, which the
    session does not keep -- is archived as well, device to device: what the loop hand-back rebuilds the local map from."""
    out = []
    for pose, v6, pts, var in scans:
        if not builder.push_scan(pose, v6, pts, var):
            continue
        info, ptrs = builder.info(), builder.device_ptrs()
        reg.add_keyframe_device(info["n_full"], ptrs["full"], params)
        session.add_keyframes_device([info["n_down"]], ptrs["down_xyz"])
        if archive is not None:
            archive.on_keyframe(builder) if hasattr(archive, "on_keyframe") else archive.add_from(builder)
        if corners is None:
            out.append((info["id"], info["pose"], info["jour"]))
            continue
        corners.extract_device(info["n_full"], ptrs["full"], corner_params)
        c = corners.read()
        out.append((info["id"], info["pose"], info["jour"], (c["locations"], c["occupancy"])))
    return out
