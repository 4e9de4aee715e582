"""Times the top-down half of the global BA on one GPU: vxba.PoseGraph.optimize on the pose graph of the 500-keyframe corridor session of
BASELINE configs[4] -- odometry chain + prior + the edges of both levels from vxba_hba_pass -- next to the pass that produced the edges and
to the numpy checker (tests/_pgo_ref.py, dense Cholesky) on the same graph.  Wall clock around calls that end in a device synchronisation;
median of --repeats after --warmup.  --profile-run: one pass + optimisations only, no checker (for rocprofv3 --kernel-trace --stats)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from voxel_slam_amd import hba, synth, vxba

ap = argparse.ArgumentParser()
ap.add_argument("--keyframes", type=int, default=500)
ap.add_argument("--pts", type=int, default=20_000)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--profile-run", action="store_true")
a = ap.parse_args()
K = a.keyframes
clouds, poses, gt = synth.corridor_session(K, a.pts, synth.MASTER_SEED + 5000)
coarse = vxba.VoxelizeParams(voxel_size=2.0, max_layer=2, min_points=10, min_eigen_value=0.02, eigen_ratio=(1 / 9, 1 / 9, 1 / 9, 1 / 9))
fine = vxba.VoxelizeParams(voxel_size=1.0, max_layer=2, min_points=10, min_eigen_value=0.01, eigen_ratio=(1 / 16, 1 / 16, 1 / 9, 1 / 9))
ses = vxba.HbaSession()
ses.add_keyframes(clouds)
t_pass = []
for _ in range(3 if a.profile_run else a.warmup + 5):
    t = time.perf_counter()
    up = ses.run_pass(poses, coarse, fine, wdsize=10, mgsize=5, top_max_iter=2, n_threads=4)
    t_pass.append(time.perf_counter() - t)
ses.close()
# the session's keyframe poses are the truth perturbed independently by 0.05 deg / 0.02 m: a relative pose between neighbours is off by sqrt(2) of that
odom_v6 = np.array([2 * np.deg2rad(0.05) ** 2] * 3 + [2 * 0.02 ** 2] * 3)
g = vxba.PoseGraph(poses)
g.add_priors([0], poses[:1], np.full((1, 6), hba.PRIOR_V6))
g.add_edges(*hba.chain_edges(poses, odom_v6))
g.add_edges(up["edges1"], None)
g.add_edges(up["edges2"], None)
t_opt = []
for _ in range(a.warmup + a.repeats):
    g.set_poses(poses)
    t = time.perf_counter()
    out = g.optimize()
    t_opt.append(time.perf_counter() - t)
t_opt = np.array(t_opt[a.warmup:])
res = dict(keyframes=K, factors=g.num_factors(), edges=[len(up["edges1"]), len(up["edges2"])], hba_pass_s_median=float(np.median(t_pass[-5:])),
           pgo_optimize_s_median=float(np.median(t_opt)), pgo_optimize_s_min_max=[float(t_opt.min()), float(t_opt.max())], repeats=a.repeats,
           outer_iterations=len(out["report"]), cg_iterations=[r["cg_iterations"] for r in out["report"]], cg_capped=[r["cg_capped"] for r in out["report"]],
           accepted=[r["accepted"] for r in out["report"]], cost=[out["report"][0]["cost_before"], out["report"][-1]["cost_after"]],
           launches=out["launches"], host_syncs=out["host_syncs"],
           error_before_m_rad=list(synth.pose_errors(poses, gt)), error_after_m_rad=list(synth.pose_errors(out["poses"], gt)))
res["us_per_cg_iteration_upper_bound"] = 1e6 * res["pgo_optimize_s_median"] / max(1, sum(res["cg_iterations"]))
g.close()
if not a.profile_run:
    from tests import _pgo_ref as P
    ref = P.Graph(K).add_priors([0], poses[:1], np.full((1, 6), hba.PRIOR_V6)).add_edges(*hba.chain_edges(poses, odom_v6)).add_edges(*vxba.pack_edges(up["edges1"])).add_edges(*vxba.pack_edges(up["edges2"]))
    t = time.perf_counter()
    r = P.dense_lm(ref, poses)
    res["checker_dense_lm_s"] = time.perf_counter() - t
    Ra, pa = P.unpack(out["poses"]); Rb, pb = P.unpack(r["poses"])
    res["gpu_vs_checker_m_rad"] = [float(np.linalg.norm(pa - pb, axis=1).max()), float(np.linalg.norm(P.so3_log(np.transpose(Ra, (0, 2, 1)) @ Rb), axis=1).max())]
    res["checker_accepted"] = [x["accepted"] for x in r["report"]]
print(json.dumps(res), flush=True)
