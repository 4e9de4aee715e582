"""Loop-edge registration end to end and timed (vxba_loopreg_*, hba.loop_registration -> hba.loop_graph), next to the numpy checker.

    python scripts/run_loop_icp.py [--out profiles/loopreg/loop_icp.json] [--reps 20]

1. A corridor_session revisit with drifted odometry: the last keyframe against three early ones -> plane clouds, scores, ICP, loop edges ->
   pose graph -> poses; the same through the checker (tests/_loopreg_ref.py), edges and end-point error side by side.
2. Wall time of vxba_loopreg_icp on ~2 000-plane clouds: one pair and a batch of 32 (median over --reps calls, host synchronisation included),
   of the score of 64 hypotheses and of one keyframe's plane extraction; next to them the checker's time for one pair and -- where the reference's
   sources are present -- the time of the reference's own icp_normal behind tests/golden/loop_icp/ref_icp.cpp (brute-force nearest neighbour, CPU).
Records, not bars."""
import argparse
import importlib.util
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
    pass

import numpy as np  # noqa: E402

from tests import _loopreg_cases as K  # noqa: E402
from tests import _loopreg_ref as R  # noqa: E402
from voxel_slam_amd import hba, vxba  # noqa: E402


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {}

    # ---- 1. the revisit ----
    rv = K.revisit()
    t0 = time.perf_counter()
    got = hba.loop_registration(rv["cloud_cur"], rv["candidates"], rv["guesses"], rv["cur_index"])
    t_gpu = time.perf_counter() - t0
    chk = K.CheckerRegistration()
    t0 = time.perf_counter()
    ref = hba.loop_registration(rv["cloud_cur"], rv["candidates"], rv["guesses"], rv["cur_index"], reg_cls=lambda: chk)
    t_chk = time.perf_counter() - t0
    dev = np.max([R.pose_diff(R.pose_of(x["rot"], x["tra"]), R.pose_of(y["rot"], y["tra"])) for x, y in zip(got["edges"], ref["edges"])], axis=0)
    out = hba.loop_graph(rv["poses"], got["edges"], K.E2E["v6"])
    before = float(np.linalg.norm(rv["poses"][-1, 9:] - rv["gt"][-1, 9:])); after = float(np.linalg.norm(out["poses"][-1, 9:] - rv["gt"][-1, 9:]))
    print(f"revisit: {len(got['edges'])} edges of {len(rv['candidates'])} candidates; score {np.round(got['score'], 3).tolist()}; iterations {got['report'][:, 2].astype(int).tolist()}; "
          f"match_num {got['report'][:, 3].astype(int).tolist()}")
    print(f"revisit: edges vs checker {dev[0]:.2e} m {dev[1]:.2e} rad; end-point error {before:.4f} m -> {after:.4f} m; "
          f"loop_registration {1e3 * t_gpu:.1f} ms on the GPU (first call, plane extraction of 4 x {rv['cloud_cur'].shape[0]} points included), checker {1e3 * t_chk:.0f} ms")
    res["revisit"] = dict(edges=len(got["edges"]), edge_dev_m=float(dev[0]), edge_dev_rad=float(dev[1]), end_error_before_m=before, end_error_after_m=after,
                          gpu_first_call_ms=1e3 * t_gpu, checker_ms=1e3 * t_chk)

    # ---- 2. timings ----
    kf = K.keyframes()
    cl = K.icp_clouds()
    src, tar = kf["planes"][2]["rows"], kf["planes"][0]["rows"]
    guess = K.perturbed(K.pair_truth(kf, 2, 0), (1.5, -1.0, 2.0), (0.25, -0.2, 0.15))
    rng = np.random.default_rng(5)
    guesses32 = np.stack([K.perturbed(K.pair_truth(kf, 2, 0), rng.uniform(-2, 2, 3), rng.uniform(-0.3, 0.3, 3)) for _ in range(32)])
    sst, sposes = K.score_batch()
    with vxba.LoopRegistration() as r:
        s, t = r.add_cloud(src), r.add_cloud(tar)
        one = r.icp([[s, t]], guess[None])
        res["icp_one_pair_ms"] = median_ms(lambda: r.icp([[s, t]], guess[None]), a.reps)
        b32 = r.icp([[s, t]] * 32, guesses32)
        res["icp_32_pairs_ms"] = median_ms(lambda: r.icp([[s, t]] * 32, guesses32), a.reps)
        ids = [r.add_cloud(p["rows"]) for p in kf["planes"]]
        pairs = np.array([[ids[x], ids[y]] for x, y in sst], dtype=np.int32)
        res["score_64_ms"] = median_ms(lambda: r.score(pairs, sposes, *K.SCORE_THRESHOLDS), a.reps)
        res["add_keyframe_240k_points_ms"] = median_ms(lambda: r.add_keyframe(kf["clouds"][0]), max(3, a.reps // 4))
        res["sizes"] = dict(source_planes=int(src.shape[0]), target_planes=int(tar.shape[0]), one_pair_iterations=int(one["iterations"][0]),
                            batch_iterations=sorted(set(b32["iterations"].tolist())), batch_accepted=int(b32["accept"].sum()), launches=int(b32["launches"]), host_syncs=int(b32["host_syncs"]))
    t0 = time.perf_counter(); c = R.icp(src, tar, guess); res["checker_one_pair_ms"] = 1e3 * (time.perf_counter() - t0)
    assert c["iterations"] == res["sizes"]["one_pair_iterations"]
    res["reference_one_pair_ms"] = None
    spec = importlib.util.spec_from_file_location("make_golden_loop_icp", os.path.join(ROOT, "tests", "golden", "loop_icp", "make_golden_loop_icp.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    if os.path.exists(os.path.join(G.REF_SRC, "loop_refine.hpp")):
        with tempfile.TemporaryDirectory() as td:
            L, _ = G.load_reference(G.compile_harness(td))
            res["reference_one_pair_ms"] = median_ms(lambda: G.ref_icp(L, src, tar, guess, 14.0), 5, warmup=1)
    print(f"icp, {src.shape[0]} x {tar.shape[0]} planes: one pair {res['icp_one_pair_ms']:.3f} ms ({res['sizes']['one_pair_iterations']} iterations), 32 pairs {res['icp_32_pairs_ms']:.3f} ms "
          f"(iterations {res['sizes']['batch_iterations']}); {res['sizes']['launches']} launches, {res['sizes']['host_syncs']} host synchronisations per call")
    print(f"score of 64 hypotheses {res['score_64_ms']:.3f} ms; plane cloud of a 240 000-point keyframe {res['add_keyframe_240k_points_ms']:.3f} ms")
    print(f"checker (numpy, one pair) {res['checker_one_pair_ms']:.0f} ms; reference icp_normal behind the shim (one pair, CPU) "
          + (f"{res['reference_one_pair_ms']:.0f} ms" if res["reference_one_pair_ms"] is not None else "not present here"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
