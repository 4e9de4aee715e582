"""The host launchers of csrc/vxba_kernels.hip with and without dispatch events (run with ``-m gpu``): set_profiling bits 1, 2 and 32 switch
launch_k3_hessian, launch_k2_residual and launch_k23_fused to the launch whose events are tied to the dispatch (vxk::launch, csrc/vxba_launch.hpp),
vxba_voxelize_profile does the same for launch_k1_build_aos inside the voxeliser.  Events time a kernel, they must not change what it computes, which
instantiation runs or how often.

One factor per (W, V, precision): synth.make_scene at W in {1, 3, 10} (the two NPAIR regimes of the Hessian sweep and an odd window with padding
columns) and V in {1, 65, 515} (one lane; one voxel past a wave; several workgroups with a ragged tail), all well-posed scenes.  The same sequence
runs three times on it -- unprofiled, profiled (1 | 2 | 4 | 32), unprofiled -- and a second profiled time for the counts:
    acc_evaluate2, evaluate_only_residual, damping_iter with fused_sweeps 1, damping_iter with fused_sweeps 0.
Every sweep warm-starts from the decomposition the one before it left in the factor, and acc_evaluate2 and an LM call linearise on the cache of their
entry poses.  So each run of the sequence first puts the factor back where the first run found it (clear, push_voxels with a zero cache), and a residual sweep at the
initial poses stands in front of acc_evaluate2 and of either LM call, as in upstream's loop; those sweeps are part of the sequence, profiled and
compared like the rest.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROFILED = 1 | 2 | 4 | 32
WS, VS, PRECISIONS = (1, 3, 10), (1, 65, 515), ("f64", "mixed", "mixed_f32_clusters")


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


_SCENES = {}


def _scene(W, V):
    from voxel_slam_amd import synth
    if (W, V) not in _SCENES:
        _SCENES[W, V] = synth.make_scene(win_size=W, pts_per_scan=40 * V, n_voxels=V, fix_frac=0.3, seed=1000 + 37 * W + V)
    return _SCENES[W, V]


def _sequence(vx, f, sc):
    """The sequence, from a freshly pushed factor; every array and scalar it returns, as bytes."""
    f.clear()
    V = sc.n_voxels     # a zero cache: clear() keeps the rows of the run before, and the first sweep would warm-start from them; zeros are no basis, it starts cold
    f.push_voxels(sc.clusters, sc.fix, sc.coe, np.zeros((V, 3)), np.zeros((V, 9)), np.zeros((V, 10)))
    out = [np.float64(f.evaluate_only_residual(sc.poses_init))]
    H, J, r = f.acc_evaluate2(sc.poses_init)
    out += [H, J, np.float64(r), np.float64(f.evaluate_only_residual(sc.poses_gt))]
    for fused in (1, 0):
        f.set_option("fused_sweeps", fused)
        out.append(np.float64(f.evaluate_only_residual(sc.poses_init)))     # an LM call linearises on the cache of its entry poses, like upstream

        got = vx.Lidar_BA_Optimizer().damping_iter(sc.poses_init, f, max_iter=3)
        out += [got["poses"], got["hess"], got["resis"], got["trace"], np.int64(got["is_converge"])]
    return [np.asarray(a).tobytes() for a in out]


def _counts(f):
    kt = f.kernel_times()
    return {**{k: v["calls"] for k, v in kt.items()}, "fused": f.fused_time()["calls"]}


def _run_case(vx, W, V, precision):
    """Unprofiled, profiled, unprofiled, profiled.  Returns the fused launches of a profiled run."""
    sc = _scene(W, V)
    f = vx.LidarFactor(W)
    f.set_precision(precision)
    plain = _sequence(vx, f, sc)
    c0 = _counts(f)
    assert not any(c0.values()), c0
    f.set_profiling(PROFILED)
    with_events = _sequence(vx, f, sc)
    c1 = _counts(f)
    times = {**f.kernel_times(), "fused": f.fused_time()}
    f.set_profiling(0)
    plain_again = _sequence(vx, f, sc)
    assert _counts(f) == c1, "an unprofiled run moved the counts"
    assert with_events == plain, f"W {W} V {V} {precision}: events changed a result"
    assert plain_again == plain, f"W {W} V {V} {precision}: the run after the profiled one differs"
    # each kind that ran: three residual sweeps outside the LM calls and those inside, one Hessian sweep + reduction per acc_evaluate2 and LM call
    ran = ["k3_hessian", "k2_residual", "k3_finalize"] + (["fused"] if c1["fused"] else [])
    for kind in ran:
        assert c1[kind] > 0 and np.isfinite(times[kind]["ms_sum"]) and times[kind]["ms_sum"] > 0, (kind, c1, times)
    assert c1["k1_build"] == 0 and c1["k2_residual"] >= 4 and c1["k3_hessian"] >= 2
    # the fused launch: the first LM call runs it where the factor allows it (csrc/vxba_capi_core.hip, fused_sweeps) -- never on f32 cluster rows
    assert (c1["fused"] > 0) == (precision != "mixed_f32_clusters"), c1
    f.set_profiling(PROFILED)
    assert _sequence(vx, f, sc) == plain
    c2 = _counts(f)
    assert {k: c2[k] - c1[k] for k in c1} == c1, "two profiled runs of one sequence count differently"
    return c1["fused"]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("W", WS)
def test_events_change_nothing(vx, W, V, precision):
    _run_case(vx, W, V, precision)


@pytest.mark.parametrize("n_cells", (1, 16, 17, 1025))
def test_cluster_build_under_the_voxeliser_profile(vx, n_cells):
    """build_clusters while vxba_voxelize_profile is on and off: one, sixteen (one row group of k1_build_rows_kernel), seventeen and 1025 cells.  (The
    stand-alone entry point passes no events whatever the profile says; the voxeliser below does.)"""
    rng = np.random.Generator(np.random.PCG64(n_cells))
    counts = rng.integers(1, 40, size=n_cells)
    counts[0] = 300 if n_cells > 1 else 5                                  # one long cell for k1_long_cells_kernel
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    xyz = rng.uniform(-3, 3, size=(int(ptr[-1]), 3))
    off = vx.build_clusters(xyz, ptr)
    vx.voxelize_profile(True)
    try:
        on = vx.build_clusters(xyz, ptr)
    finally:
        vx.voxelize_profile(False)
    assert on.tobytes() == off.tobytes() and np.array_equal(off[:, 9], counts)


def test_voxeliser_cluster_build_with_events(vx):
    """launch_k1_build_aos with events: voxelize_push under the profile gives the factor it gives without, and the profile saw launches."""
    from voxel_slam_amd import synth
    xyz, fp, poses, _ = synth.make_scans(win_size=3, pts_per_scan=3000)
    P = vx.VoxelizeParams(voxel_size=1.0, max_layer=2, min_points=10, min_eigen_value=0.01, eigen_ratio=(1 / 16, 1 / 16, 1 / 9, 1 / 9))

    def run():
        f = vx.LidarFactor(3)
        ids = f.voxelize_push(xyz, fp, poses, P)
        return ids.tobytes(), f.read_clusters().tobytes()
    off = run()
    vx.voxelize_profile(True)
    try:
        on = run()
    finally:
        prof = vx.voxelize_profile(False)
    assert on == off and len(off[0]) > 0
    assert prof["launches"] > 0 and prof["launches"] % 2 == 0 and np.isfinite(prof["ms_sum"]) and prof["ms_sum"] > 0


def _child(mode, **env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_launch_variants", mode], cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_one_lane_form_of_the_fused_launch():
    """VXBA_K23_PAIR=0 is read once per process: the W = 10, V = 515 case in a child (started like tests/test_gpu_sweep_exact.py starts its own)."""
    _child("--one-lane", VXBA_K23_PAIR="0")


def test_first_call_of_a_process_is_a_profiled_fused_launch():
    """Where an LDS opt-in of another instantiation than the one launched would show: nothing has been opted in yet, and the very first vxba call that
    launches the fused kernel (147 KB of LDS at W = 10) does so with events."""
    _child("--first-call")


def _main(argv):
    from voxel_slam_amd import vxba
    if "--one-lane" in argv:
        assert os.environ.get("VXBA_K23_PAIR") == "0"
        vxba.load_library()
        assert _run_case(vxba, 10, 515, "f64") > 0
        return 0
    if "--first-call" in argv:
        sc = _scene(10, 515)
        f = vxba.LidarFactor(10)
        f.set_profiling(PROFILED)
        f.push_voxels(sc.clusters, sc.fix, sc.coe)
        f.evaluate_only_residual(sc.poses_init)                                        # the cache of the entry poses; this launch needs no opt-in
        got = vxba.Lidar_BA_Optimizer().damping_iter(sc.poses_init, f, max_iter=3)     # raises unless the call returns VXBA_OK
        assert f.fused_time()["calls"] > 0 and np.isfinite(got["poses"]).all() and np.isfinite(got["resis"]).all()
        return 0
    return 2


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
