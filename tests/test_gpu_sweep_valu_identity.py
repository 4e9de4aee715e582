"""The sweeps' results, bit for bit, at the smallest shapes at which their lane roles, masks and address expressions differ (run with ``-m gpu``).

The residual half of the fused launch (csrc/vxba_k23.hpp), the stand-alone residual sweep (k2_residual_kernel) and phase A of the Hessian sweep
(csrc/vxba_k3.hpp) are worked over for the instructions they issue, never for the arithmetic: same fp64 operations in the same order.  So every
array below must equal, byte for byte, what the library computed BEFORE that work.  The fixtures tests/golden/valu_identity/w<W>_v<V>.npy were
recorded on an MI355X from the commit before it (``python -m tests.test_gpu_sweep_valu_identity --record``); one flat float64 array per case,
`_layout` names its pieces.  No CPU reference is involved: no case is left out, and nothing is compared to a tolerance except the two forms of
the loop against each other, with the literals of tests/test_gpu_parity.py::test_fused_launch_is_the_three_launch_iteration_to_round_off.

Shapes.  W in {1, 2, 3, 9, 10}: odd W gives the upper lane of a pair an empty last slot, W <= 3 the small-pair MFMA waves.  V in {1, 7, 33, 197,
515}: a wave with one lane pair, a tail wave with a few pairs, a workgroup run that is no multiple of 32 voxels, more than one workgroup, and
(515) stand-alone sweeps over a sub-range whose head and end sit inside a batch.  At these sizes a fused launch always takes the lane-pair form
of the residual half (no workgroup owns more than 256 voxels) and lm_steps has no head / end; the one-lane form is reached through the
launcher's own switch VXBA_K23_PAIR=0, which a process reads once: test_one_lane_form_of_the_fused_launch runs those cases in a child process.

The mask of a window (`_scene`), by voxel index a: a % 5 == 1 leaves the lower half of the frames [0, H1) unobserved, a % 5 == 2 the upper half
[H1, W), a % 5 == 4 every other frame; a % 5 in {2, 3} has no fix cluster, the others have one; at W >= 3 NO voxel observes frame W - 1; the
unobserved rows of every third voxel hold N == 0 beside non-zero moments (what a select on N is for: an all-zero row would add zeros anyway).

The two forms of the loop against each other, on every window.  The parity test's pose bound (1e-11 m) is set on a 2000-voxel window; it is
asserted as it stands from V = 33 on.  A pose difference between the forms is a last-bit difference of the merged clusters (lane pair against
running sum) divided, to first order, by the smallest eigenvalue of the damped, Marquardt-scaled system the step solves, lambda_min(D^-1/2 H
D^-1/2) + u with D = diag H and u >= 0.01 / 9 inside a three-step solve (u starts at 0.01 and an accepted step divides it by at most 3).  One
plane fixes three of a pose's six degrees of freedom, so the 1- and 7-voxel windows are rank-deficient or nearly so (lambda_min 1e-16 ... 3e-3
against >= 1.2e-2 from V = 33 on) and their bound is the literal times the ratio of that effective eigenvalue at the least determined V >= 33
window of the same W to the window's own -- both taken from the RECORDED Hessians (`k3_H` of the fixtures), not from the library under test.
W = 1: the only pose is the gauge; no form may move it at all (asserted: byte-equal to the initial pose), and accepted / rejected is then the
sign of a difference of equal residuals, so only the step total is compared there."""
import os
import subprocess
import sys

import numpy as np
import pytest

from voxel_slam_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "valu_identity")
WS = (1, 2, 3, 9, 10)
VS = (1, 7, 33, 197, 515)
ONE_LANE = ((9, 515), (10, 515))
LM_STEPS, PER_SOLVE = 6, 3


def _scene(W, V):
    sc = synth.make_scene(win_size=W, pts_per_scan=40 * V, n_voxels=V, fix_frac=1.0, seed=3100 + 16 * W + V, rot_sigma_deg=0.1, trans_sigma=0.03)
    H1 = (W + 1) // 2
    cl, fix = sc.clusters.copy(), sc.fix.copy()
    a = np.arange(V)
    cl[np.ix_(a % 5 == 1, np.arange(W) < H1)] = 0.0
    cl[np.ix_(a % 5 == 2, np.arange(W) >= H1)] = 0.0
    cl[np.ix_(a % 5 == 4, np.arange(W) % 2 == 1)] = 0.0
    if W >= 3:
        cl[:, W - 1] = 0.0
    fix[(a % 5 == 2) | (a % 5 == 3)] = 0.0
    # every third voxel: its unobserved rows keep N == 0 but carry finite non-zero moments (a caller's stale row, which push_voxels copies as it
    # is): the reference skips a frame on N alone (voxel_map.hpp:258), and so must every select on N in the sweeps
    stale = (cl[:, :, 9] == 0.0) & (a % 3 == 0)[:, None]
    cl[stale, :9] = np.array([3.0, -0.5, 0.25, 2.0, 0.125, 1.5, -1.0, 0.5, 2.0])
    coe = 0.5 + 1.5 * ((7 * a) % 11) / 10.0
    return sc, np.ascontiguousarray(cl), fix, coe


def _layout(W, V):
    """(name, length) of the pieces of a case's fixture, in order."""
    n = 6 * W
    sub = V >= 33
    L = [("inputs_sum", 4), ("k2_residual", 1), ("k2_eigval", 3 * V), ("k2_eigvec", 9 * V), ("k2_merged", 10 * V),
         ("k3_H", n * n), ("k3_J", n), ("k3_r", 1)]
    if sub:
        L += [("sub_k2_residual", 1), ("sub_k3_H", n * n), ("sub_k3_J", n), ("sub_k3_r", 1)]
    L += [("three_poses", 12 * W), ("three_resis", 2), ("three_stats", 3),
          ("fused_poses", 12 * W), ("fused_resis", 2), ("fused_stats", 3), ("fused_eigval", 3 * V), ("fused_eigvec", 9 * V), ("fused_merged", 10 * V)]
    return L


def _split(W, V, flat):
    out, o = {}, 0
    for name, ln in _layout(W, V):
        out[name] = flat[o:o + ln]
        o += ln
    assert o == flat.size, (o, flat.size)
    return out


def _loop(vxba, W, cl, fix, coe, poses, fused):
    f = vxba.LidarFactor(W)
    f.push_voxels(cl, fix, coe)
    f.evaluate_only_residual(poses)
    f.set_option("fused_sweeps", fused)
    f.snapshot_cache()
    p, r, st = f.lm_steps(poses, LM_STEPS, PER_SOLVE)
    cache = f.read_cache()
    f.close()
    return p, r, np.array([st["iters"], st["accepted"], st["rejected"]], dtype=np.float64), cache


def compute(vxba, W, V, only_fused=False):
    """Every piece of `_layout` through the public API (only_fused: the fused loop's pieces alone)."""
    sc, cl, fix, coe = _scene(W, V)
    poses = sc.poses_init
    got = {"inputs_sum": np.array([cl.sum(), fix.sum(), coe.sum(), poses.sum()])}
    if not only_fused:
        f = vxba.LidarFactor(W)
        f.push_voxels(cl, fix, coe)
        got["k2_residual"] = np.array([f.evaluate_only_residual(poses)])
        got["k2_eigval"], got["k2_eigvec"], got["k2_merged"] = f.read_cache()
        H, J, r = f.acc_evaluate2(poses)
        got["k3_H"], got["k3_J"], got["k3_r"] = H, J, np.array([r])
        if V >= 33:
            head, end = 3, V - 4
            got["sub_k2_residual"] = np.array([f.evaluate_only_residual(poses, head, end)])
            H, J, r = f.acc_evaluate2(poses, head, end)
            got["sub_k3_H"], got["sub_k3_J"], got["sub_k3_r"] = H, J, np.array([r])
        f.close()
        got["three_poses"], got["three_resis"], got["three_stats"], _ = _loop(vxba, W, cl, fix, coe, poses, 0)
    got["fused_poses"], got["fused_resis"], got["fused_stats"], (got["fused_eigval"], got["fused_eigvec"], got["fused_merged"]) = _loop(vxba, W, cl, fix, coe, poses, 2)
    return {k: np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for k, v in got.items()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _golden(W, V, suffix=""):
    return _split(W, V, np.load(os.path.join(GOLDEN, f"w{W}_v{V}{suffix}.npy")))


def _assert_identical(got, ref, names):
    assert np.array_equal(_bits(got["inputs_sum"]), _bits(ref["inputs_sum"])), "the window itself differs from the recorded one (numpy / libm), not the library"
    bad = []
    for name in names:
        same = np.array_equal(_bits(got[name]), _bits(ref[name]))
        with np.errstate(invalid="ignore"):
            d = np.abs(got[name] - ref[name])
        print(f"  {name:16s} {'identical' if same else 'DIFFERS'}  max|diff| {np.nanmax(d) if d.size else 0.0:.3e}  ({int((_bits(got[name]) != _bits(ref[name])).sum())} of {d.size} values)")
        if not same:
            bad.append(name)
    assert not bad, f"not byte-identical to the recorded results: {bad}"


@pytest.fixture(scope="module")
def vx():
    from voxel_slam_amd import vxba
    vxba.load_library()
    return vxba


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("W", WS)
def test_sweeps_and_both_loop_forms_keep_their_bits(vx, W, V):
    got = compute(vx, W, V)
    ref = _golden(W, V)
    _assert_identical(got, ref, [n for n, _ in _layout(W, V) if n != "inputs_sum"])
    # the two forms of the loop against each other: tests/test_gpu_parity.py::test_fused_launch_is_the_three_launch_iteration_to_round_off, bench-driver leg
    d_pose = np.abs(got["fused_poses"] - got["three_poses"]).max()
    atol = _pose_bound(W, V)
    print(f"  fused vs three launches: poses {d_pose:.2e} (bound {atol:.2e})  residual {abs(got['fused_resis'][1] / got['three_resis'][1] - 1):.2e}  steps {got['fused_stats']} {got['three_stats']}")
    assert got["fused_stats"][0] == got["three_stats"][0] == LM_STEPS
    if W >= 2:
        assert np.array_equal(got["fused_stats"], got["three_stats"]), (got["fused_stats"], got["three_stats"])
    else:   # the gauge pose stays where it is, bit for bit, in both forms
        p0 = _scene(W, V)[0].poses_init.reshape(-1)
        assert np.array_equal(_bits(got["fused_poses"]), _bits(p0)) and np.array_equal(_bits(got["three_poses"]), _bits(p0))
    assert np.isclose(got["fused_resis"][1], got["three_resis"][1], rtol=1e-10)
    assert np.allclose(got["fused_poses"], got["three_poses"], rtol=0, atol=atol), (d_pose, atol)


U_MIN = 0.01 / 9.0   # smallest damping inside a three-step solve: lm_decide starts a solve at u = 0.01, an accepted step multiplies it by >= 1 / 3


def _lambda_eff(W, V):
    """Smallest eigenvalue of the recorded Hessian at the initial poses, Marquardt-scaled over the frames that have a block at all, + U_MIN."""
    n = 6 * W
    H = _golden(W, V)["k3_H"].reshape(n, n)
    d = np.abs(np.diag(H))
    live = d > 0
    Hs = H[np.ix_(live, live)] / np.sqrt(np.outer(d[live], d[live]))
    return float(np.abs(np.linalg.eigvalsh(Hs)).min()) + U_MIN


def _pose_bound(W, V):
    """1e-11 (the parity test's literal) from V = 33 on; below, scaled by how much less the window determines its poses (module docstring)."""
    if V >= 33:
        return 1e-11
    ref = min(_lambda_eff(W, v) for v in VS if v >= 33)
    return 1e-11 * max(1.0, ref / _lambda_eff(W, V))


def test_one_lane_form_of_the_fused_launch():
    """k23_finish (one lane per voxel) at V = 515: a child process with VXBA_K23_PAIR=0 computes the fused loop's pieces and compares them itself."""
    env = dict(os.environ, VXBA_K23_PAIR="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_sweep_valu_identity", "--check-one-lane"], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


FUSED_NAMES = ["fused_poses", "fused_resis", "fused_stats", "fused_eigval", "fused_eigvec", "fused_merged"]


def _one_lane(vxba, W, V):
    got = compute(vxba, W, V, only_fused=True)
    return np.concatenate([got[n] for n in ["inputs_sum"] + FUSED_NAMES])


def _main(argv):
    from voxel_slam_amd import vxba
    vxba.load_library()
    if "--record" in argv:
        out = argv[argv.index("--record") + 1] if len(argv) > argv.index("--record") + 1 else GOLDEN
        os.makedirs(out, exist_ok=True)
        if os.environ.get("VXBA_K23_PAIR") == "0":
            for W, V in ONE_LANE:
                np.save(os.path.join(out, f"w{W}_v{V}_one_lane.npy"), _one_lane(vxba, W, V))
            return 0
        for W in WS:
            for V in VS:
                got = compute(vxba, W, V)
                flat = np.concatenate([got[n] for n, _ in _layout(W, V)])
                finite = all(np.isfinite(v).all() for v in got.values())
                print(f"W {W:2d} V {V:3d}: {flat.size} doubles  finite {finite}  stats three {got['three_stats']} fused {got['fused_stats']}  "
                      f"poses fused-three {np.abs(got['fused_poses'] - got['three_poses']).max():.2e}  resis {got['fused_resis']} {got['three_resis']}", flush=True)
                np.save(os.path.join(out, f"w{W}_v{V}.npy"), flat)
        return 0
    if "--check-one-lane" in argv:
        assert os.environ.get("VXBA_K23_PAIR") == "0"
        rc = 0
        for W, V in ONE_LANE:
            flat, ref = _one_lane(vxba, W, V), np.load(os.path.join(GOLDEN, f"w{W}_v{V}_one_lane.npy"))
            same = flat.size == ref.size and np.array_equal(_bits(flat), _bits(ref))
            print(f"W {W} V {V} one-lane fused loop: {'identical' if same else 'DIFFERS'}")
            rc |= 0 if same else 1
        return rc
    return 2


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
