"""Loop-edge registration, CPU side: the checker (tests/_loopreg_ref.py) against the reference's own icp_normal through the fixture
tests/golden/loop_icp/loop_icp.npz, the device's per-point and per-pair arithmetic (csrc/vxba_loopreg_math.hpp) compiled for the host against
the checker, and the conditions that keep the GPU tests (tests/test_gpu_loopreg.py) honest on every input they use."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import _loopreg_cases as K
from tests import _loopreg_ref as R
from voxel_slam_amd import hba, synth

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")

# A verdict of the device and of the checker can differ only where a gate quantity, a step norm or an eigenvalue lies within the scatter of two
# float64 evaluation orders (~1e-15 relative) of its threshold.  The GPU tests compare verdicts for EQUALITY, so every input they use must keep
# every such quantity at least this far from its threshold: nine orders above the scatter -- a condition on the inputs, not a tolerance.
DECISIVE = 1e-6
LAMBDA_CLEAR = 1e-9          # no voxel's smallest eigenvalue this close to plane_detection_thre
DEGENERATE_GAP = 1e-3        # (lambda1 - lambda0) / lambda2 below this: the normal's direction is ill-conditioned; at most 1 % of the plane voxels
CHECKER_FACTOR = 10.0        # the checker reproduces the fixture's reference poses within this times the difference measured at generation time


@pytest.fixture(scope="module")
def G():
    spec = importlib.util.spec_from_file_location("tests._make_golden_loop_icp", os.path.join(HERE, "golden", "loop_icp", "make_golden_loop_icp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "loopreg_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libloopreg_hostcheck.so")
    hdr = os.path.join(HERE, "..", "voxel-slam_amd", "csrc", "vxba_loopreg_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.lrh_gate.argtypes = [C.c_int, f64p, f32p, f32p, f64p, f64p, f64p, u8p, f64p]
    L.lrh_jac.argtypes = [C.c_int, f64p, f32p, f32p, f64p]
    L.lrh_accumulate.argtypes = [C.c_int, f64p, f32p, f32p, f64p, f64p]
    L.lrh_solve.argtypes = [C.c_int, f64p, f64p, f64p]
    L.lrh_exp.argtypes = [C.c_int, f64p, f64p]
    L.lrh_retract.argtypes = [C.c_int, f64p, f64p, f64p]
    L.lrh_state_machine.argtypes = [C.c_int, f64p, f64p, C.c_double, C.c_int, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
    L.lrh_voxel_coord.argtypes = [C.c_int, f64p, C.c_double, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
    return L


# ---- the checker against the reference's icp_normal ------------------------------------------------------------------------------------
def test_fixture_is_small_and_holds_arrays_only(G):
    assert os.path.getsize(G.FIXTURE) <= 1 << 20
    g = G.load_fixture()
    assert all(v.dtype.kind in "fiuU" for v in g.values())
    assert str(g["backend"]).startswith("reference")
    assert g["src"].dtype == np.float32 and g["tar"].dtype == np.float32 and g["src"].shape[1] == 6 and g["tar"].shape[1] == 6
    assert [int(g[f"{c}_accept"]) for c in G.CASES] == [1, 0, 0, 0]


def test_fixture_inputs_are_what_the_generator_builds(G):
    g, inp = G.load_fixture(), G.inputs()
    assert np.array_equal(g["src"], inp["src"]) and np.array_equal(g["tar"], inp["tar"])
    for c in G.CASES:
        rng_, pose0, eigval = inp["cases"][c]
        assert tuple(g[f"{c}_tar_range"]) == rng_ and np.array_equal(g[f"{c}_pose0"], pose0) and float(g[f"{c}_icp_eigval"]) == eigval


def test_checker_reproduces_the_reference_on_the_golden_cases(G):
    g = G.load_fixture()
    bound = CHECKER_FACTOR * g["checker_vs_ref"]
    assert bound[0] < 1e-12 and bound[1] < 1e-12, bound          # the stored difference is rounding, many orders below the 1e-7 contract
    for c in G.CASES:
        r = R.icp(g["src"], G.case_target(g, c), g[f"{c}_pose0"], icp_eigval=float(g[f"{c}_icp_eigval"]))
        assert int(r["accept"]) == int(g[f"{c}_accept"]), c
        assert np.all(np.isfinite(r["pose"])) and np.all(np.isfinite(K.report_row(r))), c
        if c != "d":
            dt, dr = R.pose_diff(r["pose"], g[f"{c}_pose"])
            print(f"case {c}: checker vs reference {dt:.2e} m {dr:.2e} rad; iterations {r['iterations']}, is_converge {r['is_converge']}, match_num {r['match_num']}")
            assert dt <= bound[0] and dr <= bound[1], (c, dt, dr, bound)
    # what the cases were chosen for
    a = R.icp(g["src"], g["tar"], g["a_pose0"])
    assert a["accept"] and a["iterations"] == 5 and [t["match_num"] for t in a["trace"]] == [1399, 1989, 1989, 1872, 1872]
    dt, dr = R.pose_diff(a["pose"], g["pose_true"])
    assert dt < 2e-3 and dr < 1e-4                               # the registration itself: within the noise of the planes
    b = R.icp(g["src"], g["tar"], g["b_pose0"], icp_eigval=float(g["b_icp_eigval"]))
    assert b["is_converge"] == 1 and not b["accept"] and np.array_equal(b["pose"], a["pose"]) and a["eig"][0] < float(g["b_icp_eigval"])
    c = R.icp(g["src"], g["tar"], g["c_pose0"])
    assert c["iterations"] == 20 and c["is_converge"] == 0 and not c["failed"] and not c["accept"]
    d = R.icp(g["src"], G.case_target(g, "d"), g["d_pose0"])
    assert d["failed"] and 0 < d["match_num"] < 6 and d["iterations"] == 1 and d["is_converge"] == 0 and not d["accept"]


def test_committed_fixture_is_what_the_recipe_generates_from_the_reference(G):
    if not os.path.exists(os.path.join(G.REF_SRC, "loop_refine.hpp")):
        pytest.skip("the reference is not on this machine")
    g = G.load_fixture()
    with tempfile.TemporaryDirectory() as td:
        L, backend = G.load_reference(G.compile_harness(td))
        d = G.build(L, backend)
    assert backend == str(g["backend"])
    keys = [k for k in d if k != "backend"]
    assert sorted(keys) == sorted(k for k in g if k != "backend")
    for k in keys:
        assert np.array_equal(d[k], g[k]), k


# ---- the device's arithmetic, compiled for the host, against the checker ----------------------------------------------------------------
def _random_pairs(rng, n):
    """Source / target rows and poses around the thresholds of both gate vectors: normals a few degrees to tens of degrees apart (some flipped),
    centres from centimetres to metres apart."""
    poses = np.stack([R.pose_of(synth.rodrigues(rng.normal(0, 0.3, 3)), rng.normal(0, 2, 3)) for _ in range(n)])
    src = np.zeros((n, 6), np.float32); tar = np.zeros((n, 6), np.float32)
    src[:, :3] = rng.uniform(-20, 20, (n, 3))
    nv = rng.normal(size=(n, 3)); nv /= np.linalg.norm(nv, axis=1)[:, None]
    src[:, 3:] = nv
    for k in range(n):
        p, nn_ = R.transform(poses[k], src[k:k + 1])
        tn = synth.rodrigues(rng.normal(0, 0.08, 3)) @ nn_[0] * (1.0 if rng.uniform() < 0.5 else -1.0)
        tar[k, :3] = p[0] + rng.normal(0, 1.0, 3) * rng.choice([0.05, 0.3, 1.5])
        tar[k, 3:] = tn
    return poses, src, tar


def test_host_gate_flags_equal_the_checkers(hm):
    rng = np.random.default_rng(3)
    n = 20000
    poses, src, tar = _random_pairs(rng, n)
    for gates in (R.GATES0, R.GATES1, (0.2, 0.2, 0.5, np.inf)):
        g = np.asarray(gates, dtype=np.float64)
        p = np.zeros((n, 3)); nv = np.zeros((n, 3)); ok = np.zeros(n, np.uint8); rr = np.zeros(n)
        hm.lrh_gate(n, poses, src, tar, g, p, nv, ok, rr)
        want_p = np.zeros((n, 3)); want_n = np.zeros((n, 3))
        for k in range(0, n):
            want_p[k], want_n[k] = [x[0] for x in R.transform(poses[k], src[k:k + 1])]
        assert np.array_equal(p, want_p) and np.array_equal(nv, want_n)          # the same roundings, in the same order
        inc, add, rrw, pp, _ = R.gate_quantities(want_p, want_n, tar, np.arange(n))
        want_ok, margin = R.verdict_margin(inc, add, rrw, pp, g)
        assert np.array_equal(rr, rrw)
        assert np.array_equal(ok.astype(bool), want_ok)
        assert 0.2 < want_ok.mean() < 0.8, want_ok.mean()                         # both verdicts are exercised


def test_host_jacobian_sums_solve_and_exp_agree_with_the_checker_to_rounding(hm):
    rng = np.random.default_rng(4)
    n = 500
    poses, src, tar = _random_pairs(rng, n)
    jac = np.zeros((n, 6))
    hm.lrh_jac(n, poses, src, tar, jac)
    for k in range(n):
        want = R.jac_rows(poses[k], src[k:k + 1], tar[k:k + 1, 3:].astype(np.float64))[0]
        assert np.allclose(jac[k], want, rtol=1e-14, atol=1e-14)
    # against the definition: d rr / d(dphi, dt) by central differences of the update R <- R Exp(dphi), t <- t + dt
    for k in range(5):
        def rr_at(dx):
            P = R.retract(poses[k], dx); p, _ = R.transform(P, src[k:k + 1])
            return float(tar[k, 3:].astype(np.float64) @ (p[0] - tar[k, :3].astype(np.float64)))
        num = np.array([(rr_at(1e-6 * np.eye(6)[q]) - rr_at(-1e-6 * np.eye(6)[q])) / 2e-6 for q in range(6)])
        assert np.allclose(num, jac[k], rtol=1e-7, atol=1e-7)                 # [hat(p_s) R^T n_t ; n_t] IS the derivative of rr under that update
    # the 35 sums under one pose
    P0 = poses[0]
    rr = rng.normal(0, 0.05, n)
    acc = np.zeros(35)
    hm.lrh_accumulate(n, P0, src, tar, rr, acc)
    J = R.jac_rows(P0, src, tar[:, 3:].astype(np.float64)); tn = tar[:, 3:].astype(np.float64)
    H = J.T @ J
    assert np.allclose(acc[:21], H[np.triu_indices(6)], rtol=1e-12, atol=1e-9)
    assert np.allclose(acc[21:27], J.T @ rr, rtol=1e-12, atol=1e-9) and np.isclose(acc[27], 0.5 * (rr * rr).sum(), rtol=1e-12)
    assert np.allclose(acc[28:34], (tn.T @ tn)[np.triu_indices(3)], rtol=1e-12, atol=1e-9) and acc[34] == n
    # the solve
    m = 200
    hu = np.zeros((m, 21)); jt = rng.normal(size=(m, 6)); dx = np.zeros((m, 6))
    Hs = []
    for k in range(m):
        A = rng.normal(size=(40, 6)) * rng.uniform(0.1, 10, 6); Hk = A.T @ A
        Hs.append(Hk); hu[k] = Hk[np.triu_indices(6)]
    hm.lrh_solve(m, hu, jt, dx)
    for k in range(m):
        want = np.linalg.solve(Hs[k], -jt[k])
        assert np.allclose(dx[k], want, rtol=1e-9 * np.linalg.cond(Hs[k]) / 1e4 + 1e-10, atol=1e-12), k
    sing = np.zeros((1, 21)); out = np.zeros((1, 6))
    hm.lrh_solve(1, sing, jt[:1].copy(), out)
    assert not np.all(np.isfinite(out))                                          # a singular system yields a step the state machine refuses
    # Exp and the update
    w = np.concatenate([rng.normal(0, 0.5, (50, 3)), rng.normal(0, 1e-6, (20, 3)), np.zeros((1, 3)), [[1e-12, 0, 0]]])
    E = np.zeros((w.shape[0], 9))
    hm.lrh_exp(w.shape[0], np.ascontiguousarray(w), E)
    for k in range(w.shape[0]):
        assert np.allclose(E[k].reshape(3, 3), R.so3_exp(w[k]), rtol=0, atol=4e-16), k
    dxs = rng.normal(0, 0.05, (50, 6)); Ps = poses[:50].copy(); outp = np.zeros((50, 12))
    hm.lrh_retract(50, Ps, dxs, outp)
    for k in range(50):
        assert np.allclose(outp[k], R.retract(Ps[k], dxs[k]), rtol=0, atol=1e-14)


def _run_machine(hm, match, dx, step_tol=1e-3, max_iter=20):
    match = np.ascontiguousarray(match, dtype=np.float64); dx = np.ascontiguousarray(dx, dtype=np.float64).reshape(-1, 6)
    states = np.zeros((len(match), 5), dtype=np.int32)
    n = hm.lrh_state_machine(len(match), match, dx, step_tol, max_iter, states)
    st = dict(iter=0, done=0, is_converge=0, failed=0)
    want = []
    for k in range(len(match)):
        if st["done"]:
            break
        ap = R.advance(st, match[k], dx[k], step_tol, max_iter)
        want.append([st["iter"], st["done"], st["is_converge"], st["failed"], int(ap)])
    assert n == len(want) and np.array_equal(states[:n], np.array(want, dtype=np.int32).reshape(n, 5))
    return states[:n]


def test_host_state_machine_on_scripted_step_norms(hm):
    big, small = [0.01, 0, 0, 0.02, 0, 0], [5e-4, 0, 0, 0, 5e-4, 0]
    rot_only_small = [5e-4, 0, 0, 0, 2e-3, 0]
    # two large steps, a small one (gates tighten), a large one, a small one (stop)
    s = _run_machine(hm, [100] * 8, [big, big, small, big, small, big, big, big])
    assert s.shape[0] == 5 and s[:, 2].tolist() == [0, 0, 1, 1, 1] and s[:, 1].tolist() == [0, 0, 0, 0, 1] and not s[:, 3].any() and s[:, 4].all()
    # small in rotation only is not small
    s = _run_machine(hm, [100] * 3, [rot_only_small] * 3, max_iter=3)
    assert s[:, 2].tolist() == [0, 0, 0] and s[-1, 1] == 1 and s[-1, 0] == 3
    # twenty iterations without a small step: stops at the cap, never converged
    s = _run_machine(hm, [100] * 25, [big] * 25)
    assert s.shape[0] == 20 and s[-1].tolist() == [20, 1, 0, 0, 1] and not s[:-1, 1].any()
    # the first small step at iteration 20: is_converge is set AND the cap stops the pair
    s = _run_machine(hm, [100] * 25, [big] * 19 + [small] * 6)
    assert s.shape[0] == 20 and s[-1].tolist() == [20, 1, 1, 0, 1]
    # fewer than six matches: stopped, failed, is_converge cleared, the step not applied -- also after the gates had tightened
    s = _run_machine(hm, [100, 100, 5, 100], [big, small, big, big])
    assert s.shape[0] == 3 and s[-1].tolist() == [3, 1, 0, 1, 0]
    s = _run_machine(hm, [0], [[np.nan] * 6])
    assert s[-1].tolist() == [1, 1, 0, 1, 0]
    # a step that is not finite
    for bad in (np.nan, np.inf, -np.inf):
        s = _run_machine(hm, [100, 100], [big, [0, bad, 0, 0, 0, 0]])
        assert s[-1].tolist() == [2, 1, 0, 1, 0]


def test_host_voxel_coordinate_is_the_references(hm):
    v = np.array([0.0, -0.0, 0.5, 1.0, -0.5, -1.0, -1.5, -2.0, 2.999999, 3.0, -1e-12, 7.25, -7.25, 1e5, -1e5])
    for vs in (1.0, 0.5, 2.0):
        out = np.zeros(v.size, dtype=np.int64)
        hm.lrh_voxel_coord(v.size, v, vs, out)
        assert np.array_equal(out, R.voxel_coords(v[:, None], vs)[:, 0])
    out = np.zeros(v.size, dtype=np.int64)
    hm.lrh_voxel_coord(v.size, v, 1.0, out)
    assert out[:8].tolist() == [0, 0, 0, 1, -1, -2, -2, -3]          # an exact negative integer lands in the cell below it


# ---- the checker's own invariants ---------------------------------------------------------------------------------------------------------
def test_plane_cloud_order_sign_and_invariance_of_everything_downstream():
    kf = K.keyframes()
    pl = kf["planes"][0]
    rows, co = pl["rows"], pl["coords"]
    key = (co[:, 0] * (1 << 42)) + (co[:, 1] * (1 << 21)) + co[:, 2]
    assert np.all(np.diff(key) > 0)                                               # ascending, lexicographic in (x, y, z), no voxel twice
    lead = rows[np.arange(rows.shape[0]), 3 + np.argmax(np.abs(rows[:, 3:]), axis=1)]
    assert np.all(lead > 0) and np.allclose(np.linalg.norm(rows[:, 3:].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert co.min() < 0 and np.all(pl["lam"][:, 0] < 0.01)
    # row order and normal signs of the target do not change what the ICP computes (beyond the order of its sums)
    src, tar = kf["planes"][2]["rows"], rows
    guess = K.perturbed(K.pair_truth(kf, 2, 0), (1.5, -1.0, 2.0), (0.25, -0.2, 0.15))
    a = R.icp(src, tar, guess)
    rng = np.random.default_rng(1)
    perm = rng.permutation(tar.shape[0]); flip = np.where(rng.uniform(size=tar.shape[0]) < 0.5, -1.0, 1.0).astype(np.float32)
    tar2 = tar[perm].copy(); tar2[:, 3:] *= flip[:, None]
    b = R.icp(src, tar2, guess)
    assert (a["accept"], a["iterations"], a["match_num"]) == (b["accept"], b["iterations"], b["match_num"])
    dt, dr = R.pose_diff(a["pose"], b["pose"])
    assert dt < 1e-12 and dr < 1e-12


def test_loop_drift_and_edge_form():
    rv = K.revisit()
    i, j = 0, rv["cur_index"]
    tr = synth.relative_pose(rv["gt"][i], rv["gt"][j])
    assert hba.loop_drift(rv["gt"][i], rv["gt"][j], tr[9:]) < 1e-12             # the true edge puts the keyframe where it truly is
    d = hba.loop_drift(rv["poses"][i], rv["poses"][j], tr[9:])
    assert abs(d - np.linalg.norm(rv["poses"][j, 9:] - rv["gt"][j, 9:])) < 1e-9   # pose 0 is the truth: the drift is the end-point error


# ---- the conditions that keep the GPU tests honest ------------------------------------------------------------------------------------------
def _assert_decisive(tag, r, ties_allowed=False):
    print(f"{tag}: verdict margin {r['margin']:.3e}, raw per quantity {np.array2string(np.asarray(r['raw']), precision=3)}, ties {r['ties']}" +
          (f", step margin {r['step_margin']:.3e}" if "step_margin" in r else ""))
    assert ties_allowed or r["ties"] == 0, tag
    assert r["margin"] >= DECISIVE, (tag, r["margin"])
    assert np.all(np.asarray(r["raw"]) >= DECISIVE), (tag, r["raw"])
    if "step_margin" in r:
        assert r["step_margin"] >= DECISIVE, (tag, r["step_margin"])


def test_honesty_plane_extraction_inputs():
    kf = K.keyframes()
    rv = K.revisit()
    clouds = dict(kf0=kf["clouds"][0], kf1=kf["clouds"][1], kf2=kf["clouds"][2], kf3=kf["clouds"][3], boundary=K.boundary_cloud(), revisit_cur=rv["cloud_cur"],
                  **{f"revisit_{i}": c for i, c in rv["candidates"]})
    for name, c in clouds.items():
        pl = R.plane_cloud(c)
        lam = pl["lam"]
        clear = float(np.abs(pl["lam_min_all"] - 0.01).min())
        degenerate = float(np.mean((lam[:, 1] - lam[:, 0]) / lam[:, 2] < DEGENERATE_GAP))
        print(f"{name}: {pl['rows'].shape[0]} planes of {pl['lam_min_all'].size} voxels; lambda_min clear of the threshold by {clear:.2e}; near-degenerate share {degenerate:.4f}")
        assert pl["rows"].shape[0] > 30 and clear >= LAMBDA_CLEAR and degenerate <= 0.01, name
    b = R.plane_cloud(K.boundary_cloud())
    assert b["coords"][:, 0].min() == -3 and b["coords"][:, 0].max() == 2                       # the lattice's x = -3.0 .. -2.125 sit in cell -3 ... and x = 3.0 in no plane voxel
    pts = K.boundary_cloud()
    assert np.sum(pts[:, 0] == np.round(pts[:, 0])) > 300 and np.sum((pts[:, 0] == np.round(pts[:, 0])) & (pts[:, 0] < 0)) > 100


def test_honesty_associate_and_golden_inputs(G):
    g = G.load_fixture()
    src, tar = g["src"], g["tar"]
    assert src.shape[0] % 256 and tar.shape[0] % 256 and tar.shape[0] % 1024
    a = R.icp(src, tar, g["a_pose0"])
    for tag, pose in (("initial", g["a_pose0"]), ("converged", a["pose"])):
        for gates in (R.GATES0, R.GATES1):
            _assert_decisive(f"associate {tag} {gates}", R.associate(src, tar, pose, gates))
    for c in G.CASES:
        r = R.icp(src, G.case_target(g, c), g[f"{c}_pose0"], icp_eigval=float(g[f"{c}_icp_eigval"]))
        _assert_decisive(f"golden {c}", r)
        assert r["eig_margin"] > 1.0
    # the one input built to have ties: every target row twice
    d = R.associate(src, K.duplicated_target(tar), g["a_pose0"], R.GATES0)
    assert d["ties"] == src.shape[0] and np.all(d["nn"] < tar.shape[0]) and np.array_equal(d["nn"], R.associate(src, tar, g["a_pose0"], R.GATES0)["nn"])
    _assert_decisive("duplicated target", d, ties_allowed=True)


def test_honesty_large_pair():
    s, t, pose = K.big_pair()
    assert s.shape[0] % 256 and t.shape[0] % 1024
    _assert_decisive("50 000 x 50 000", R.associate(s, t, pose, R.GATES0))


def test_honesty_score_batch():
    kf = K.keyframes()
    st, poses = K.score_batch()
    nt, dt = K.SCORE_THRESHOLDS
    useful = []
    for b, ((s, t), P) in enumerate(zip(st, poses)):
        r = R.associate(kf["planes"][s]["rows"], kf["planes"][t]["rows"], P, (nt, nt, dt, np.inf))
        r["raw"] = r["raw"][:3]                                                   # the score has no point-to-point gate
        _assert_decisive(f"score {b}", r)
        useful.append(int(r["matched"].sum()))
    assert len(set(useful)) > 40 and min(useful) > 100                            # 64 different hypotheses, none trivial


def test_honesty_icp_batch_and_revisit():
    cl = K.icp_clouds()
    st, poses = K.icp_batch()
    res = []
    for b, ((s, t), P) in enumerate(zip(st, poses)):
        r = R.icp(cl[s], cl[t], P)
        _assert_decisive(f"icp {b} ({cl[s].shape[0]} x {cl[t].shape[0]})", r)
        assert r["eig_margin"] > 1e-3
        res.append(r)
    assert len(set(r["iterations"] for r in res)) >= 3 and 0 < sum(r["accept"] for r in res) < 32 and len(set((cl[s].shape[0], cl[t].shape[0]) for s, t in st)) > 10
    rv = K.revisit()
    reg = K.CheckerRegistration()
    out = hba.loop_registration(rv["cloud_cur"], rv["candidates"], rv["guesses"], rv["cur_index"], reg_cls=lambda: reg)
    assert out["tried"].all() and out["accept"].all() and len(out["edges"]) == len(rv["candidates"])
    for b, r in enumerate(reg.last_icp):
        _assert_decisive(f"revisit icp {b}", r)
    for b, r in enumerate(reg.last_score):
        assert r["ties"] == 0 and r["margin"] >= DECISIVE, (b, r)
    for e in out["edges"]:
        tr = synth.relative_pose(rv["gt"][e["i"]], rv["gt"][e["j"]])
        assert np.linalg.norm(tr[9:] - e["tra"]) < 2e-3 and e["j"] == rv["cur_index"] and e["rot"].shape == (3, 3)
