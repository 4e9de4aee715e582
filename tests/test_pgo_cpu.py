"""Pose-graph optimiser, CPU side: the checker (tests/_pgo_ref.py) against finite differences and its own invariants, the device's
per-factor arithmetic (csrc/vxba_pgo_math.hpp) compiled for the host against the checker, and the condition that keeps the GPU tests
(tests/test_gpu_pgo.py) honest: on every graph they use, the model of the device's CG finishes inside the default cap and the checker
stops at the optimum."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _pgo_ref as P
from voxel_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")

# The graphs of the GPU tests (name -> synth.pose_graph arguments): the five rows of the issue's table.
GRAPHS = {
    "hba105": dict(K=105, hba=True),
    "hba500": dict(K=500, hba=True),
    "hba1000": dict(K=1000, hba=True, seed=synth.MASTER_SEED + 7001),    # (the default seed's third cost change is 1.0e-6: on the stopping threshold itself)
    "loop200": dict(K=200, loops=((0, 199), (5, 195), (10, 190))),
    "loop500": dict(K=500, loops=((0, 499), (5, 495), (10, 490))),
}
# Settings of the runs that are held against the checker: the library's defaults (stop on a relative cost change below 1e-6) with room in max_iter.
RUN = dict(max_iter=20, rel_cost_tol=1e-6)
GN_STEP_AT_OPTIMUM = 1e-5     # m / rad: a full Gauss-Newton step from where the checker stopped moves no pose by more (a tenth of the 1e-4 contract)
DECISIVE = 1e-11              # every accept / reject decision rests on a relative cost change above this; the f64 sums of ~1e4 costs scatter by ~1e-15


def make_graph(d):
    return P.Graph(d.poses.shape[0]).add_edges(d.edge_ij, d.edge_data).add_priors(d.prior_node, d.prior_pose, d.prior_v6)


def gn_step(g, X):
    D, grad, B, _ = g.linearize(X)
    return float(np.abs(P.dense_solve(g, D, grad, B, 0.0)).max())


@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "pgo_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libpgo_hostcheck.so")
    hdr = os.path.join(HERE, "..", "voxel-slam_amd", "csrc", "vxba_pgo_math.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.pgoh_between.argtypes = [C.c_int] + [f64p] * 8
    L.pgoh_between_residual.argtypes = [C.c_int] + [f64p] * 4
    L.pgoh_prior.argtypes = [C.c_int] + [f64p] * 4
    L.pgoh_retract.argtypes = [C.c_int] + [f64p] * 3
    L.pgoh_inv6.argtypes = [C.c_int, f64p]
    return L


def _random_factors(rng, angles):
    """One between factor per residual angle: random poses, a measurement that leaves exactly that rotation residual and ~0.3 m of translation."""
    n = len(angles)
    Ri = np.array([synth.rodrigues(rng.normal(size=3)) for _ in range(n)]); Rj = np.array([synth.rodrigues(rng.normal(size=3)) for _ in range(n)])
    pi, pj = rng.normal(size=(n, 3)) * 3, rng.normal(size=(n, 3)) * 3
    Z = np.zeros((n, 12))
    for k, a in enumerate(angles):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        Zr = Ri[k].T @ Rj[k] @ synth.rodrigues(-a * ax)              # Zr^T R_i^T R_j = Exp(a ax)
        Z[k, :9] = Zr.reshape(9)
        Z[k, 9:] = Ri[k].T @ (pj[k] - pi[k]) + rng.normal(size=3) * 0.3
    return synth.pack_poses(Ri, pi), synth.pack_poses(Rj, pj), Z


ANGLES = [1e-9, 1e-8, 1e-7, 9e-7, 1.1e-6, 1e-5, 1e-4, 9e-4, 1e-3, 1.1e-3, 9.9e-3, 1.01e-2, 0.1, 0.5, 1.0, 2.0, 2.5]


def test_log_is_accurate_at_converged_residual_angles():
    """Log(Exp(w)) = w to 1e-12 relative from 1e-9 to 2.5 rad -- where the reference's acos form is 1.7e-7 off at 1e-3 rad."""
    rng = np.random.default_rng(11)
    for a in ANGLES:
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        w = P.so3_log(synth.rodrigues(a * ax)[None])[0]
        # the matrix itself holds the angle to 1e-16 absolute: relative 1e-16 / a
        assert np.linalg.norm(w - a * ax) <= a * (1e-12 + 4e-16 / a), (a, w - a * ax)


def test_checker_jacobians_match_central_differences():
    rng = np.random.default_rng(12)
    Pi, Pj, Z = _random_factors(rng, ANGLES * 3)
    e0, Ji, Jj = P.between_lin(Pi, Pj, Z)
    assert np.allclose(np.linalg.norm(e0[:, :3], axis=1), ANGLES * 3, rtol=1e-6, atol=1e-15)
    h = 1e-6
    for k in range(12):
        d = np.zeros((len(Pi), 6)); d[:, k % 6] = h
        if k < 6:
            ep = P.between_lin(P.retract(Pi, d), Pj, Z)[0]; em = P.between_lin(P.retract(Pi, -d), Pj, Z)[0]
            J = Ji[:, :, k]
        else:
            ep = P.between_lin(Pi, P.retract(Pj, d), Z)[0]; em = P.between_lin(Pi, P.retract(Pj, -d), Z)[0]
            J = Jj[:, :, k - 6]
        assert np.abs((ep - em) / (2 * h) - J).max() < 2e-8, k
    e0, J = P.prior_lin(Pi, Z)
    for k in range(6):
        d = np.zeros((len(Pi), 6)); d[:, k] = h
        fd = (P.prior_lin(P.retract(Pi, d), Z)[0] - P.prior_lin(P.retract(Pi, -d), Z)[0]) / (2 * h)
        assert np.abs(fd - J[:, :, k]).max() < 2e-8, k


def test_device_arithmetic_on_host_matches_checker(hm):
    """e, J_i, J_j and B = J_i^T W J_j of vxba_pgo_math.hpp per factor, to 1e-9 relative, residual angles around 1e-6 and 1e-3 rad included."""
    rng = np.random.default_rng(13)
    Pi, Pj, Z = _random_factors(rng, ANGLES * 4)
    n = len(Pi)
    w = 10.0 ** rng.uniform(1, 6, size=(n, 6))
    e = np.zeros((n, 6)); Ji = np.zeros((n, 36)); Jj = np.zeros((n, 36)); B = np.zeros((n, 36))
    hm.pgoh_between(n, Pi, Pj, Z, w, e, Ji, Jj, B)
    er, Jir, Jjr = P.between_lin(Pi, Pj, Z)
    Br = np.einsum("fka,fkb->fab", Jir, w[:, :, None] * Jjr)
    for got, ref in ((e, er), (Ji.reshape(n, 6, 6), Jir), (Jj.reshape(n, 6, 6), Jjr), (B.reshape(n, 6, 6), Br)):
        for f in range(n):
            assert np.allclose(got[f], ref[f], rtol=1e-9, atol=1e-9 * np.abs(ref[f]).max()), (f, np.abs(got[f] - ref[f]).max())
    # the rotation residual entry by entry, down to 1e-9 rad: the product Zr^T R_i^T R_j carries a few ulp of 1 whatever its angle, and the two sides
    # add its nine terms in different orders
    assert np.allclose(e[:, :3], er[:, :3], rtol=1e-9, atol=2e-15)
    e2 = np.zeros((n, 6))
    hm.pgoh_between_residual(n, Pi, Pj, Z, e2)
    assert np.array_equal(e2, e)                                      # the cost kernel's residual is the linearisation's
    ep = np.zeros((n, 6)); Jp = np.zeros((n, 36))
    hm.pgoh_prior(n, Pi, Z, ep, Jp)
    epr, Jpr = P.prior_lin(Pi, Z)
    assert np.allclose(ep, epr, rtol=1e-9, atol=1e-12) and np.allclose(Jp.reshape(n, 6, 6), Jpr, rtol=1e-9, atol=1e-12)
    # retraction and the preconditioner's 6 x 6 inverse
    dx = rng.normal(size=(n, 6)) * np.array(ANGLES * 4)[:, None]
    out = np.zeros((n, 12))
    hm.pgoh_retract(n, Pi, dx, out)
    assert np.allclose(out, P.retract(Pi, dx), rtol=0, atol=1e-14)
    A = np.array([(lambda M: M @ M.T + 1e-3 * np.eye(6))(rng.normal(size=(6, 6))) * 10.0 ** rng.uniform(-3, 6) for _ in range(50)])
    Ai = A.copy().reshape(50, 36)
    hm.pgoh_inv6(50, Ai)
    for k in range(50):
        assert np.allclose(Ai[k].reshape(6, 6) @ A[k], np.eye(6), atol=1e-9 * np.linalg.cond(A[k]) ** 0.5)


def test_optimum_moves_with_the_gauge():
    """Every pose and the prior moved by one rigid motion T (X -> T X): the residuals are unchanged, and the optimum moves with it."""
    d = synth.random_pose_graph(K=20, extra_edges=30)
    T_R, T_p = synth.rodrigues(np.array([0.4, -0.7, 1.1])), np.array([5.0, -3.0, 2.0])

    def move(Pk):
        R, p = P.unpack(Pk)
        return P.pack(T_R @ R, p @ T_R.T + T_p)

    g0 = make_graph(d)
    g1 = P.Graph(20).add_edges(d.edge_ij, d.edge_data).add_priors(d.prior_node, move(d.prior_pose), d.prior_v6)
    assert np.allclose(g0.residuals(d.poses), g1.residuals(move(d.poses)), rtol=0, atol=1e-12)
    a, b = P.dense_lm(g0, d.poses, **RUN), P.dense_lm(g1, move(d.poses), **RUN)
    assert [r["accepted"] for r in a["report"]] == [r["accepted"] for r in b["report"]]
    et, er = synth.pose_errors(move(a["poses"]), b["poses"])
    assert et < 1e-9 and er < 1e-9, (et, er)
    assert gn_step(g0, a["poses"]) < GN_STEP_AT_OPTIMUM


def test_dense_hessian_is_the_operator_of_the_cg_model():
    d = synth.random_pose_graph(K=12, extra_edges=10)
    g = make_graph(d)
    D, grad, B, _ = g.linearize(d.poses)
    m = P.CgModel(g)
    x = np.random.default_rng(3).normal(size=(12, 6))
    H = g.dense_hessian(D, B)
    assert np.allclose(m.apply(D, B, 0.0, x).reshape(-1), H @ x.reshape(-1), rtol=1e-12, atol=1e-9 * np.abs(H).max())
    assert np.isclose(m.block_sum(x), x.sum(), rtol=1e-13)
    dx, r, info = m.solve(D, grad, B, 1e-6, tol=1e-10)
    assert not info["cg_capped"] and np.allclose(dx, P.dense_solve(g, D, grad, B, 1e-6), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("name", list(GRAPHS) + ["random20"])
def test_gpu_test_graphs_converge_inside_the_default_cg_cap(name):
    """The condition that keeps the GPU tests from hiding a failure: with the DEFAULT cap (2 x unknowns) and tolerance the model of the device's CG
    ends every solve by its tolerance, the LM loop built on it takes the dense loop's accept / reject decisions, and where the dense loop
    stops a full Gauss-Newton step moves no pose by more than GN_STEP_AT_OPTIMUM."""
    d = synth.random_pose_graph(K=20, extra_edges=30) if name == "random20" else synth.pose_graph(**GRAPHS[name])
    g = make_graph(d)
    dense = P.dense_lm(g, d.poses, **RUN)
    assert len(dense["report"]) < RUN["max_iter"]
    gs = gn_step(g, dense["poses"])
    rel = [abs(r["cost_before"] - r["cost_after"]) / r["cost_before"] for r in dense["report"]]
    print(name, "Gauss-Newton step left at the checker's stop %.2e" % gs, "relative cost changes", ["%.1e" % x for x in rel])
    assert gs < GN_STEP_AT_OPTIMUM
    assert min(rel) > DECISIVE           # no decision of this run is taken by rounding: the GPU's sequence can be held to the checker's
    cg = P.dense_lm(g, d.poses, solver=P.CgModel(g).solver(), **RUN)
    print(name, "factors", g.F, "CG iterations per outer", [r["cg_iterations"] for r in cg["report"]], "accepted", [r["accepted"] for r in cg["report"]])
    assert not any(r["cg_capped"] for r in cg["report"])
    assert max(r["cg_iterations"] for r in cg["report"]) < max(200, 12 * g.K)
    assert [r["accepted"] for r in cg["report"]] == [r["accepted"] for r in dense["report"]]
    et, er = synth.pose_errors(cg["poses"], dense["poses"])
    assert et < 1e-6 and er < 1e-6, (et, er)
