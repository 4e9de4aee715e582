"""The sweeps' exact reference, its cases and its criteria, checked without a GPU (tests/_sweep_ref.py, tests/_sweep_cases.py).

  * the reference against mathematics: hessian_exact from the exact cache is the gradient and the Hessian of sum coe lambda_0, by central
    differences in mpmath;
  * the reference against the oracle, and the calibration: the CPU oracle meets every criterion with the constants K_ORACLE_* recorded in
    tests/_sweep_cases.py (so they cannot drift), and how far its eigenvalues are from the exact ones stays on record;
  * the host build of the kernels' per-entry arithmetic (tests/test_device_math_on_host.py's harness) meets the same criteria: a wrong
    bound shows here, before a GPU is involved -- and the one that did (the rotation blocks on the expanded magnitude alone) stays on record;
  * degraded sweeps are rejected, every one of them and each by the criterion it is meant for, while the older max-norm comparison at
    1e-10 accepts two of them;
  * the cases are what they claim to be.

Central differences: with f = sum coe lambda_0 along x (+) h e (rotations R Exp(h e), translations p + h e), [f(h) - f(-h)] / 2h and the
four-point second difference are off by h^2 / 6 times a fourth (third) derivative.  Every derivative of lambda_0 costs a factor of at most
(lever arm) / (eigenvalue gap) ~ 10 m / 0.05, so f'''' / f'' <= 1e5 and the truncation at h = 1e-20 is at most 1e-35 of the element;
rounding (400 bits: 1e-120 / h^2) is nothing.  Asserted: 1e-30 M element by element, the issue's figure (measured: 3e-42 M for H, 3e-41 M
for J -- M is two to three orders above the element), twelve orders below what a wrong term would give.

One expectation of the issue does not hold and is asserted as it is: dropping ONE pair record of the 513-record block is NOT accepted by
the max-norm comparison at 1e-10 (it moves that block by 1 / 513 of itself, 4e-3 of the largest entry); no single record of these windows
is that small.  Two variants are accepted by it and rejected element by element: one entry's rows rounded to f32 among 513 records
(max-norm 3.6e-11), and the block (1, 9), which is one pair record, kept in f32."""
import ctypes as C

import numpy as np
import pytest
import mpmath as mp
from mpmath import mpf

from tests import _oracle as O
from tests import _sweep_cases as S
from tests import _sweep_ref as R
from tests.test_device_math_on_host import hm  # noqa: F401  (the fixture: both host builds of csrc/vxba_math.hpp)
from voxel_slam_amd import synth


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def test_cases_are_what_they_claim():
    c = S.case("wide11")
    runs = S.run_lengths(c)
    assert {runs[(i, i)] for i in range(11) if (i, i) in runs} == {1025, 513, 512, 511, 65, 64, 63, 1, 2}
    assert (8, 8) not in runs and not any(8 in k for k in runs)                               # the empty frame
    assert set(runs.values()) >= {1, 2, 63, 64, 65, 511, 512, 513, 1025}
    assert runs[(1, 9)] == 1 and runs[(0, 9)] == 2 and runs[(9, 10)] == 2                    # a frame pair with one shared voxel
    assert all(runs[(i, j)] == min(S.WIDE11_N[i], S.WIDE11_N[j]) for (i, j) in runs if j < 9)
    tasks = lambda n: -(-n // S.WIDE_TASK_RECORDS)
    assert (tasks(511), tasks(512), tasks(513), tasks(1025)) == (1, 1, 2, 3)
    assert any(h < 512 < e and (h > 0 or e < c.V) for h, e in c.ranges[1:]) and any(h == 512 for h, e in c.ranges[1:])
    c = S.case("wide12")
    assert c.V == 65 and set(S.run_lengths(c).values()) == {65}
    c = S.case("wide128")
    obs = c.clusters[:, :, 9] != 0
    assert all(set(np.nonzero(obs[a])[0]) == {a, (7 * a + 3) % 128, 127} for a in range(c.V)) and obs[:, 127].all()
    assert S.reference("wide128")["M_H"].astype(bool).mean() < 0.02                            # almost all structural zeros
    for name in S.NARROW:
        c = S.case(name)
        a = np.arange(c.V)
        obs = c.clusters[:, :, 9] != 0
        H1 = (c.W + 1) // 2
        assert len(set(a % 5)) == min(c.V, 5)                                                  # (V = 1: the one voxel is of class 0)
        if c.W >= 3:
            assert not obs[:, c.W - 1].any()
        if c.V >= 7:
            assert not obs[a % 5 == 1][:, :H1].any() and not obs[a % 5 == 2][:, H1:].any() and not obs[a % 5 == 4][:, 1::2].any()
            assert obs[a % 5 == 0][:, : max(1, c.W - 1 if c.W >= 3 else c.W)].all()
            assert (c.fix[(a % 5 == 2) | (a % 5 == 3), 9] == 0).all() and (c.fix[a % 5 == 0, 9] > 0).all()
        stale = ~obs & (a % 3 == 0)[:, None]
        assert np.all(c.clusters[stale][:, :9] != 0) or not stale.any()
        assert stale.any() == (c.W >= 3 or c.V >= 7)                                            # stale moments beside N == 0 (W <= 2 at V = 1: the one voxel sees every frame)
    c = S.case("w3_v515")
    assert c.ranges == ((0, 515), (3, 511))
    far = S.case("far")
    assert np.abs(far.poses[:, 9:]).max() > 700 and np.abs(far.fix[far.fix[:, 9] > 0, 6:9] / far.fix[far.fix[:, 9] > 0, 9:]).max() > 700
    # the compressed rows with one entry that has no points: same window, one more pair record per block of that frame
    w = S.case("wide11")
    rp, fr, ent = S.csr_with_zero_entry(w.clusters, 700, 3)
    assert ent.shape[0] == (w.clusters[:, :, 9] != 0).sum() + 1 and (ent[:, 9] == 0).sum() == 1 and np.any(ent[ent[:, 9] == 0][0, :9] != 0)


def test_first_lm_step_of_the_fused_windows_is_accepted_by_the_oracle():
    for W, V in S.FUSED + ((10, 515),):
        sc, cl, fix, coe = S._scene(W, V)
        f = O.Oracle(W); f.push_voxels(cl, fix, coe); f.evaluate_only_residual(sc.poses_init)
        out = f.damping_iter(sc.poses_init, max_iter=1)
        assert out["trace"].shape[0] == 1 and out["trace"][0, 6] == 1, (W, V, out["trace"])


# ---- the reference against mathematics -------------------------------------------------------------------------------------------------
def _exp(phi):
    th = mp.sqrt(sum(x * x for x in phi))
    K = R._hat(phi)
    if th == 0:
        return [[mpf(int(r == c)) for c in range(3)] for r in range(3)]
    K2 = R._matmul(K, K)
    a, b = mp.sin(th) / th, (1 - mp.cos(th)) / (th * th)
    return [[mpf(int(r == c)) + a * K[r][c] + b * K2[r][c] for c in range(3)] for r in range(3)]


def test_reference_is_the_gradient_and_hessian_of_the_smallest_eigenvalue():
    c = S.case("w3_v7")
    with mp.workprec(400):
        ev, Uv, m = R.exact_cache(c.clusters, c.fix, c.poses, as_float=False)
        ref = R.hessian_exact(c.clusters, c.coe, c.poses, ev, Uv, m, raw=True)
        h = mpf(10) ** -20
        n = 6 * c.W
        Hfd = np.full((n, n), mpf(0), dtype=object); Jfd = np.full(n, mpf(0), dtype=object)
        base = [R._rot(c.poses[i]) for i in range(c.W)]
        for a in range(c.V):
            obs = [i for i in range(c.W) if c.clusters[a, i, 9] != 0]
            var = [6 * i + k for i in obs for k in range(6)]
            cls = {i: R._vec(c.clusters[a, i]) for i in obs}
            fixa = R._vec(c.fix[a]); ca = mpf(float(c.coe[a]))

            def f(d):
                acc = list(fixa)
                for i in obs:
                    Rm, p = base[i]
                    di = [d.get(6 * i + k, mpf(0)) for k in range(6)]
                    if any(di):
                        Rm = R._matmul(Rm, _exp(di[:3])); p = [p[k] + di[3 + k] for k in range(3)]
                    acc = [x + y for x, y in zip(acc, R.transform_exact(cls[i], Rm, p))]
                return ca * min(mp.eigsy(mp.matrix(R.covariance_exact(acc)[0]), eigvals_only=True))

            f0 = f({})
            for x in var:
                fp, fm = f({x: h}), f({x: -h})
                Jfd[x] += (fp - fm) / (2 * h)
                Hfd[x, x] += (fp - 2 * f0 + fm) / (h * h)
            for ix, x in enumerate(var):
                for y in var[ix + 1:]:
                    d2 = (f({x: h, y: h}) - f({x: h, y: -h}) - f({x: -h, y: h}) + f({x: -h, y: -h})) / (4 * h * h)
                    Hfd[x, y] += d2; Hfd[y, x] += d2
        eH = np.array([[float(abs(Hfd[r, q] - ref["H_mp"][r, q])) for q in range(n)] for r in range(n)])
        eJ = np.array([float(abs(Jfd[q] - ref["J_mp"][q])) for q in range(n)])
    live = ref["M_H"] > 0
    print(f"central differences vs hessian_exact: H {np.max(eH[live] / ref['M_H'][live]):.2e} M   J {np.max(eJ[ref['M_J'] > 0] / ref['M_J'][ref['M_J'] > 0]):.2e} M")
    assert np.all(eH <= 1e-30 * ref["M_H"]) and np.all(eJ <= 1e-30 * ref["M_J"])
    assert live.sum() == 4 * 36 and not eH[~live].any()


# ---- the oracle: the reference against it, and the calibration ------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.CASES)
def test_oracle_meets_every_criterion_with_its_measured_constants(name):
    c = S.case(name)
    k = S.oracle_constants(name)
    print(f"{name}: oracle H {k[0]:.4g} J {k[1]:.4g} merged {k[2]:.4g} eig {k[3]:.4g} {k[4]:.4g} {k[5]:.4g} {k[6]:.4g}  its own cache: residual {k[7]:.4g} eigenvalues {k[8]:.4g} (u s)")
    Ks = (S.K_ORACLE_H, S.K_ORACLE_J, S.K_ORACLE_M, S.K_ORACLE_E_RES, S.K_ORACLE_E_LAM, S.K_ORACLE_E_ORTH, S.K_ORACLE_E_ORTH1, S.K_ORACLE_CACHE_RES, S.K_ORACLE_CACHE_LAM)
    assert np.all(k <= np.array(Ks)), (k, Ks)
    if name != "wide128":          # the distance of the oracle's eigenvalues from the exact ones of the row it returns (K_ORACLE_CACHE_*)
        assert k[7] <= 2.2 and k[8] <= 2.5
    # and through the checks themselves, as the device tests call them
    f = S.oracle_factor(name)
    for head, end in c.ranges:
        H, J, r = f.acc_evaluate2(c.poses, head, end)
        S.check_hessian(H, J, r, S.reference(name, head, end), end - head, c_h=S.C_H, bitwise_symmetric=False)
    g = S.oracle_factor(name, seeded=False)
    r = g.evaluate_only_residual(c.poses2)
    ev, Uv, m = g.read_cache()
    S.check_merged(m, name, second=True)
    S.check_eig(m, *S.ql_on_rows(m))
    S.check_scalar(r, c.coe, ev[:, 0])


# ---- the kernels' per-entry arithmetic, compiled for the host -------------------------------------------------------------------------
def _host_k3(hm, fn, c, cache):
    n = 6 * c.W
    H = np.zeros((n, n)); J = np.zeros(n); rr = C.c_double(0)
    fn(c.V, c.W, c.clusters, c.coe, *cache, c.poses, H, J, C.byref(rr))
    return H.T.copy(), J, rr.value


@pytest.mark.parametrize("name", S.CASES)
def test_host_build_of_the_kernels_arithmetic_meets_the_criteria(hm, name):
    c = S.case(name)
    cache = S.seeded_cache(name)
    ref = S.reference(name)
    for what, fn in (("rows", hm.vxmh_k3), ("spare columns", hm.vxmh_k3_spare)):
        H, J, r = _host_k3(hm, fn, c, cache)
        if what == "spare columns":      # the narrow kernel's D_rt / D_tt come out of a product and are mirrored by k3_finalize on the device
            H = np.triu(H) + np.triu(H, 1).T
        S.check_hessian(H, J, r, ref, c.V, label=f"{name} host {what}")
    ev = np.zeros((c.V, 3)); Uv = np.zeros((c.V, 9)); m = np.zeros((c.V, 10)); r = C.c_double(0)
    hm.vxmh_k2(c.V, c.W, c.clusters, c.fix, c.coe, c.poses, ev, Uv, m, C.byref(r))
    S.check_merged(m, name, label=f"{name} host")
    S.check_eig(m, ev, Uv, label=f"{name} host")
    S.check_scalar(r.value, c.coe, ev[:, 0])


def test_closed_form_of_the_rotation_block_needs_its_own_magnitude(hm):
    """Why the rotation-rotation part of the diagonal blocks carries D_RR M_RR (tests/_sweep_cases.py): on M_H alone a correct evaluation of
    the closed form exceeds 4 K_ORACLE_H there -- and nowhere else."""
    for name, where in (("w10_v1", (20, 20)), ("wide128", (84, 84))):
        c = S.case(name)
        ref = S.reference(name)
        H, J, _ = _host_k3(hm, hm.vxmh_k3, c, S.seeded_cache(name))
        kH, _ = S.hessian_ratios(H, J, ref)
        assert np.unravel_index(np.argmax(kH), kH.shape) == where and S.C_H < kH.max() < 1.0 and ref["M_RR"][where] > 0, (name, kH.max())
        assert kH[ref["M_RR"] == 0].max() <= S.C_H


# ---- degraded sweeps ------------------------------------------------------------------------------------------------------------------
def _rows(c, cache, a):
    """The rank-3 rows of voxel a in float64: {frame: (3, 6) rows scaled so that H_a = -rows^T rows + D}, and z, N."""
    ev, Uv, m = cache
    Rs, ps = synth.unpack_poses(c.poses)
    hat = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    lam = ev[a]; Um = Uv[a].reshape(3, 3).T; u = Um[:, 0]; N = m[a, 9]; vbar = m[a, 6:9] / N
    out, zs = {}, {}
    for i in range(c.W):
        q = c.clusters[a, i]
        if q[9] == 0:
            continue
        P = np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]]); v = q[6:9]
        Rm, p = Rs[i], ps[i]
        r = Rm.T @ u; t = p - vbar; ut = u @ t
        c1 = hat(P @ r) + hat(v) * ut; c2 = Rm @ v + q[9] * t
        Ai = np.hstack([(Rm @ P + np.outer(t, v)) @ hat(r) - Rm @ c1, np.outer(c2, u) + (c2 @ u) * np.eye(3)]) / N
        z = np.concatenate([np.cross(v, r), q[9] * u])
        sc = np.sqrt(c.coe[a])
        out[i] = np.stack([sc * np.sqrt(2 / (lam[1] - lam[0])) * Um[:, 1] @ Ai, sc * np.sqrt(2 / (lam[2] - lam[0])) * Um[:, 2] @ Ai, sc * np.sqrt(2) / N * z])
        zs[i] = z
    return out, zs, N


def _blk(i, j):
    return np.ix_(range(6 * i, 6 * i + 6), range(6 * j, 6 * j + 6))


@pytest.fixture(scope="module")
def wide11_oracle():
    c = S.case("wide11")
    f = S.oracle_factor("wide11")
    H, J, r = f.acc_evaluate2(c.poses)
    return c, f, np.triu(H) + np.triu(H, 1).T, J, r          # (the oracle's diagonal blocks are symmetric to round-off only: mirrored here)


def _degraded(kind, c, f, H, J, r):
    """(H, J, r, reference, voxels) of one degraded variant of the oracle's output on wide11."""
    H, J = H.copy(), J.copy()
    ref, nv = S.reference("wide11"), c.V
    cache = S.seeded_cache("wide11")
    def one(a):          # one voxel's share, its diagonal blocks mirrored like the fixture's
        Ha, Ja, ra = f.acc_evaluate2(c.poses, a, a + 1)
        return np.triu(Ha) + np.triu(Ha, 1).T, Ja, ra
    if kind == "one pair record of the 513-record block":
        assert S.run_lengths(c)[(1, 1)] == 513
        H[_blk(1, 1)] -= one(100)[0][_blk(1, 1)]
    elif kind == "last task partial of the 1025-record block":           # records [1024, 1025) of block (0, 0): voxel 1024, with its gradient piece
        Ha, Ja, _ = one(1024)
        H[_blk(0, 0)] -= Ha[_blk(0, 0)]; J[:6] -= Ja[:6]
    elif kind == "one voxel":
        Ha, Ja, ra = one(300)
        H -= Ha; J -= Ja; r -= ra
    elif kind == "a block without its mirror image":
        H[_blk(2, 1)] = 0.0
    elif kind == "one off-diagonal block transposed":
        B = H[_blk(1, 2)].copy()
        H[_blk(1, 2)] = B.T; H[_blk(2, 1)] = B
    elif kind == "one entry's rows in f32":
        rows, _, _ = _rows(c, cache, 100)
        r32 = rows[1].astype(np.float32).astype(np.float64)
        for j, rj in rows.items():
            d = -(r32.T @ (r32 if j == 1 else rj)) + rows[1].T @ rj
            H[_blk(1, j)] += d
            if j != 1:
                H[_blk(j, 1)] += d.T
    elif kind == "N of the frame in one 2 / N^2 term":
        _, zs, N = _rows(c, cache, 100)
        d = -c.coe[100] * (2 / c.clusters[100, 1, 9] ** 2 - 2 / N ** 2) * np.outer(zs[1], zs[2])
        H[_blk(1, 2)] += d; H[_blk(2, 1)] += d.T
    elif kind == "a voxel outside the sub-range":
        head, end = c.ranges[1]
        H, J, r = f.acc_evaluate2(c.poses, head, end)
        Ha, Ja, ra = one(700)
        H, J, ref, nv = H + Ha, J + Ja, S.reference("wide11", head, end), end - head
        H = np.triu(H) + np.triu(H, 1).T
    elif kind == "the one-record block (1, 9) in f32":                 # a block that is ONE pair record (voxel 0), kept in f32
        assert S.run_lengths(c)[(1, 9)] == 1
        B = H[_blk(1, 9)].astype(np.float32).astype(np.float64)
        H[_blk(1, 9)] = B; H[_blk(9, 1)] = B.T
    elif kind == "1e-300 where nothing reaches":
        z = np.argwhere(ref["M_H"] == 0)[7]
        H[z[0], z[1]] = H[z[1], z[0]] = 1e-300
    else:
        raise KeyError(kind)
    return H, J, r, ref, nv


DEGRADED = ("one pair record of the 513-record block", "last task partial of the 1025-record block", "one voxel", "a block without its mirror image",
            "one off-diagonal block transposed", "one entry's rows in f32", "the one-record block (1, 9) in f32", "N of the frame in one 2 / N^2 term",
            "a voxel outside the sub-range", "1e-300 where nothing reaches")
STRUCTURAL = {"a block without its mirror image": "differs from its transpose", "1e-300 where nothing reaches": "not exact zeros"}


@pytest.mark.parametrize("kind", DEGRADED)
def test_degraded_sweeps_are_rejected(wide11_oracle, kind):
    """Each by the criterion it is meant for: the two structural ones by the structure check, every other one by the HESSIAN bound itself
    (several also move J or r; those checks come later in check_hessian and are not what rejects them)."""
    c, f, H0, J0, r0 = wide11_oracle
    S.check_hessian(H0, J0, r0, S.reference("wide11"), c.V)                      # the undegraded output passes
    H, J, r, ref, nv = _degraded(kind, c, f, H0, J0, r0)
    kH, _ = S.hessian_ratios(H, J, ref)
    frac = R.err_units(H, ref["H"], ref["H_lo"], S.hessian_bound_units(ref, nv))
    print(f"{kind}: largest |err| {kH.max():.3g} u M, {frac.max():.3g} of its bound   max-norm relerr {S.relerr(H, ref['H']):.2e}")
    if kind in STRUCTURAL:
        with pytest.raises(AssertionError, match=STRUCTURAL[kind]):
            S.check_hessian(H, J, r, ref, nv)
    else:
        assert frac.max() > 1.0
        with pytest.raises(AssertionError, match="H: .err. is"):
            S.check_hessian(H, J, r, ref, nv)


def test_max_norm_comparison_accepts_what_the_elementwise_one_rejects(wide11_oracle):
    """The gap this suite closes: relerr(H, H_ref) < 1e-10, the strictest comparison of a Hessian the older tests make, passes a sweep that
    rounded one entry's rank-3 rows to f32, and one that kept a whole one-record block in f32.  It does not pass the dropped pair record
    (module docstring)."""
    c, f, H0, J0, r0 = wide11_oracle
    for kind in ("one entry's rows in f32", "the one-record block (1, 9) in f32"):
        H, J, r, ref, nv = _degraded(kind, c, f, H0, J0, r0)
        assert S.relerr(H, ref["H"]) < 1e-10 and S.relerr(J, ref["J"]) < 1e-10, kind
    H, J, r, ref, nv = _degraded("one pair record of the 513-record block", c, f, H0, J0, r0)
    assert S.relerr(H, ref["H"]) > 1e-5
