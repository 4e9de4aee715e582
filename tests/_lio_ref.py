"""Exact reference of the odometry's point-to-plane update (csrc/vxba_lio.hip; voxelslam.cpp:855-958, voxel_map.hpp:1335-1392), in the
manner of tests/_sweep_ref.py: mpmath at 200 bits.  Test infrastructure only.

One statement of the arithmetic serves twice.  `point_terms` is written over nested lists of numpy arrays in the reference's order of
operations (voxelslam.cpp:873-919 for var_world, wld, R_inv, the Jacobian and the 34 terms; voxel_map.hpp:1340-1365 for sigma); with float64
arrays it is the vectorised float64 restatement, with object arrays of mpf it is the exact reference, and with the inputs' absolute values
and every subtraction turned into an addition it gives the magnitudes (the sum of the absolute values of the products a quantity is made of).

What stays as the code has it, because it is typed or integer work and not arithmetic to be judged: which leaf a point is tested against
(`MapIndex.lookup`: the float-typed voxel index, the descent, and `cache_leaf` for "the previous leaf if still inside its box, else a new
lookup"), and the float-typed gate quantities (`gates`).  tests/test_lio_cpu.py pins the leaf of every matched point to the oracle's.

The 34 sums: 0..20 HTH upper triangle row by row, 21..26 HTz, 27..32 nnt upper triangle, 33 the count (NSUM of csrc/vxba_lio_ctl.hpp).

The EKF step (`ekf_exact`) replays voxelslam.cpp:921-957 from given sweeps: S = cov^-1 + HTH, K = S^-1, G = K[:, :6] HTH,
vec = x_prop [-] x_curr, solution = K[:, :6] HTz + vec - G vec[:6], x_curr [+]= solution, the convergence / rematch schedule, (I - G) cov and
the smallest eigenvalue of nnt.  Log and Exp are the reference's own piecewise definitions (tools.hpp:51-91: theta = 0 above tr = 3 - 1e-6,
the factor 0.5 below theta = 0.001, the identity below |w| = 1e-11), evaluated exactly; they are definitions, not approximations to be judged."""
import math

import numpy as np
import mpmath as mp
from mpmath import mpf

from tests._sweep_ref import PREC, U64, _hp, err_units, split_hi_lo  # noqa: F401  (re-exported)

NSUM = 34
TRI6 = [(r, c) for r in range(6) for c in range(r, 6)]
TRI3 = [(r, c) for r in range(3) for c in range(r, 3)]
GRID_MARGIN = 1e-6      # see MapIndex.grid_margin and gates(): the typed comparisons round in float32 (6e-8), so the margins asked of the
GATE_MARGIN = 1e-6      # inputs are 1e-6: exact arithmetic and the float-typed code of either side then decide every row alike


def to_mp(a):
    """float64 array -> object array of mpf (exact)."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for k, x in enumerate(a.reshape(-1)):
        flat[k] = mpf(float(x))
    return out


def _sqrt(x):
    if x.dtype != object:
        return np.sqrt(x)
    return np.array([mp.sqrt(v) for v in x], dtype=object)


# ---- nested-list 3 x 3 algebra: M[r][c] is a scalar or an array over the points -------------------------------------------------------
def _mat(A):
    """(3, 3) or (n, 3, 3) array -> nested list."""
    A = np.asarray(A)
    return [[A[..., r, c] for c in range(3)] for r in range(3)]


def _mm(A, B):
    return [[A[r][0] * B[0][c] + A[r][1] * B[1][c] + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]


def _mv(A, x):
    return [A[r][0] * x[0] + A[r][1] * x[1] + A[r][2] * x[2] for r in range(3)]


def _tr(A):
    return [[A[c][r] for c in range(3)] for r in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _hat(v, sg):
    z = v[0] * 0
    return [[z, sg * v[2], v[1]], [v[2], z, sg * v[0]], [sg * v[1], v[0], z]]


def _add(A, B):
    return [[A[r][c] + B[r][c] for c in range(3)] for r in range(3)]


def point_terms(pnt, var, cen, nrm, pv, R, p, rot_var, tsl_var, mag_of=None):
    """Everything one scan point contributes when tested against one plane record, vectorised over the points.
    pnt (n, 3), var (n, 3, 3), cen / nrm (n, 3), pv (n, 6, 6); R, rot_var, tsl_var (3, 3), p (3): float64 or object (mpf) arrays.
    mag_of = None: the values.  mag_of = the dict of values: the magnitudes (pass the same inputs; absolute values are taken here).
    Returns dict(wld (3 lists), resi, d2 (|wld - centre|^2), sigma, parts [plane, point, rot, tsl], R_inv, jac (6), terms (n, 34))."""
    mag = mag_of is not None
    if mag:
        pnt, var, cen, nrm, pv, R, p, rot_var, tsl_var = (np.abs(np.asarray(x, dtype=np.float64)) for x in (pnt, var, cen, nrm, pv, R, p, rot_var, tsl_var))
    sg = 1 if mag else -1
    P = [pnt[:, k] for k in range(3)]
    C = [cen[:, k] for k in range(3)]
    N = [nrm[:, k] for k in range(3)]
    Rm, V, RV, TV = _mat(R), _mat(var), _mat(rot_var), _mat(tsl_var)
    phat = _hat(P, sg)
    if pnt.dtype != object:
        A = _mm(_mm(Rm, V), _tr(Rm))
        B = _mm(_mm(phat, RV), _tr(phat))
        var_world = _add(_add(A, B), TV)
    w = _mv(Rm, P)
    wld = [w[k] + p[k] for k in range(3)]
    d = [wld[k] + sg * C[k] for k in range(3)]
    resi = _dot(N, d)
    d2 = _dot(d, d)
    J = d + [sg * N[0], sg * N[1], sg * N[2]]
    s_plane = 0
    for c in range(6):
        t = 0
        for r in range(6):
            t = t + J[r] * pv[:, r, c]
        s_plane = s_plane + t * J[c]
    if pnt.dtype == object:
        # exact arithmetic: any algebraically equal form has the same value, so the cheap one -- n^T R V R^T n = q^T V q with q = R^T n,
        # n^T phat RV phat^T n = b^T RV b with b = phat^T n -- stands in for the 3 x 3 products above
        q_ = _mv(_tr(Rm), N)
        b_ = _mv(_tr(phat), N)
        parts = [s_plane, _dot(q_, _mv(V, q_)), _dot(b_, _mv(RV, b_)), _dot(N, _mv(TV, N))]
        sigma = parts[0] + parts[1] + parts[2] + parts[3]
    else:
        sigma = s_plane + _dot(N, _mv(var_world, N))
        parts = [s_plane, _dot(N, _mv(A, N)), _dot(N, _mv(B, N)), _dot(N, _mv(TV, N))]
    if mag:
        # 1 / x with x = 0.0005 + sum of signed terms: first-order magnitude (1 / x) (sum |terms| / x)
        R_inv = mag_of["R_inv"] * (0.0005 + sigma) / (0.0005 + mag_of["sigma"])
    else:
        half_milli = mpf(0.0005) if pnt.dtype == object else 0.0005
        R_inv = 1 / (half_milli + sigma)
    q = _mv(_tr(Rm), N)
    jh = _mv(phat, q)
    jac = jh + N
    terms = np.empty((pnt.shape[0], NSUM), dtype=pnt.dtype)
    for k, (r, c) in enumerate(TRI6):
        terms[:, k] = R_inv * jac[r] * jac[c]
    for r in range(6):
        terms[:, 21 + r] = sg * (R_inv * jac[r] * resi)
    for k, (r, c) in enumerate(TRI3):
        terms[:, 27 + k] = N[r] * N[c]
    terms[:, 33] = mpf(1) if pnt.dtype == object else 1.0
    return dict(wld=wld, resi=resi, d2=d2, sigma=sigma, parts=parts, R_inv=R_inv, jac=jac, terms=terms)


def gates(resi, d2, sigma, radius, swap=None):
    """swap: None, or "range" / "sigma" to exchange `<=` and `<` on that gate (a degraded variant).  The two float-typed gates of OctoTree::match on float64 quantities: (range_ok, sigma_ok, margin).  margin: the smaller relative
    distance of the two comparisons from equality, measured on the UNROUNDED quantities (d2 - resi^2 against 9 radius; |resi| against
    3 sqrt(sigma); a row whose range gate fails is judged on that gate alone, as the code never reaches the second)."""
    resi, d2, sigma = np.asarray(resi, dtype=np.float64), np.asarray(d2, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    dtp = np.abs(resi).astype(np.float32)
    dtc = d2.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        range_dis = dtc - dtp * dtp
        lim = np.float32(9.0) * np.asarray(radius, dtype=np.float32)
        ok1 = range_dis < lim if swap == "range" else range_dis <= lim
        three_sig = 3.0 * np.sqrt(sigma)
        ok2 = dtp.astype(np.float64) <= three_sig if swap == "sigma" else dtp.astype(np.float64) < three_sig
        q = d2 - resi * resi
        m1 = np.abs(q - lim.astype(np.float64)) / np.maximum(np.maximum(d2, lim.astype(np.float64)), 1e-300)
        m2 = np.abs(np.abs(resi) - three_sig) / np.maximum(np.maximum(np.abs(resi), three_sig), 1e-300)
    return ok1, ok1 & ok2, np.where(ok1, np.minimum(m1, m2), m1)


class MapIndex:
    """The integer work of match(feat_map, ...) and OctoTree::match's descent on a flat leaf list (synth.PlaneMapData), vectorised:
    float-typed voxel index (double division rounded to float, `-= 1` in float below zero, truncation), descent by `wld > voxel_center`
    with centres built from a float quater_length, and the box of a leaf for OctoTree::inside."""

    def __init__(self, pm):
        self.pm = pm
        self.roots, inv = np.unique(pm.loc, axis=0, return_inverse=True)
        self.root_key = self._pack(self.roots)
        assert np.all(np.diff(self.root_key) > 0)
        key = inv.reshape(-1).astype(np.int64) * 4096 + pm.layer.astype(np.int64) * 512 + pm.path.astype(np.int64)
        self.order = np.argsort(key)
        self.leaf_key = key[self.order]
        assert np.all(np.diff(self.leaf_key) > 0), "two leaves on one node"

    @staticmethod
    def _pack(loc):
        off = 1 << 20
        return ((loc[:, 0] + off) << 42) | ((loc[:, 1] + off) << 21) | (loc[:, 2] + off)

    def voxel_index(self, w):
        with np.errstate(invalid="ignore", over="ignore"):
            loc = (w / self.pm.voxel_size).astype(np.float32)
            loc = np.where(loc < 0, loc - np.float32(1.0), loc)
            ok = np.all(np.isfinite(loc) & (np.abs(loc) < 2.0 ** 20), axis=1)
            return np.where(ok[:, None], loc, 0).astype(np.int64), ok

    def lookup(self, w):
        """World points (n, 3) -> index of the plane leaf each is tested against in the caller's list, -1 where the walk finds none."""
        pm = self.pm
        loc, ok = self.voxel_index(w)
        k = self._pack(loc)
        ri = np.clip(np.searchsorted(self.root_key, k), 0, len(self.root_key) - 1)
        ok &= self.root_key[ri] == k
        c = (0.5 + loc.astype(np.float64)) * pm.voxel_size
        ql = np.float32(pm.voxel_size / 4.0)
        leaf = np.full(w.shape[0], -1, dtype=np.int64)
        prefix = np.zeros(w.shape[0], dtype=np.int64)
        open_ = ok.copy()
        for layer in range(pm.max_layer + 1):
            key = ri.astype(np.int64) * 4096 + layer * 512 + prefix
            j = np.clip(np.searchsorted(self.leaf_key, key), 0, len(self.leaf_key) - 1)
            hit = open_ & (self.leaf_key[j] == key)
            leaf[hit] = self.order[j[hit]]
            open_ &= ~hit
            if layer == pm.max_layer:
                break
            with np.errstate(invalid="ignore"):
                x = (w > c).astype(np.int64)
            prefix = prefix | ((4 * x[:, 0] + 2 * x[:, 1] + x[:, 2]) << (3 * layer))
            c = c + ((2 * x - 1).astype(np.float32) * ql).astype(np.float64)
            ql = np.float32(ql / np.float32(2))
        leaf[(leaf >= 0) & (pm.is_plane[np.maximum(leaf, 0)] == 0)] = -1
        return leaf

    def inside(self, leaf, w):
        """OctoTree::inside (voxel_map.hpp:1471-1480) of leaf[i] for w[i]; False where leaf < 0."""
        pm = self.pm
        l = np.maximum(leaf, 0)
        c, h = pm.box_center[l], pm.box_half[l][:, None]
        with np.errstate(invalid="ignore"):
            return (leaf >= 0) & np.all((w >= c - h) & (w <= c + h), axis=1)

    def cache_leaf(self, prev, w):
        """The leaf tested under the node cache: the previous one if the point is still inside its box, else a new lookup."""
        keep = self.inside(prev, w)
        return np.where(keep, prev, self.lookup(w)), keep

    def grid_margin(self, w):
        """Distance of every coordinate from the nearest plane of the finest grid (voxel faces, every descent centre and every leaf box lie
        on it when voxel_size / 4 and its halves are exact in float, which `exact_grid` asserts), relative to max(|w|, voxel_size)."""
        step = self.pm.voxel_size / (1 << max(self.pm.max_layer, 1))
        f = w / step
        return np.min(np.abs(f - np.rint(f)) * step / np.maximum(np.abs(w), self.pm.voxel_size), axis=1)

    def exact_grid(self):
        pm = self.pm
        step = pm.voxel_size / (1 << max(pm.max_layer, 1))
        ok = float(np.float32(pm.voxel_size / 4.0)) == pm.voxel_size / 4.0 and math.frexp(pm.voxel_size)[0] == 0.5
        f = np.concatenate([(pm.box_center - pm.box_half[:, None]).reshape(-1), (pm.box_center + pm.box_half[:, None]).reshape(-1)]) / step
        return ok and bool(np.all(f == np.rint(f)))


def pose_of(state):
    """(R 3 x 3, p 3) of a flat state vector (R column-major)."""
    s = np.asarray(state, dtype=np.float64)
    return s[:9].reshape(3, 3).T.copy(), s[9:12].copy()


def world(pnt, state):
    R, p = pose_of(state)
    with np.errstate(invalid="ignore", over="ignore"):
        return pnt @ R.T + p


class Sweep:
    """One sweep of a scan against a map at one pose, by the float64 restatement, with the first `n_exact` rows redone in mpmath.
    leaf: the leaf every row is tested against (MapIndex.lookup / cache_leaf).  Attributes over the rows: flag, sigma, sig_mag, margin,
    terms / mags (n, 34) float64 (zero rows where unmatched); for the exact rows terms_hi + terms_lo and sigma_hi + sigma_lo."""

    def __init__(self, pm, pnt, var, state, cov, leaf, n_exact=0, exact_from=None):
        """exact_from: a sweep of the same points at the same state and covariance whose exact rows are taken over where the leaf is the same."""
        n = pnt.shape[0]
        R, p = pose_of(state)
        cov = np.asarray(cov, dtype=np.float64)
        rv, tv = cov[:3, :3].copy(), cov[3:6, 3:6].copy()
        self.n, self.leaf = n, leaf
        t = np.nonzero(leaf >= 0)[0]
        l = leaf[t]
        args = (pnt[t], var[t], pm.center[l], pm.normal[l], pm.plane_var[l])
        with np.errstate(invalid="ignore", over="ignore"):
            v = point_terms(*args, R, p, rv, tv)
            m = point_terms(*args, R, p, rv, tv, mag_of=v)
        ok1, ok, marg = gates(v["resi"], v["d2"], v["sigma"], pm.radius[l])
        self.flag = np.zeros(n, dtype=bool); self.flag[t] = ok
        self.range_ok = np.zeros(n, dtype=bool); self.range_ok[t] = ok1
        self.margin = np.full(n, np.inf); self.margin[t] = marg
        self.sigma = np.zeros(n); self.sigma[t] = np.where(ok, v["sigma"], 0.0)
        self.sig_mag = np.zeros(n); self.sig_mag[t] = np.where(ok, m["sigma"], 0.0)
        self.resi = np.zeros(n); self.resi[t] = v["resi"]
        self.d2 = np.zeros(n); self.d2[t] = v["d2"]
        self.sigma_all = np.zeros(n); self.sigma_all[t] = v["sigma"]
        self.R_inv = np.ones(n); self.R_inv[t] = v["R_inv"]
        self._sums = {}
        self.terms = np.zeros((n, NSUM)); self.terms[t] = np.where(ok[:, None], v["terms"], 0.0)
        self.mags = np.zeros((n, NSUM)); self.mags[t] = np.where(ok[:, None], m["terms"], 0.0)
        self.n_exact = min(n_exact, n)
        self.terms_hi, self.terms_lo = self.terms.copy(), np.zeros((n, NSUM))
        self.sigma_hi, self.sigma_lo = self.sigma.copy(), np.zeros(n)
        self.k_term = self.k_sigma = 0.0
        if self.n_exact and exact_from is not None and np.array_equal(leaf[: self.n_exact], exact_from.leaf[: self.n_exact]):
            for name in ("terms_hi", "terms_lo", "sigma_hi", "sigma_lo"):
                getattr(self, name)[: self.n_exact] = getattr(exact_from, name)[: self.n_exact]
            for name in ("k_term", "k_sigma", "exact_resi", "exact_sigma", "exact_d2"):
                setattr(self, name, getattr(exact_from, name))
        elif self.n_exact:
            self._exact(pm, pnt, var, R, p, rv, tv)

    @_hp
    def _exact(self, pm, pnt, var, R, p, rv, tv):
        e = np.nonzero(self.leaf[: self.n_exact] >= 0)[0]          # every row that is tested against a leaf
        self.exact_resi, self.exact_sigma, self.exact_d2 = {}, {}, {}
        if e.size == 0:
            return
        l = self.leaf[e]
        x = point_terms(to_mp(pnt[e]), to_mp(var[e]), to_mp(pm.center[l]), to_mp(pm.normal[l]), to_mp(pm.plane_var[l]), to_mp(R), to_mp(p), to_mp(rv), to_mp(tv))
        # the verdict of exact arithmetic is the restatement's: both gates clear by GATE_MARGIN (asserted by the CPU test on `margin`)
        f = self.flag[e]
        hi, lo = split_hi_lo(x["terms"][f])
        ef = e[f]
        if ef.size:
            self.k_term = float(err_units(self.terms[ef], hi, lo, self.mags[ef]).max())
            self.terms_hi[ef], self.terms_lo[ef] = hi, lo
            shi, slo = split_hi_lo(np.array(x["sigma"], dtype=object)[f])
            self.k_sigma = float(err_units(self.sigma[ef], shi, slo, self.sig_mag[ef]).max())
            self.sigma_hi[ef], self.sigma_lo[ef] = shi, slo
        self.exact_resi = dict(zip(e.tolist(), x["resi"]))
        self.exact_sigma = dict(zip(e.tolist(), x["sigma"]))
        self.exact_d2 = dict(zip(e.tolist(), x["d2"]))

    def sums(self, n):
        """(S hi, S lo, A) over the first n rows: the exact sum of the exact terms where they exist and math.fsum of the restatement's terms
        above (split hi + lo, so the reference itself carries no rounding beyond the terms'), and the sum of the magnitudes."""
        if n in self._sums:
            return self._sums[n]
        S = np.zeros(NSUM); L = np.zeros(NSUM)
        f = np.nonzero(self.flag[:n])[0]
        for k in range(NSUM):
            cols = np.concatenate([self.terms_hi[f, k], self.terms_lo[f, k]])
            s = math.fsum(cols)
            S[k], L[k] = s, math.fsum(np.concatenate([cols, [-s]]))
        self._sums[n] = S, L, self.mags[:n].sum(axis=0)
        return self._sums[n]


def unpack34(res):
    """A sweep dict (HTH 6 x 6, HTz 6, nnt 3 x 3, match_num) -> the 34 sums."""
    out = np.zeros(NSUM)
    for k, (r, c) in enumerate(TRI6):
        out[k] = res["HTH"][r, c]
    out[21:27] = res["HTz"]
    for k, (r, c) in enumerate(TRI3):
        out[27 + k] = res["nnt"][r, c]
    out[33] = res["match_num"]
    return out


# ---- the EKF step -----------------------------------------------------------------------------------------------------------------------
def _mp_log(dR):
    tr = dR[0, 0] + dR[1, 1] + dR[2, 2]
    theta = mpf(0) if tr > mpf(3.0) - mpf(1e-6) else mp.acos((tr - 1) / 2)
    f = mpf(0.5) if abs(theta) < mpf(0.001) else theta / mp.sin(theta) / 2
    K = [dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]
    gap = mpf(3.0) - tr          # the branch compares 3 - tr with 1e-6, and |theta| with 0.001
    branch = min(abs(gap - mpf(1e-6)) / max(abs(gap), mpf(1e-6)), mpf(1) if theta == 0 else abs(abs(theta) - mpf(0.001)) / mpf(0.001))
    return [f * k for k in K], f, branch


def _mp_exp(w):
    n = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    if n < mpf(1e-11):
        return mp.eye(3)
    k = [x / n for x in w]
    K = mp.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return mp.eye(3) + mp.sin(n) * K + (1 - mp.cos(n)) * (K * K)


def jacobi_cond(S):
    d = 1.0 / np.sqrt(np.diag(S))
    return float(np.linalg.cond(S * d[:, None] * d[None, :]))


@_hp
def ekf_exact(state, cov, sweeps, literal=False):
    """Replay of voxelslam.cpp:921-957 in mpmath from the given sweeps (dicts of HTH, HTz, nnt, match_num, one per iteration that was run).
    Returns dict: iterations, rematch (the rematch_num after every iteration), converged (per iteration), margin (the smallest relative
    distance of any convergence comparison or Log / Exp branch from its threshold), state (24, float64 nearest) with R (mp 3 x 3) and
    x (mp list of the 12 vector components), cov / cov_lo, bound_state (15) and bound_cov (15, 15) in units of u (already multiplied by the
    Jacobi-scaled condition number, summed over the iterations), kappa (per iteration), min_eig (mpf), per-iteration K, G, vec, sol."""
    s = np.asarray(state, dtype=np.float64)
    R0 = mp.matrix(3, 3)
    for r in range(3):
        for c in range(3):
            R0[r, c] = mpf(float(s[3 * c + r]))
    x0 = [mpf(float(v)) for v in s[9:21]]
    Rc, xc = R0.copy(), list(x0)
    C = mp.matrix(15, 15)
    cov = np.asarray(cov, dtype=np.float64)
    for r in range(15):
        for c in range(15):
            C[r, c] = mpf(float(cov[r, c]))
    Cinv = C ** -1
    out = dict(rematch=[], converged=[], kappa=[], K=[], G=[], vec=[], sol=[], margin=mpf(1))
    bound_state = np.zeros(15)
    rematch, done = 0, False
    for it, sw in enumerate(sweeps):
        assert not done, "more sweeps than the exact schedule runs"
        H = mp.matrix(6, 6); z = mp.matrix(6, 1)
        for r in range(6):
            z[r] = mpf(float(sw["HTz"][r]))
            for c in range(6):
                H[r, c] = mpf(float(sw["HTH"][r, c]))
        S = Cinv.copy()
        for r in range(6):
            for c in range(6):
                S[r, c] += H[r, c]
        K = S ** -1
        K6 = K[:, 0:6]
        G = K6 * H
        dR = Rc.T * R0
        wv, f, br = _mp_log(dR)
        vec = mp.matrix(wv + [x0[k] - xc[k] for k in range(12)])
        # magnitude of vec: the sum of the absolute values of what each component is made of (two 3-term dot products; two numbers).
        # literal=True: |vec_i| itself (tests/_lio_cases.py, "Magnitudes", says what that measures)
        if literal:
            vmag = [abs(v) for v in vec]
        else:
            vmag = [f * sum(abs(Rc[k, a]) * abs(R0[k, b]) + abs(Rc[k, b]) * abs(R0[k, a]) for k in range(3)) for a, b in ((2, 1), (0, 2), (1, 0))]
            vmag += [abs(x0[k]) + abs(xc[k]) for k in range(12)]
        sol = K6 * z + vec - G * vec[0:6, 0]
        mag = [sum(abs(K[i, j]) * abs(z[j]) for j in range(6)) + vmag[i] + sum(abs(G[i, j]) * vmag[j] for j in range(6)) for i in range(15)]
        kap = jacobi_cond(np.array(S.tolist(), dtype=np.float64))
        bound_state += kap * np.array([float(m) for m in mag])
        Rc = Rc * _mp_exp([sol[0], sol[1], sol[2]])
        xc = [xc[k] + sol[3 + k] for k in range(12)]
        rot_add = mp.sqrt(sol[0] ** 2 + sol[1] ** 2 + sol[2] ** 2); tra_add = mp.sqrt(sol[3] ** 2 + sol[4] ** 2 + sol[5] ** 2)
        a, b = rot_add * mpf(57.3), tra_add * 100
        conv = a < mpf(0.01) and b < mpf(0.015)
        m = min(abs(a - mpf(0.01)) / mpf(0.01), abs(b - mpf(0.015)) / mpf(0.015), br, abs(rot_add - mpf(1e-11)) / max(rot_add, mpf(1e-11)))
        out["margin"] = min(out["margin"], m)
        if conv or (rematch == 0 and it == 4 - 2):
            rematch += 1
        for key, v in (("rematch", rematch), ("converged", bool(conv)), ("kappa", kap), ("K", K), ("G", G), ("vec", vec), ("sol", sol)):
            out[key].append(v)
        if rematch >= 2 or it == 4 - 1:
            done = True
            G15 = mp.zeros(15, 15)
            G15[:, 0:6] = G
            Cn = (mp.eye(15) - G15) * C
            cm = np.array([[float(abs(C[r, c]) + sum(abs(G[r, k]) * abs(C[k, c]) for k in range(6))) for c in range(15)] for r in range(15)])
            out["bound_cov"] = kap * cm
            ex = np.array(Cn.tolist(), dtype=object)
            out["cov"], out["cov_lo"] = split_hi_lo(ex)
    out["finished"] = done
    out["iterations"] = len(sweeps)
    out["R"], out["x"] = Rc, xc
    st = s.copy()
    for r in range(3):
        for c in range(3):
            st[3 * c + r] = float(Rc[r, c])
    st[9:21] = [float(v) for v in xc]
    out["state"] = st
    out["bound_state"] = bound_state
    nn = mp.matrix([[mpf(float(sweeps[-1]["nnt"][r, c])) for c in range(3)] for r in range(3)])
    out["min_eig"] = min(mp.eigsy(nn, eigvals_only=True))
    out["nnt_norm"] = float(np.linalg.norm(sweeps[-1]["nnt"], 2))
    return out


@_hp
def state_error(got, ex):
    """|got [-] exact| per tangent component (15): the rotation as the vee of the skew part of R*^T R (its first-order Log), the rest plainly."""
    g = np.asarray(got, dtype=np.float64)
    Rg = mp.matrix(3, 3)
    for r in range(3):
        for c in range(3):
            Rg[r, c] = mpf(float(g[3 * c + r]))
    dR = ex["R"].T * Rg
    e = [abs(dR[2, 1] - dR[1, 2]) / 2, abs(dR[0, 2] - dR[2, 0]) / 2, abs(dR[1, 0] - dR[0, 1]) / 2]
    e += [abs(mpf(float(g[9 + k])) - ex["x"][k]) for k in range(12)]
    return np.array([float(v) for v in e])


# float64 models of the EKF algebra (python floats: no contraction), for the measured constants and the degraded variants
def dm_inverse(A):
    """csrc/vxba_imu.hpp dm_inverse: LU with row pivoting, column by column solves; A row-major nested / ndarray, returns ndarray."""
    n = len(A)
    lu = [[float(A[i][j]) for j in range(n)] for i in range(n)]
    perm = list(range(n))
    for k in range(n):
        piv = max(range(k, n), key=lambda i: (abs(lu[i][k]), -i))
        if lu[piv][k] == 0.0:
            raise ZeroDivisionError("singular")
        if piv != k:
            lu[k], lu[piv] = lu[piv], lu[k]; perm[k], perm[piv] = perm[piv], perm[k]
        d = lu[k][k]
        for i in range(k + 1, n):
            lu[i][k] /= d
        for j in range(k + 1, n):
            ukj = lu[k][j]
            if ukj == 0.0:
                continue
            for i in range(k + 1, n):
                lu[i][j] -= lu[i][k] * ukj
    inv = np.zeros((n, n))
    for c in range(n):
        x = [1.0 if perm[i] == c else 0.0 for i in range(n)]
        for j in range(n):
            if x[j] != 0.0:
                for i in range(j + 1, n):
                    x[i] -= lu[i][j] * x[j]
        for j in range(n - 1, -1, -1):
            x[j] /= lu[j][j]
            for i in range(j):
                x[i] -= lu[i][j] * x[j]
        inv[:, c] = x
    return inv


def gauss_jordan(A):
    """The device EKF's elimination order (lio_ekf_kernel): in-place Gauss-Jordan without pivoting, every entry from the old matrix."""
    S = np.array(A, dtype=np.float64)
    n = S.shape[0]
    for p in range(n):
        ip = 1.0 / S[p, p]
        N = S - np.outer(S[:, p], S[p, :]) * ip
        N[p, :] = S[p, :] * ip
        N[:, p] = -S[:, p] * ip
        N[p, p] = ip
        S = N
    return S


def _so3_log(dR):
    tr = dR[0, 0] + dR[1, 1] + dR[2, 2]
    theta = 0.0 if tr > 3.0 - 1e-6 else math.acos(0.5 * (tr - 1))
    f = 0.5 if abs(theta) < 0.001 else 0.5 * theta / math.sin(theta)
    return f * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])


def _so3_exp(w):
    n = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if n < 1e-11:
        return np.eye(3)
    k = w / n
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(n) * K + (1 - math.cos(n)) * (K @ K)


def ekf_f64(state, cov, sweeps, inverse=dm_inverse, variant=None):
    """The host path of vxba_lio_state_estimation in float64 from given sweeps: dict(state, cov, iterations).  variant: None, "f32S" (the
    inverse taken on S rounded to float32), "gcols" (G applied with five columns instead of six), "inplace" ((I - G) cov updated in place)."""
    s = np.asarray(state, dtype=np.float64).copy()
    cov = np.asarray(cov, dtype=np.float64).copy()
    R0, x0 = s[:9].reshape(3, 3).T.copy(), s[9:21].copy()
    Rc, xc = R0.copy(), x0.copy()
    cinv = dm_inverse(cov)
    ng = 5 if variant == "gcols" else 6
    rematch, it_done = 0, 0
    for it, sw in enumerate(sweeps):
        S = cinv.copy()
        S[:6, :6] += sw["HTH"]
        if variant == "f32S":
            S = S.astype(np.float32).astype(np.float64)
        K = inverse(S)
        G = np.zeros((15, 6))
        for c in range(6):
            for k in range(6):
                G[:, c] += K[:, k] * sw["HTH"][k, c]
        vec = np.concatenate([_so3_log(Rc.T @ R0), x0 - xc])
        sol = np.zeros(15)
        for k in range(6):
            sol += K[:, k] * sw["HTz"][k]
        sol += vec
        for k in range(ng):
            sol -= G[:, k] * vec[k]
        Rc = Rc @ _so3_exp(sol[:3]); xc = xc + sol[3:]
        conv = math.sqrt(sol[0] ** 2 + sol[1] ** 2 + sol[2] ** 2) * 57.3 < 0.01 and math.sqrt(sol[3] ** 2 + sol[4] ** 2 + sol[5] ** 2) * 100 < 0.015
        if conv or (rematch == 0 and it == 2):
            rematch += 1
        it_done = it + 1
        if rematch >= 2 or it == 3:
            if variant == "inplace":
                for c in range(15):
                    for r in range(15):
                        t = cov[r, c]
                        for k in range(6):
                            t -= G[r, k] * cov[k, c]
                        cov[r, c] = t
            else:
                nc = cov.copy()
                for k in range(ng):
                    nc -= np.outer(G[:, k], cov[k, :])
                cov = nc
            break
    s[:9] = Rc.T.reshape(9); s[9:21] = xc
    return dict(state=s, cov=cov, iterations=it_done)


# ---- var_init / pvec_update ---------------------------------------------------------------------------------------------------------------
def var_init_terms(xyz, ext_R, ext_p, dept_err, beam_err, exact=False, norms=None):
    """var_init with calcBodyVar (voxelslam.hpp:164-201) over float32 sensor points: (pnt (n, 3), var (n, 3, 3), (|b1|, |b2|)) as float64 / mpf
    object arrays.  The float-typed quantities (range, range_var, the beam variance from a float degree_inc) are taken as the code types them.
    norms = the third result of a value run: the magnitudes instead (absolute values, every subtraction an addition, the two
    normalisations dividing by the true norms)."""
    mag = norms is not None
    xyz = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    pb = xyz.copy()
    pb[pb[:, 2] == 0, 2] = 0.0001
    rng = np.sqrt(pb[:, 0] ** 2 + pb[:, 1] ** 2 + pb[:, 2] ** 2).astype(np.float32).astype(np.float64)
    range_var = float(np.float32(dept_err) * np.float32(dept_err))
    dv = math.pow(math.sin(float(np.float32(beam_err)) * 0.017453293), 2)
    E = np.asarray(ext_R, dtype=np.float64); ep = np.asarray(ext_p, dtype=np.float64)
    cv = to_mp if exact else (lambda a: np.asarray(a, dtype=np.float64))
    sg = 1 if mag else -1
    if mag:
        pb, E, ep = np.abs(pb), np.abs(E), np.abs(ep)
    P = [cv(pb[:, k]) for k in range(3)]
    r = cv(rng); Em = _mat(cv(E)); rvar = cv(np.array(range_var)).reshape(())[()]; dvv = cv(np.array(dv)).reshape(())[()]
    nn = _sqrt(_dot(P, P))
    d = [P[k] / nn for k in range(3)]
    one = P[0] * 0 + 1
    b1 = [one, one, sg * (d[0] + d[1]) / d[2]]
    n1 = _sqrt(_dot(b1, b1)); b1 = [b / n1 for b in b1]
    cross = lambda a, b: [a[1] * b[2] + sg * a[2] * b[1], a[2] * b[0] + sg * a[0] * b[2], a[0] * b[1] + sg * a[1] * b[0]]
    b2 = cross(b1, d)
    n2 = _sqrt(_dot(b2, b2))
    if mag:
        b1 = [b * n1 / norms[0] for b in b1]
        b2 = [b / norms[1] for b in cross(b1, d)]
    else:
        b2 = [b / n2 for b in b2]
    a1 = [r * v for v in cross(d, b1)]; a2 = [r * v for v in cross(d, b2)]
    V = [[d[i] * rvar * d[j] + a1[i] * dvv * a1[j] + a2[i] * dvv * a2[j] for j in range(3)] for i in range(3)]
    W = _mm(_mm(Em, V), _tr(Em))
    pnt = [_mv(Em, P)[k] + cv(np.array(ep[k])).reshape(())[()] for k in range(3)]
    n = xyz.shape[0]
    dt = object if exact else np.float64
    op, ov = np.empty((n, 3), dtype=dt), np.empty((n, 3, 3), dtype=dt)
    for i in range(3):
        op[:, i] = pnt[i]
        for j in range(3):
            ov[:, i, j] = W[i][j]
    return op, ov, (n1, n2)


def pvec_terms(pnt, var, state, cov, exact=False, mag=False):
    """pvec_update (voxelslam.hpp:203-215): (world points (n, 3), world covariances (n, 3, 3))."""
    R, p = pose_of(state)
    cov = np.asarray(cov, dtype=np.float64)
    rv, tv = cov[:3, :3], cov[3:6, 3:6]
    cv = to_mp if exact else (lambda a: np.asarray(a, dtype=np.float64))
    sg = 1 if mag else -1
    if mag:
        pnt, var, R, p, rv, tv = (np.abs(x) for x in (pnt, var, R, p, rv, tv))
    P = [cv(pnt[:, k]) for k in range(3)]
    Rm, V, RV, TV = _mat(cv(R)), _mat(cv(var)), _mat(cv(rv)), _mat(cv(tv))
    pm_ = cv(p)
    phat = _hat(P, sg)
    W = _add(_add(_mm(_mm(Rm, V), _tr(Rm)), _mm(_mm(phat, RV), _tr(phat))), TV)
    w = _mv(Rm, P)
    n = pnt.shape[0]
    dt = object if exact else np.float64
    op, ov = np.empty((n, 3), dtype=dt), np.empty((n, 3, 3), dtype=dt)
    for i in range(3):
        op[:, i] = w[i] + pm_[i]
        for j in range(3):
            ov[:, i, j] = W[i][j] + P[0] * 0
    return op, ov
