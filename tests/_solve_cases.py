"""Deterministic systems for the damped-solve tests (tests/test_solve_cpu.py, tests/test_gpu_solve.py, scripts/run_solve_accuracy.py).

Every matrix is A = Q diag(s) Q^T with a log-spaced spectrum s and a random orthogonal Q.  The solvers damp what they
are given -- they solve (H + u diag(H)) x = -J -- and with a random Q the damping term alone would bring every condition number down to a
few thousand.  So the prescribed spectrum is that of the DAMPED system: H gets the off-diagonal entries of A and the diagonal A_ii / (1 + u),
and the condition number a family claims is the one the elimination meets (tests/test_solve_cpu.py asserts it).

Families (narrow solve, every W in 1 .. 10; the host solve also at W = 11, 37, 128):
  spd_1e2 / spd_1e6 / spd_1e10 / spd_1e13   positive definite, u = 0.01
  indef                                     cond 1e4, a quarter of the eigenvalues negative (the exact-Hessian case of test_gpu_edges.py)
  scaled_lo / scaled_hi                     spd_1e6 with H and J times 1e-140 / 1e+140
  null_mid / null_last / null_pair / null_allbut1   empty frames (block rows and columns 0, J = 0 there); the live part is spd_1e6
  diagonal                                  a diagonal Hessian
  u_1e-6 / u_0.01 / u_10                    H itself with cond 1e6, damped by the three values
  li (W in LI_WINDOWS)                      the LiDAR-inertial form: E symmetric and indefinite, H + u diag(H) + E with cond 1e6, e random

Acceptance of the indefinite cases (tests/test_gpu_solve.py): unpivoted elimination has element growth there, so the yardstick is the numpy
model of the same elimination (tests/test_solve4_model.py) and eta_device <= K eta_model + n 2^-53 1e-3.  K is twice the largest per-case
ratio of eta between variants of the model that differ only in rounding (measured_rounding_ratio below: products as written / every a - g l
as one single-rounding FMA through longdouble; reciprocal by division / a 2^-23 estimate refined by the kernel's cubic step e = 1 - d r,
r (1 + e + e^2)).  The device differs from the model in exactly these roundings, hence the factor two.
Measured on the CPU when this file was written: largest ratio 3.12 (indef, W = 9), K = 6.25.  The tests measure it again at run time
(indefinite_K) and use that figure; test_solve_cpu.py checks the figure recorded here against it.
"""
import functools
import zlib

import numpy as np

from . import _solve_ref as R
from . import test_solve4_model as M4

NARROW_WINDOWS = tuple(range(1, 11))
LI_WINDOWS = (2, 3, 5, 6, 9, 10)
HOST_WINDOWS = (1, 2, 5, 10, 11, 37, 128)
WIDE_SIZES = (66, 96, 192, 222, 594, 768)
WIDE_CONDS = (1e2, 1e6, 1e10)
RECORDED_RATIO = 3.12      # see the header


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def spectral(m, s, rng):
    """Q diag(s) Q^T (m x m), rounded to float64 and symmetric to the bit.  The terms are summed decade by decade of |s|, smallest first, each
    decade a float64 product and the sum in longdouble: a term's rounding error is then relative to its own eigenvalues, not to the largest,
    and the small end of a cond 1e13 spectrum survives (a plain float64 product would bury it; a longdouble product takes seconds at m = 762)."""
    if m == 0:
        return np.zeros((0, 0))
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    s = np.asarray(s, dtype=np.float64)
    dec = np.floor(np.log10(np.abs(s))).astype(int)
    A = np.zeros((m, m), dtype=np.longdouble)
    for d in np.unique(dec):
        Qd = Q[:, dec == d]
        A += (Qd * s[dec == d][None, :]) @ Qd.T
    A = np.asarray(A, dtype=np.float64)
    return np.tril(A) + np.tril(A, -1).T


def log_spectrum(m, cond, neg_quarter=False, rng=None):
    s = np.logspace(0, -np.log10(cond), m) if m > 1 else np.ones(m)
    if neg_quarter:
        # a quarter of the signs, all in the upper half of the magnitudes (never the largest): the negative end stays well above 1e-3 lambda_max
        flip = 1 + rng.permutation(max(1, m // 2 - 1))[:max(1, m // 4)]
        s[flip] *= -1.0
    return s


def poses(W, rng):
    Rp = np.zeros((W, 12))
    for j in range(W):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(Q) < 0:
            Q[:, 0] *= -1
        Rp[j, :9] = Q.T.reshape(9)          # column-major
        Rp[j, 9:] = rng.standard_normal(3) * 5
    return Rp


def undamp(A, u):
    """H with H + u diag(H) == A up to one rounding per diagonal entry."""
    H = A.copy()
    H[np.diag_indices(A.shape[0])] = np.diag(A) / (1.0 + u)
    return H


def embed(W, Alive, live_frames, rng, jscale=1.0):
    """(6W)^2 gauge-fixed H (frame 0: identity) with Alive on the rows of live_frames, zeros on the other frames; J likewise."""
    n = 6 * W
    H, J = np.zeros((n, n)), np.zeros(n)
    idx = np.concatenate([np.arange(6 * f, 6 * f + 6) for f in live_frames]) if len(live_frames) else np.zeros(0, int)
    H[np.ix_(idx, idx)] = Alive
    J[idx] = rng.standard_normal(idx.size) * jscale
    H[:6, :6] = np.eye(6)
    return H, J


def raw_from_fixed(H, J, rng):
    """What the Hessian sweep hands over before the gauge fix: the same system with frame 0's rows and columns filled in."""
    n = H.shape[0]
    Hr, Jr = H.copy(), J.copy()
    blk = rng.standard_normal((6, n))
    Hr[:6, :] = blk
    Hr[:, :6] = blk.T
    Hr[:6, :6] = blk[:, :6] @ blk[:, :6].T + np.eye(6)
    Jr[:6] = rng.standard_normal(6)
    return Hr, Jr


def jscale(cond):
    """Scale of the right-hand side: 0.3 x the smallest eigenvalue (the largest is 1), so that a step turns a frame by a fraction of a radian.  With
    J of order 1 the steps of the ill-conditioned cases turn by up to 1e12 radians, and the trial rotations then measure how the angle was
    rounded, on the device and on the host alike."""
    return 0.3 / cond


def _case(name, W, H, J, u, rng, kind, cond=None, dead=(), **kw):
    c = dict(name=name, W=W, H=H, J=J, u=u, Rp=poses(W, rng), kind=kind, cond=cond, dead=tuple(dead))
    c.update(kw)
    return c


def null_sets(W):
    """name -> empty frames (among 1 .. W-1), the sets that exist at this W."""
    out = {}
    if W >= 3:
        out["null_mid"] = (W // 2,)
    if W >= 2:
        out["null_last"] = (W - 1,)
    if W >= 4:
        out["null_pair"] = (1, W - 1)
        keep = W // 2
        out["null_allbut1"] = tuple(f for f in range(1, W) if f != keep)
    return out


@functools.lru_cache(maxsize=None)
def narrow_cases(W):
    """All LiDAR-only cases of one window size (any W >= 1), as a tuple of dicts (shared, never modified)."""
    m = 6 * W - 6
    live = list(range(1, W))
    out = []
    if W == 1:
        rng = _rng("w1")
        H, J = embed(1, np.zeros((0, 0)), [], rng)
        return (_case("w1", 1, H, J, 0.01, rng, "spd", cond=1.0),)
    base = {}
    for cond in (1e2, 1e6, 1e10, 1e13):
        rng = _rng("spd", W, cond)
        A = spectral(m, log_spectrum(m, cond), rng)
        H, J = embed(W, undamp(A, 0.01), live, rng, jscale(cond))
        name = f"spd_1e{int(round(np.log10(cond)))}"
        out.append(_case(name, W, H, J, 0.01, rng, "spd", cond=cond))
        base[name] = out[-1]
    rng = _rng("indef", W)
    A = spectral(m, log_spectrum(m, 1e4, True, rng), rng)
    H, J = embed(W, undamp(A, 0.01), live, rng, jscale(1e4))
    out.append(_case("indef", W, H, J, 0.01, rng, "indef", cond=1e4))
    b6 = base["spd_1e6"]
    for name, f in (("scaled_lo", 1e-140), ("scaled_hi", 1e140)):
        H = b6["H"] * f
        H[:6, :6] = np.eye(6)
        out.append(dict(b6, name=name, H=H, J=b6["J"] * f, kind="scaled", scale=f))
    for name, dead in null_sets(W).items():
        rng = _rng(name, W)
        lv = [f for f in live if f not in dead]
        A = spectral(6 * len(lv), log_spectrum(6 * len(lv), 1e6), rng)
        H, J = embed(W, undamp(A, 0.01), lv, rng, jscale(1e6))
        out.append(_case(name, W, H, J, 0.01, rng, "null", cond=1e6, dead=dead))
    rng = _rng("diagonal", W)
    H, J = embed(W, np.diag(rng.permutation(np.logspace(0, -6, m))), live, rng, jscale(1e6))
    out.append(_case("diagonal", W, H, J, 0.01, rng, "spd", cond=1e6))
    for u, tag in ((1e-6, "u_1e-6"), (0.01, "u_0.01"), (10.0, "u_10")):
        rng = _rng("u", W)              # the same H for the three values
        A = spectral(m, log_spectrum(m, 1e6), rng)
        H, J = embed(W, A, live, rng, jscale(1e6))
        out.append(_case(tag, W, H, J, u, rng, "spd", cond=None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def li_case(W):
    """The LiDAR-inertial form: li_rec = [u | poses | e | E column-major]; (H + u diag(H) + E)[6:, 6:] has cond 1e6."""
    rng = _rng("li", W)
    n, m, u = 6 * W, 6 * W - 6, 0.01
    A = spectral(m, log_spectrum(m, 1e6), rng)
    G = rng.standard_normal((n, n)) * 0.05
    E = G + G.T                                   # symmetric, indefinite, the size of A's entries
    T = A - E[6:, 6:]
    H, J = embed(W, undamp(T, u), list(range(1, W)), rng, jscale(1e6))
    e = rng.standard_normal(n) * jscale(1e6)
    c = _case("li", W, H, J, u, rng, "li", cond=1e6, E=E, e=e)
    c["li_rec"] = np.concatenate([[u], c["Rp"].reshape(-1), e, E.T.reshape(-1)])
    return c


def host_cases(W):
    """The same families for the host's pivoted LDL^T, which takes any W up to 128."""
    return narrow_cases(W)


@functools.lru_cache(maxsize=None)
def wide_case(n, cond):
    """packed = [H column-major | JacT | residual] for the wide Cholesky: gauge-fixed and raw (frame 0 filled in) versions of the same system."""
    W, u = n // 6, 0.01
    rng = _rng("wide", n, cond)
    A = spectral(n - 6, log_spectrum(n - 6, cond), rng)
    H, J = embed(W, undamp(A, u), list(range(1, W)), rng, jscale(cond))
    Hr, Jr = raw_from_fixed(H, J, rng)
    res = float(rng.uniform(1, 2))
    pack = lambda Hm, Jv: np.concatenate([Hm.T.reshape(-1), Jv, [res]])
    return dict(name=f"wide_{n}_1e{int(round(np.log10(cond)))}", n=n, W=W, H=H, J=J, u=u, cond=cond, residual=res, packed=pack(H, J), packed_raw=pack(Hr, Jr), dead=())


@functools.lru_cache(maxsize=None)
def wide_negative_case(n=96):
    """Leading part positive definite, then one strongly negative diagonal entry (index k): the Cholesky must report a pivot, not a result."""
    c = dict(wide_case(n, 1e2))
    k = 6 + (n - 6) // 2
    H = c["H"].copy()
    H[k, k] = -10.0
    c.update(name=f"wide_{n}_negative", H=H, k=k, packed=np.concatenate([H.T.reshape(-1), c["J"], [c["residual"]]]))
    return c


# ---- variants of the model's arithmetic ------------------------------------------------------------------------------------------------
def fma_ld(c, a, b):
    """c - a b with one rounding, emulated through longdouble (64-bit significand: the product of two float64 is not exact there, the
    double rounding that remains is far below what the comparison is about)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(np.asarray(c, dtype=np.longdouble) - np.asarray(a, dtype=np.longdouble) * np.asarray(b, dtype=np.longdouble), dtype=np.float64)


def round_rel(q, bits):
    """q rounded to `bits` significand bits (any exponent: float32 itself would flush the block-scaled cases)."""
    mant, ex = np.frexp(q)
    return np.ldexp(np.round(mant * 2.0 ** bits) / 2.0 ** bits, ex)


def rcp_device(d, est_bits=23, null_rule=True):
    """s4_rcp of vxba_solve4.hpp on the host: an estimate good to est_bits, e = 1 - d r, r (1 + e + e^2), each step one FMA."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = round_rel(1.0 / d, est_bits)
        e = fma_ld(1.0, d, r)
        t = fma_ld(e, -e, e)
        q = fma_ld(r, -r, t)
    return np.where(np.abs(d) > 1e-300, q, 0.0) if null_rule else q


class FmaOps(M4.Ops):
    def fnma(self, c, a, b):
        return fma_ld(c, a, b)


class RcpOps(M4.Ops):
    def rcp(self, d):
        return rcp_device(d)


class FmaRcpOps(FmaOps, RcpOps):
    pass


ROUNDING_VARIANTS = (M4.Ops, FmaOps, RcpOps, FmaRcpOps)


def model_dxi(c, ops=None):
    return M4.solve4_model(c["H"], c["J"], c["u"], c["W"], 0, E=c.get("E"), e=c.get("e"), ops=ops)


def case_eta(c, dxi):
    A, b, idx = R.system(c["H"], c["J"], c["u"], c.get("E"), c.get("e"), c["dead"])
    return R.eta(A, b, dxi[idx])


@functools.lru_cache(maxsize=None)
def measured_rounding_ratio():
    """Largest per-case ratio of eta between the rounding variants of the model over the indefinite cases; (ratio, case name)."""
    worst, where = 1.0, None
    for W in NARROW_WINDOWS[1:]:
        c = next(k for k in narrow_cases(W) if k["name"] == "indef")
        etas = [case_eta(c, model_dxi(c, V())) for V in ROUNDING_VARIANTS]
        r = max(etas) / min(etas)
        if r > worst:
            worst, where = r, f"indef W={W}"
    return worst, where


def indefinite_K():
    return 2.0 * measured_rounding_ratio()[0]


# ---- acceptance criteria of the narrow solve, shared by the device tests and by the CPU tests that show they have teeth ------------------
@functools.lru_cache(maxsize=None)
def _model_eta(W, name):
    c = li_case(W) if name == "li" else next(k for k in narrow_cases(W) if k["name"] == name)
    return case_eta(c, model_dxi(c))


@functools.lru_cache(maxsize=None)
def _exact(W, name):
    c = li_case(W) if name == "li" else next(k for k in narrow_cases(W) if k["name"] == name)
    A, b, idx = R.system(c["H"], c["J"], c["u"], c.get("E"), c.get("e"), c["dead"])
    return R.exact_solve(A, b)[1], idx


def check_dxi(c, dxi):
    """Raises AssertionError unless dxi is acceptable for case c (a narrow_cases / li_case dict).  Returns the figures it judged."""
    W, n = c["W"], 6 * c["W"]
    cap = n * R.U53
    dxi = np.asarray(dxi)
    assert dxi.shape == (n,) and np.all(np.isfinite(dxi)), f"{c['name']} W={W}: dxi not finite"
    assert np.all(dxi[:6] == 0.0), f"{c['name']} W={W}: gauge rows moved"
    for f in c["dead"]:
        assert np.all(dxi[6 * f:6 * f + 6] == 0.0), f"{c['name']} W={W}: empty frame {f} moved: {dxi[6 * f:6 * f + 6]}"
    eta = case_eta(c, dxi)
    xm, idx = _exact(W, c["name"])
    ferr, xnorm = R.forward_error(dxi[idx], xm)
    msg = f"{c['name']} W={W}: eta {eta:.3e} = {eta / cap:.3g} x n 2^-53; forward error {ferr:.3e} on |x| = {xnorm:.3e}"
    if c["kind"] == "indef":
        em = _model_eta(W, c["name"])
        K = indefinite_K()
        assert eta <= K * em + cap * 1e-3, msg + f"; model eta {em:.3e}, K {K:.3g}"
    else:
        assert eta <= cap, msg
        if c["cond"] is not None:
            assert ferr <= c["cond"] * cap * xnorm, msg + f"; cond {c['cond']:.0e}"
    return dict(eta=eta, cap=cap, ferr=ferr, xnorm=xnorm)
