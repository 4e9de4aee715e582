"""The residual and the Hessian sweep in high precision (mpmath), written from the mathematics: SURVEY.md Appendix A.3 / A.4.

Test infrastructure only.  Inputs are float64 arrays (or arrays of mpf) and are taken as exact; every operation runs at `PREC` bits, so what
is returned is the true value of the operation to ~1e-58 of its magnitude.  Layouts are those of the C ABI: a cluster is [Pxx Pxy Pxz Pyy Pyz
Pzz | vx vy vz | N], a pose [R column-major | p], an eigenvector matrix column-major (u_0 first), H is returned as H[r, c].

Every result comes with its MAGNITUDE M, element by element: the same expression with every input replaced by its absolute value and every
subtraction by an addition.  A floating-point evaluation of the expression, in whatever order and association, is off by a small multiple of
u * M; an element no term reaches has M == 0 and must be an exact zero.  The magnitudes are evaluated in float64 (sums of non-negative
products: relative error ~1e-14, nothing next to the factor the criteria carry).  The issue asks for the element-wise maximum of the
magnitude of the rank-3 form (-G^T G - 2/N^2 z z^T + blockdiag D) and of the oracle's expanded form (oracle/vxo_ba.hpp:139-170): they are the
SAME number.  A^T M A and G^T G expand into the same products; the remaining terms differ only in that the expanded form writes
(2/N)(1 - n/N) w u^T and (2/N)(n - n^2/N) u u^T where the rank-3 form adds (2/N) w u^T to -(2/N^2) n w u^T (and likewise u u^T), and with
subtraction turned into addition both become (2/N)(1 + n/N) |w||u|^T and (2/N)(n + n^2/N) |u||u|^T.  2/(lambda_0 - lambda_k) enters with its
exact absolute value (to float64 rounding).

A third algebra gets a magnitude of its own, M_RR, for the rotation-rotation part of D_i only; M_H does not know of it.  With
z = P r + (u.t) v one has c1 = hat(z), the antisymmetric part of (2/N)(c1 - hat(r) P) hat(r) is what -hat(g)/2 removes, and the symmetric
part has the closed form (vector identities, P symmetric)
    (N/2) Drr = (r z^T + z r^T)/2 - (z.r) I  +  (r.r)(tr P I - P) - tr P r r^T + P r r^T + r (P r)^T - (r.P r) I,
a third of the operations of hat(r) P hat(r), and what the kernels evaluate (csrc/vxba_math.hpp).  It was added to this reference AFTER
the host build of the kernels' arithmetic had exceeded the criterion on the expanded magnitude alone (tests/_sweep_cases.py tells the
story): the closed form is the same matrix, but it reaches an element through products of size (2 coe / N)(r.r) tr P that cancel, so where
the expanded form's element is a sum of small products -- the plane normal along a body axis -- no evaluation of the closed form can be
within a fraction of u of that small magnitude.  M_RR is the closed form's own magnitude; the Hessian criterion adds a counted multiple of
it on those nine elements of each diagonal block and on no other element.

Measured on the development machine (one core, mpmath 1.3.0, PREC = 200): exact cache + hessian_exact of the whole window, memoised by case
in tests/_sweep_cases.py:
  narrow W 10 V 197: 0.5 + 2.5 s     narrow W 9 V 197: 0.4 + 2.0 s     narrow W 3 V 515: 0.7 + 0.9 s     far W 5 V 33: 0.1 + 0.1 s
  wide W 11 V 1025: 1.8 + 4.4 s      wide W 12 V 65: 0.2 + 2.0 s       wide W 128 V 40: 0.1 + 0.6 s
(wide W 11 is the one case above the 3 s asked for: its 1025 voxels are what the run lengths need; its two sub-ranges cost 2.3 and 1.1 s).
merged_exact: at most 0.4 s.  eig_residuals: 1.0 ms per voxel."""
import functools

import numpy as np
import mpmath as mp
from mpmath import mpf

PREC = 200
U64 = 2.0 ** -53


def _hp(fn):
    """Run fn at PREC bits at least (a caller's higher working precision is kept); mpmath's global precision is left alone."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with mp.workprec(max(mp.mp.prec, PREC)):
            return fn(*a, **k)
    return wrapped

_PI = ((0, 1, 2), (1, 3, 4), (2, 4, 5))     # index of P[r][c] in the packed six


def _m(x):
    return x if isinstance(x, mpf) else mpf(float(x))


def _vec(a):
    return [_m(x) for x in a]


def _sym(c6):
    return [[c6[_PI[r][c]] for c in range(3)] for r in range(3)]


def _rot(pose):
    """R[r][c] and p of a packed pose."""
    q = _vec(pose)
    return [[q[3 * c + r] for c in range(3)] for r in range(3)], q[9:12]


def _matvec(A, x):
    return [A[r][0] * x[0] + A[r][1] * x[1] + A[r][2] * x[2] for r in range(3)]


def _matTvec(A, x):
    return [A[0][c] * x[0] + A[1][c] * x[1] + A[2][c] * x[2] for c in range(3)]


def _matmul(A, B):
    return [[A[r][0] * B[0][c] + A[r][1] * B[1][c] + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]


def _hat(v):
    z = mpf(0)
    return [[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


@_hp
def transform_exact(cl, R, p):
    """tools.hpp:357-363: the cluster seen from the world, packed."""
    P, v, n = _sym(cl[:6]), cl[6:9], cl[9]
    Rv = _matvec(R, v)
    RP = _matmul(R, P)
    out = [None] * 10
    for r in range(3):
        for c in range(r, 3):
            out[_PI[r][c]] = RP[r][0] * R[c][0] + RP[r][1] * R[c][1] + RP[r][2] * R[c][2] + Rv[r] * p[c] + p[r] * Rv[c] + n * p[r] * p[c]
    for r in range(3):
        out[6 + r] = Rv[r] + n * p[r]
    out[9] = n
    return out


@_hp
def merged_exact(clusters, fix, poses):
    """World cluster of every voxel, fix + sum over the frames with N != 0 of transform(cluster_i, pose_i): ((V, 10) array of mpf, M (V, 10))."""
    clusters = np.asarray(clusters); fix = np.asarray(fix)
    V, W = clusters.shape[:2]
    Rp = [_rot(poses[i]) for i in range(W)]
    out = np.empty((V, 10), dtype=object)
    for a in range(V):
        acc = _vec(fix[a])
        for i in range(W):
            if clusters[a, i, 9] != 0:
                t = transform_exact(_vec(clusters[a, i]), *Rp[i])
                acc = [x + y for x, y in zip(acc, t)]
        out[a] = acc
    return out, merged_magnitude(clusters, fix, poses)


def merged_magnitude(clusters, fix, poses):
    cl = np.abs(np.asarray(clusters, dtype=np.float64)).copy()
    cl[cl[:, :, 9] == 0] = 0.0                     # a frame is skipped on N alone, whatever its moments hold
    po = np.abs(np.asarray(poses, dtype=np.float64)).reshape(-1, 12)
    R = np.transpose(po[:, :9].reshape(-1, 3, 3), (0, 2, 1)); p = po[:, 9:]
    P = cl[..., [[0, 1, 2], [1, 3, 4], [2, 4, 5]]]; v = cl[..., 6:9]; n = cl[..., 9]
    Rv = np.einsum("irc,aic->air", R, v)
    PP = np.einsum("irk,aikl,icl->airc", R, P, R) + Rv[..., :, None] * p[None, :, None, :] + p[None, :, :, None] * Rv[..., None, :] \
        + n[..., None, None] * p[None, :, :, None] * p[None, :, None, :]
    M = np.abs(np.asarray(fix, dtype=np.float64)).copy()
    M[:, :6] += PP.sum(axis=1)[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    M[:, 6:9] += (Rv + n[..., None] * p[None]).sum(axis=1)
    M[:, 9] += n.sum(axis=1)
    return M


@_hp
def covariance_exact(merged_row):
    """C = P/N - vbar vbar^T and the scale s = max|P/N| + |vbar|^2 of one merged row."""
    m = _vec(merged_row)
    N = m[9]
    vb = [x / N for x in m[6:9]]
    P = _sym(m[:6])
    Cm = [[P[r][c] / N - vb[r] * vb[c] for c in range(3)] for r in range(3)]
    s = max(abs(P[r][c] / N) for r in range(3) for c in range(3)) + _dot(vb, vb)
    return Cm, s


@_hp
def eig_exact(Cm):
    """Ascending eigenvalues and eigenvectors (columns; largest component of each positive) of a 3 x 3 symmetric matrix of mpf."""
    E, Q = mp.eigsy(mp.matrix(Cm))
    order = sorted(range(3), key=lambda k: E[k])
    lam = [E[k] for k in order]
    Uc = []
    for k in order:
        col = [Q[r, k] for r in range(3)]
        big = max(col, key=abs)
        Uc.append([x if big > 0 else -x for x in col])
    return lam, Uc            # Uc[k] = u_k


@_hp
def eig_residuals(merged, eigval, eigvec):
    """Backward-error quantities of a claimed decomposition of one float64 merged row (nothing here depends on an eigenvalue gap):
    dict(res = ||C u_k - lambda_k u_k||_inf for k = 0, 1, 2, orth = ||U^T U - I||_max, dlam = |lambda_k - exact lambda_k|, s), floats."""
    Cm, s = covariance_exact(merged)
    lam = _vec(eigval); q = _vec(eigvec)
    u = [q[3 * k: 3 * k + 3] for k in range(3)]
    res = [max(abs(x - lam[k] * y) for x, y in zip(_matvec(Cm, u[k]), u[k])) for k in range(3)]
    orth = max(abs(_dot(u[i], u[j]) - (1 if i == j else 0)) for i in range(3) for j in range(3))
    exact = sorted(mp.eigsy(mp.matrix(Cm), eigvals_only=True))
    return dict(res=[float(x) for x in res], orth=float(orth), dlam=[float(abs(lam[k] - exact[k])) for k in range(3)], s=float(s))


@_hp
def exact_cache(clusters, fix, poses, as_float=True):
    """(eigval (V, 3), eigvec (V, 9), merged (V, 10)): the exact decomposition of the exact merged cluster, rounded to float64 (as_float) or
    left as mpf.  A voxel without any point gets zeros and the identity."""
    merged, _ = merged_exact(clusters, fix, poses)
    V = merged.shape[0]
    ev = np.empty((V, 3), dtype=object); U = np.empty((V, 9), dtype=object)
    for a in range(V):
        if merged[a, 9] == 0:
            ev[a] = [mpf(0)] * 3; U[a] = _vec(np.eye(3).reshape(9)); continue
        lam, Uc = eig_exact(covariance_exact(merged[a])[0])
        ev[a] = lam; U[a] = Uc[0] + Uc[1] + Uc[2]
    if as_float:
        return ev.astype(np.float64), U.astype(np.float64), merged.astype(np.float64)
    return ev, U, merged


@_hp
def split_hi_lo(ex):
    """An array of mpf as two float64 arrays hi + lo."""
    hi = ex.astype(np.float64)
    return hi, (ex - hi.astype(object)).astype(np.float64)


def _split(x):
    """An mpf as hi + lo in float64."""
    hi = float(x)
    return hi, float(x - mpf(hi))


@_hp
def hessian_exact(clusters, coe, poses, eigval, eigvec, merged, head=0, end=None, raw=False):
    """H, J and r of acc_evaluate2 over the voxels [head, end) from the GIVEN cache (the sweep never recomputes the decomposition), and the
    magnitudes: dict(H, H_lo, J, J_lo, r, r_lo, r_mag, M_H, M_J, M_RR, S_RR; hessian_magnitude).  H + H_lo is the exact value to ~2^-106; err(X) = |(X - H) - H_lo| in float64.
    raw: also H_mp, J_mp, arrays of mpf at the working precision (the cache may then be given as mpf too)."""
    clusters = np.asarray(clusters)
    V, W = clusters.shape[:2]
    end = V if end is None else end
    n = 6 * W
    Rp = [_rot(poses[i]) for i in range(W)]
    blocks, Jac = {}, {}
    r_sum, r_mag = mpf(0), mpf(0)
    two, half = mpf(2), mpf(1) / 2
    for a in range(head, end):
        lam = _vec(eigval[a]); q = _vec(eigvec[a]); mg = _vec(merged[a]); ca = _m(coe[a])
        r_sum += ca * lam[0]; r_mag += abs(ca * lam[0])
        obs = [i for i in range(W) if clusters[a, i, 9] != 0]
        if not obs:
            continue
        u, u1, u2 = q[0:3], q[3:6], q[6:9]
        N = mg[9]
        vbar = [x / N for x in mg[6:9]]
        s1, s2, sz = ca * two / (lam[1] - lam[0]), ca * two / (lam[2] - lam[0]), ca * two / (N * N)
        rows = {}
        for i in obs:
            cl = _vec(clusters[a, i]); P, v, ni = _sym(cl[:6]), cl[6:9], cl[9]
            R, p = Rp[i]
            r = _matTvec(R, u)
            t = [p[k] - vbar[k] for k in range(3)]
            ut = _dot(u, t)
            hv, hr = _hat(v), _hat(r)
            w = _matvec(hv, r)
            hPr = _hat(_matvec(P, r))
            c1 = [[hPr[x][y] + hv[x][y] * ut for y in range(3)] for x in range(3)]
            Rv = _matvec(R, v)
            c2 = [Rv[k] + ni * t[k] for k in range(3)]
            RP = _matmul(R, P)
            left = _matmul([[RP[x][y] + t[x] * v[y] for y in range(3)] for x in range(3)], hr)
            Rc1 = _matmul(R, c1)
            c2u = _dot(c2, u)
            A = [[(left[x][y] - Rc1[x][y]) / N for y in range(3)] + [(c2[x] * u[y] + (c2u if x == y else 0)) / N for y in range(3)] for x in range(3)]
            g = [A[0][c] * u[0] + A[1][c] * u[1] + A[2][c] * u[2] for c in range(6)]
            g1 = [A[0][c] * u1[0] + A[1][c] * u1[1] + A[2][c] * u1[2] for c in range(6)]
            g2 = [A[0][c] * u2[0] + A[1][c] * u2[1] + A[2][c] * u2[2] for c in range(6)]
            z = w + [ni * x for x in u]
            rows[i] = (g1, g2, z, [s1 * x for x in g1], [s2 * x for x in g2], [sz * x for x in z])
            Ji = Jac.setdefault(i, [mpf(0)] * 6)
            for c in range(6):
                Ji[c] += ca * g[c]
            # D_i (A.4)
            hrP = _matmul(hr, P)
            Drr = _matmul([[c1[x][y] - hrP[x][y] for y in range(3)] for x in range(3)], hr)
            hg = _hat(g[0:3])
            B = blocks.setdefault((i, i), [mpf(0)] * 36)
            k2N = ca * two / N
            for x in range(3):
                for y in range(3):
                    B[6 * x + y] += k2N * Drr[x][y] - ca * half * hg[x][y]
                    d = k2N * w[x] * u[y]
                    B[6 * x + 3 + y] += d
                    B[6 * (3 + y) + x] += d
                    B[6 * (3 + x) + 3 + y] += k2N * ni * u[x] * u[y]
        for ii, i in enumerate(obs):
            _, _, _, a1, a2, a3 = rows[i]
            for j in obs[ii:]:
                g1j, g2j, zj = rows[j][:3]
                B = blocks.setdefault((i, j), [mpf(0)] * 36)
                for x in range(6):
                    ax1, ax2, ax3 = a1[x], a2[x], a3[x]
                    o = 6 * x
                    for y in range(6):
                        B[o + y] -= ax1 * g1j[y] + ax2 * g2j[y] + ax3 * zj[y]
    H = np.zeros((n, n)); Hlo = np.zeros((n, n)); J = np.zeros(n); Jlo = np.zeros(n)
    for (i, j), B in blocks.items():
        for x in range(6):
            for y in range(6):
                hi, lo = _split(B[6 * x + y])
                H[6 * i + x, 6 * j + y] = hi; Hlo[6 * i + x, 6 * j + y] = lo
                if i != j:
                    H[6 * j + y, 6 * i + x] = hi; Hlo[6 * j + y, 6 * i + x] = lo
    for i, Ji in Jac.items():
        for c in range(6):
            J[6 * i + c], Jlo[6 * i + c] = _split(Ji[c])
    M_H, M_J, M_RR, S_RR = hessian_magnitude(clusters, coe, poses, eigval, eigvec, merged, head, end)
    extra = {}
    if raw:
        Hm = np.full((n, n), mpf(0), dtype=object); Jm = np.full(n, mpf(0), dtype=object)
        for (i, j), B in blocks.items():
            for x in range(6):
                for y in range(6):
                    Hm[6 * i + x, 6 * j + y] = Hm[6 * j + y, 6 * i + x] = B[6 * x + y]
        for i, Ji in Jac.items():
            Jm[6 * i: 6 * i + 6] = Ji
        extra = dict(H_mp=Hm, J_mp=Jm)
    return dict(**extra, H=H, H_lo=Hlo, J=J, J_lo=Jlo, r=float(r_sum), r_lo=float(r_sum - mpf(float(r_sum))), r_mag=float(r_mag), M_H=M_H, M_J=M_J, M_RR=M_RR, S_RR=S_RR)


def _hatnp(v, signed):
    """hat(v) of (..., 3) vectors, or |hat(v)| of non-negative ones."""
    z = np.zeros_like(v[..., 0])
    m = -1.0 if signed else 1.0
    return np.stack([np.stack([z, m * v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, m * v[..., 0]], -1), np.stack([m * v[..., 1], v[..., 0], z], -1)], -2)


def _np_terms(clusters, coe, poses, eigval, eigvec, merged, head, end, signed):
    """The per-voxel pieces of A.4 in float64 over the voxels [head, end): the values (signed) or their magnitudes (every input replaced by
    its absolute value, every subtraction by an addition)."""
    f = (lambda x: np.asarray(x).astype(np.float64)) if signed else (lambda x: np.abs(np.asarray(x).astype(np.float64)))
    m = -1.0 if signed else 1.0
    V, W = np.asarray(clusters).shape[:2]
    sl = slice(head, end)
    n = 6 * W
    cl = f(clusters)[sl].copy(); cl[cl[:, :, 9] == 0] = 0.0          # a frame is skipped on N alone, whatever its moments hold
    obs = cl[:, :, 9] != 0
    lam = np.asarray(eigval).astype(np.float64)[sl]; q = f(eigvec)[sl]; mg = f(merged)[sl]; ca = f(coe)[sl]
    po = f(poses).reshape(-1, 12)
    R = np.transpose(po[:, :9].reshape(-1, 3, 3), (0, 2, 1)); p = po[:, 9:]
    u, u1, u2 = q[:, 0:3], q[:, 3:6], q[:, 6:9]
    N = np.where(mg[:, 9] == 0, 1.0, mg[:, 9])
    vbar = mg[:, 6:9] / N[:, None]
    live = obs.any(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s1 = np.where(live, np.abs(2.0 / (lam[:, 1] - lam[:, 0])), 0.0); s2 = np.where(live, np.abs(2.0 / (lam[:, 2] - lam[:, 0])), 0.0)
    P = cl[..., [[0, 1, 2], [1, 3, 4], [2, 4, 5]]]; v = cl[..., 6:9]; ni = cl[..., 9]
    r = np.einsum("ikc,ak->aic", R, u)                                  # R^T u
    t = p[None] + m * vbar[:, None]
    ut = np.einsum("ak,aik->ai", u, t)
    hv, hr = _hatnp(v, signed), _hatnp(r, signed)
    w = np.einsum("aixy,aiy->aix", hv, r)
    Pr = np.einsum("aixy,aiy->aix", P, r)
    c1 = _hatnp(Pr, signed) + hv * ut[..., None, None]
    c2 = np.einsum("ixy,aiy->aix", R, v) + ni[..., None] * t
    left = np.einsum("aixk,aiky->aixy", np.einsum("ixk,aiky->aixy", R, P) + t[..., :, None] * v[..., None, :], hr) + m * np.einsum("ixk,aiky->aixy", R, c1)
    right = c2[..., :, None] * u[:, None, None, :] + np.einsum("aik,ak->ai", c2, u)[..., None, None] * np.eye(3)
    A = np.concatenate([left, right], axis=-1) / N[:, None, None, None] * obs[..., None, None]           # (a, i, 3, 6)
    g = np.einsum("aikc,ak->aic", A, u); g1 = np.einsum("aikc,ak->aic", A, u1); g2 = np.einsum("aikc,ak->aic", A, u2)
    z = np.concatenate([w, ni[..., None] * u[:, None, :]], axis=-1) * obs[..., None]
    nv = end - head
    k2N = (ca * 2.0 / N)[:, None, None, None]
    Drr = k2N * np.einsum("aixk,aiky->aixy", c1 + m * np.einsum("aixk,aiky->aixy", hr, P), hr) + m * 0.5 * ca[:, None, None, None] * _hatnp(g[..., 0:3], signed)
    Drt = k2N * w[..., :, None] * u[:, None, None, :]
    Dtt = k2N * ni[..., None, None] * u[:, None, :, None] * u[:, None, None, :]
    D = np.concatenate([np.concatenate([Drr, Drt], -1), np.concatenate([np.swapaxes(Drt, -1, -2), Dtt], -1)], -2) * obs[..., None, None]
    return dict(G1=g1.reshape(nv, n), G2=g2.reshape(nv, n), Z=z.reshape(nv, n), g=g, D=D, w1=ca * s1, w2=ca * s2, wz=ca * 2.0 / (N * N), ca=ca, k2N=k2N, obs=obs,
                P=P, r=r, v=v, ut=ut, Pr=Pr)


def hessian_magnitude(clusters, coe, poses, eigval, eigvec, merged, head=0, end=None):
    """(M_H (6W, 6W), M_J (6W), M_RR, S_RR) of the voxels [head, end).  M_H, M_J: module docstring.  M_RR, zero outside the rotation-rotation
    part of the diagonal blocks: the magnitude of the CLOSED FORM of D_rr (module docstring) summed over the voxels; S_RR, same support: the
    sum over the voxels of |D_rr|, the values (float64), which is what adding the voxels' D_rr in any order can lose per unit of u."""
    V, W = np.asarray(clusters).shape[:2]
    end = V if end is None else end
    n = 6 * W
    if end <= head:
        return np.zeros((n, n)), np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    T = _np_terms(clusters, coe, poses, eigval, eigvec, merged, head, end, signed=False)
    M = np.einsum("a,ax,ay->xy", T["w1"], T["G1"], T["G1"]) + np.einsum("a,ax,ay->xy", T["w2"], T["G2"], T["G2"]) + np.einsum("a,ax,ay->xy", T["wz"], T["Z"], T["Z"])
    Ds = T["D"].sum(axis=0)
    # the closed form of the symmetric rotation-rotation block (module docstring): its own magnitude
    P, r, v, ut, Pr = T["P"], T["r"], T["v"], T["ut"], T["Pr"]
    zm = Pr + ut[..., None] * v
    rr = np.einsum("aix,aix->ai", r, r)[..., None, None]
    trP = (P[..., 0, 0] + P[..., 1, 1] + P[..., 2, 2])[..., None, None]
    outer = lambda x, y: x[..., :, None] * y[..., None, :]
    I3 = np.eye(3)
    Dc = 0.5 * (outer(r, zm) + outer(zm, r)) + np.einsum("aix,aix->ai", zm, r)[..., None, None] * I3 + rr * (trP * I3 + P) + trP * outer(r, r) \
        + outer(Pr, r) + outer(r, Pr) + np.einsum("aix,aix->ai", r, Pr)[..., None, None] * I3
    Dcs = (T["k2N"] * Dc * T["obs"][..., None, None]).sum(axis=0)
    M_RR = np.zeros((n, n))
    for i in range(W):
        M[6 * i: 6 * i + 6, 6 * i: 6 * i + 6] += Ds[i]
        M_RR[6 * i: 6 * i + 3, 6 * i: 6 * i + 3] = Dcs[i]
    M_J = (T["ca"][:, None, None] * T["g"]).sum(axis=0).reshape(n)
    X = _np_terms(clusters, coe, poses, eigval, eigvec, merged, head, end, signed=True)
    Dabs = np.abs(X["D"]).sum(axis=0)
    S_RR = np.zeros((n, n))
    for i in range(W):
        S_RR[6 * i: 6 * i + 3, 6 * i: 6 * i + 3] = Dabs[i, :3, :3]
    return M, M_J, M_RR, S_RR


def err_units(X, hi, lo, M, u=U64):
    """|X - exact| / (u * M) element by element (0 where M == 0 and X == 0, inf where M == 0 and X != 0)."""
    e = np.abs((np.asarray(X) - hi) - lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = e / (u * M)
    k[(M == 0) & (e == 0)] = 0.0
    k[(M == 0) & (e != 0)] = np.inf
    return k
