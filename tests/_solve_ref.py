"""Exact arithmetic for the damped LM solves (tests/test_solve_cpu.py, tests/test_gpu_solve.py, scripts/run_solve_accuracy.py).

The system of one LM step (Lidar_BA_Optimizer::damping_iter, voxel_map.hpp:397-410) is (H + u diag(H))[6:, 6:] x = -J[6:] -- frame 0 is the
gauge -- and in the LiDAR-inertial shells (H + u diag(H) + E)[6:, 6:] x = (e - J)[6:].  Everything here takes the float64 inputs as exact
numbers: the matrix is formed in mpmath (60 digits), solved by LU with partial pivoting, and q1 / the trial poses are evaluated in mpmath at
whatever dxi they are asked about.  The normwise backward error uses a numpy.longdouble residual (80-bit: eps 1.08e-19), which is enough for
errors of the order of 2^-53 and costs nothing at n = 768, where mpmath would take minutes.
"""
import mpmath as mp
import numpy as np

DPS = 60
U53 = 2.0 ** -53          # unit round-off of float64


def system(H, J, u, E=None, e=None, dead=()):
    """float64 (A, b) of the damped, gauge-fixed system over the live rows, and the index of those rows.  dead: frames whose rows and columns
    are left out (empty frames).  The float64 A carries one rounding per diagonal entry; eta() works on the longdouble version."""
    n = H.shape[0]
    keep = np.ones(n, bool)
    keep[:6] = False
    for f in dead:
        keep[6 * f:6 * f + 6] = False
    idx = np.flatnonzero(keep)
    A = np.array(H, dtype=np.longdouble)
    A[np.diag_indices(n)] += np.longdouble(u) * np.diag(H).astype(np.longdouble)
    b = -np.asarray(J, dtype=np.longdouble)
    if E is not None:
        A = A + np.asarray(E, dtype=np.longdouble)
        b = b + np.asarray(e, dtype=np.longdouble)
    return A[np.ix_(idx, idx)], b[idx], idx


def eta(A, b, x):
    """Normwise backward error ||b - A x||_2 / (||A||_2 ||x||_2 + ||b||_2) with the residual in longdouble.  A, b: from system()."""
    A = np.asarray(A, dtype=np.longdouble)
    b = np.asarray(b, dtype=np.longdouble)
    xl = np.asarray(x, dtype=np.longdouble)
    if A.shape[0] == 0:
        return 0.0
    # one common power of two takes the block-scaled systems (1e+-140) away from the ends of the exponent range; eta does not change
    sc = np.longdouble(2.0) ** -int(np.floor(np.log2(float(np.abs(A).max()) or 1.0)))
    A, b = A * sc, b * sc
    r = b - A @ xl
    den = np.longdouble(np.linalg.norm(A.astype(np.float64), 2)) * np.sqrt(xl @ xl) + np.sqrt(b @ b)
    if den == 0:
        return 0.0 if not np.any(r) else np.inf
    return float(np.sqrt(r @ r) / den)


def exact_solve(A, b):
    """x of A x = b with A, b taken as exact (longdouble or float64 entries are converted digit for digit).  Returns (float64 x, mp vector)."""
    n = A.shape[0]
    if n == 0:
        return np.zeros(0), mp.matrix(0, 1)
    with mp.workdps(DPS):
        Am = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                Am[i, j] = _mpf(A[i, j])
        bm = mp.matrix([_mpf(v) for v in b])
        xm = mp.lu_solve(Am, bm)
        return np.array([float(v) for v in xm]), xm


def _mpf(v):
    """mpf of a float64 / longdouble without loss (a longdouble is split into two float64 pieces)."""
    v = np.longdouble(v)
    hi = np.float64(v)
    lo = np.float64(v - np.longdouble(hi))
    return mp.mpf(float(hi)) + mp.mpf(float(lo))


def forward_error(x, xm):
    """||x - x_exact||_2 and ||x_exact||_2 in mpmath, as floats."""
    with mp.workdps(DPS):
        d = mp.sqrt(sum((mp.mpf(float(a)) - b) ** 2 for a, b in zip(x, xm)))
        return float(d), float(mp.sqrt(sum(b ** 2 for b in xm)))


def exact_q1(H, J, u, dxi):
    """0.5 dxi . (u D dxi - J), D = diag(H), at the given float64 dxi (voxel_map.hpp:410).  Returns (float value, float sum of |terms|)."""
    with mp.workdps(DPS):
        tot, mag = mp.mpf(0), mp.mpf(0)
        for i in range(6, H.shape[0]):
            x = mp.mpf(float(dxi[i]))
            t1 = mp.mpf(float(u)) * mp.mpf(float(H[i, i])) * x * x
            t2 = mp.mpf(float(J[i])) * x
            tot += t1 - t2
            mag += abs(t1) + abs(t2)
        return float(tot / 2), float(mag / 2)


def exact_trial_poses(Rp, dxi):
    """Rp (W, 12): R column-major | p.  The trial poses R Exp(dphi), p + dp with the exponential in mpmath.  Returns (W, 12) of mp numbers
    (rotation part) as a list of lists, and the float64 translations x + dxi (a single float64 addition is what every solver does)."""
    W = Rp.shape[0]
    rots = []
    with mp.workdps(DPS):
        for j in range(W):
            w = [mp.mpf(float(v)) for v in dxi[6 * j:6 * j + 3]]
            th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
            Em = mp.eye(3)
            if th != 0:
                K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
                Em = Em + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)
            R = mp.matrix(3, 3)
            for r in range(3):
                for c in range(3):
                    R[r, c] = mp.mpf(float(Rp[j, 3 * c + r]))
            RE = R * Em
            rots.append([RE[q % 3, q // 3] for q in range(9)])      # column-major
    trans = Rp[:, 9:12] + np.asarray(dxi).reshape(W, 6)[:, 3:6]
    return rots, trans


def rotation_error(xt, rots):
    """max |xt[j, 0:9] - exact| over all frames."""
    with mp.workdps(DPS):
        return max(float(abs(mp.mpf(float(xt[j, q])) - rots[j][q])) for j in range(len(rots)) for q in range(9))
