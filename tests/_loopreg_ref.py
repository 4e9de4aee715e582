"""Numpy model of the loop-edge registration (include/vxba.h: vxba_loopreg_*): the CHECKER of tests/test_gpu_loopreg.py and of
tests/test_loopreg_cpu.py, never the thing run.

Three consumers of one association -- plane cloud extraction (STDescManager::init_voxel_map / BTCOctoTree::init_plane, BTC.cpp:96-139,
279-338), the verify score (plane_geometric_verify, BTC.cpp:1422-1479) and icp_normal (loop_refine.hpp:47-145) -- written so that every
quantity a decision rests on is formed by the same sequence of roundings as csrc/vxba_loopreg_math.hpp forms it: float32 distances by
numpy float32 operations (no contraction) and a brute-force first-minimum ``argmin``; float64 transforms and gate quantities as explicit
elementwise expressions, never through a matrix product whose summation order belongs to a BLAS.

BTC.cpp itself cannot be compiled in the test environment (visualization_msgs, <execution>, Eigen::EigenSolver), so extraction and score are
pinned to this model and ``numpy.linalg.eigh``; the ICP is pinned to the reference's own icp_normal through tests/golden/loop_icp.
"""
import numpy as np

GATES0 = (0.2, 0.2, 0.5, 3.0)
GATES1 = (0.1, 0.1, 0.1, 1.0)
DEFAULTS = dict(max_iter=20, gates0=GATES0, gates1=GATES1, step_tol=1e-3, icp_eigval=14.0)
PLANE_DEFAULTS = dict(voxel_size=1.0, voxel_init_num=10, plane_detection_thre=0.01)


# ---- plane cloud ---------------------------------------------------------------------------------------------------------------
def voxel_coords(xyz, voxel_size):
    """BTC.cpp:287-295: divide, subtract 1.0 where negative, truncate."""
    loc = np.asarray(xyz, dtype=np.float64) / voxel_size
    loc = np.where(loc < 0, loc - 1.0, loc)
    return np.trunc(loc).astype(np.int64)


def plane_cloud(xyz, voxel_size=1.0, voxel_init_num=10, plane_detection_thre=0.01):
    """Returns dict(rows (n, 6) float32 in ascending (x, y, z) voxel order with the largest-magnitude normal component positive, coords (n, 3),
    lam (n, 3) ascending eigenvalues of the plane voxels, lam_min_all: the smallest eigenvalue of EVERY voxel with N > voxel_init_num)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    empty = dict(rows=np.zeros((0, 6), np.float32), coords=np.zeros((0, 3), np.int64), lam=np.zeros((0, 3)), lam_min_all=np.zeros(0))
    if xyz.shape[0] == 0:
        return empty
    vc = voxel_coords(xyz, voxel_size)
    order = np.lexsort((vc[:, 2], vc[:, 1], vc[:, 0]))            # stable: input order inside a voxel
    vs, ps = vc[order], xyz[order]
    head = np.concatenate([[True], np.any(vs[1:] != vs[:-1], axis=1)])
    start = np.nonzero(head)[0]
    N = np.diff(np.concatenate([start, [xyz.shape[0]]]))
    x, y, z = ps[:, 0], ps[:, 1], ps[:, 2]
    mom = np.stack([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z], axis=1)
    sums = np.add.reduceat(mom, start, axis=0)
    keep = N > voxel_init_num
    if not keep.any():
        return empty
    sums, Nk, coords = sums[keep], N[keep].astype(np.float64), vs[start][keep]
    c = sums[:, 6:9] / Nk[:, None]
    C6 = sums[:, :6] / Nk[:, None] - np.stack([c[:, 0] * c[:, 0], c[:, 0] * c[:, 1], c[:, 0] * c[:, 2], c[:, 1] * c[:, 1], c[:, 1] * c[:, 2], c[:, 2] * c[:, 2]], axis=1)
    M = np.zeros((c.shape[0], 3, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = C6.T
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    lam, vec = np.linalg.eigh(M)
    is_plane = lam[:, 0] < plane_detection_thre
    n = vec[is_plane][:, :, 0]
    lead = n[np.arange(n.shape[0]), np.argmax(np.abs(n), axis=1)]
    n = n * np.where(lead < 0, -1.0, 1.0)[:, None]
    rows = np.concatenate([c[is_plane], n], axis=1).astype(np.float32)
    return dict(rows=rows, coords=coords[is_plane], lam=lam[is_plane], lam_min_all=lam[:, 0])


# ---- association ---------------------------------------------------------------------------------------------------------------
def transform(pose, src):
    """p = R p_s + t and n = R n_s in float64 from the float32 fields, each component ((R0 x + R1 y) + R2 z) + t (pose: [R column-major 9 | t 3])."""
    P = np.asarray(pose, dtype=np.float64).reshape(12)
    s = np.asarray(src, dtype=np.float32).reshape(-1, 6).astype(np.float64)
    p = np.stack([((P[r] * s[:, 0] + P[3 + r] * s[:, 1]) + P[6 + r] * s[:, 2]) + P[9 + r] for r in range(3)], axis=1)
    n = np.stack([(P[r] * s[:, 3] + P[3 + r] * s[:, 4]) + P[6 + r] * s[:, 5] for r in range(3)], axis=1)
    return p, n


def nearest(q, tar, chunk=512):
    """Brute force in float32: d = (dx dx + dy dy) + dz dz, first minimum.  Returns (index (S,), exact ties (S,) bool: another target at the same
    float32 distance as the nearest)."""
    q = np.asarray(q, dtype=np.float32); t = np.asarray(tar, dtype=np.float32)[:, :3]
    S = q.shape[0]
    nn = np.zeros(S, dtype=np.int32); tie = np.zeros(S, dtype=bool)
    if t.shape[0] == 0:
        nn[:] = -1
        return nn, tie
    tx, ty, tz = t[:, 0][None, :], t[:, 1][None, :], t[:, 2][None, :]
    for s0 in range(0, S, chunk):
        qq = q[s0:s0 + chunk]
        dx = tx - qq[:, 0:1]; dy = ty - qq[:, 1:2]; dz = tz - qq[:, 2:3]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        k = np.argmin(d, axis=1)
        nn[s0:s0 + chunk] = k
        tie[s0:s0 + chunk] = (d == d[np.arange(d.shape[0]), k][:, None]).sum(axis=1) > 1
    return nn, tie


def gate_quantities(p, n, tar, nn):
    t = np.asarray(tar, dtype=np.float32).reshape(-1, 6).astype(np.float64)[nn]
    tp, tn = t[:, :3], t[:, 3:]
    d = p - tp
    i, a = n - tn, n + tn
    inc = np.sqrt((i[:, 0] * i[:, 0] + i[:, 1] * i[:, 1]) + i[:, 2] * i[:, 2])
    add = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    rr = (tn[:, 0] * d[:, 0] + tn[:, 1] * d[:, 1]) + tn[:, 2] * d[:, 2]
    pp = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return inc, add, rr, pp, tn


def verdict_margin(inc, add, rr, pp, g):
    """Per point: (verdict, the smallest change of any gate quantity that flips it).  The verdict is (A or B) and C and D; a true one flips when C or D
    does, or when every true one of A, B does; a false one flips only when every false term has turned."""
    mA, mB, mC, mD = np.abs(inc - g[0]), np.abs(add - g[1]), np.abs(np.abs(rr) - g[2]), np.abs(pp - g[3])
    A, B, Cc, D = inc < g[0], add < g[1], np.abs(rr) < g[2], pp < g[3]
    ok = (A | B) & Cc & D
    ab_true = np.where(A & B, np.maximum(mA, mB), np.where(A, mA, mB))
    m_true = np.minimum(np.minimum(mC, mD), ab_true)
    m_false = np.maximum.reduce([np.where(A | B, 0.0, np.minimum(mA, mB)), np.where(Cc, 0.0, mC), np.where(D, 0.0, mD)])
    return ok, np.where(ok, m_true, m_false)


def associate(src, tar, pose, gates):
    """dict(nn, matched, ties, margin: smallest verdict margin, raw: the smallest |quantity - threshold| per gate quantity, and the quantities)."""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 6); tar = np.asarray(tar, dtype=np.float32).reshape(-1, 6)
    g = np.asarray(gates, dtype=np.float64)
    S = src.shape[0]
    p, n = transform(pose, src)
    nn, tie = nearest(p.astype(np.float32), tar)
    if S == 0 or tar.shape[0] == 0:
        return dict(nn=nn, matched=np.zeros(S, bool), ties=0, margin=np.inf, raw=np.full(4, np.inf), p=p, n=n, rr=np.zeros(S), tn=np.zeros((S, 3)))
    inc, add, rr, pp, tn = gate_quantities(p, n, tar, nn)
    ok, m = verdict_margin(inc, add, rr, pp, g)
    raw = np.array([np.abs(inc - g[0]).min(), np.abs(add - g[1]).min(), np.abs(np.abs(rr) - g[2]).min(), np.abs(pp - g[3]).min()])
    return dict(nn=nn, matched=ok, ties=int(tie.sum()), margin=float(m.min()), raw=raw, p=p, n=n, rr=rr, tn=tn)


def score(src, tar, pose, normal_threshold, dis_threshold):
    a = associate(src, tar, pose, (normal_threshold, normal_threshold, dis_threshold, np.inf))
    useful = int(a["matched"].sum())
    S = np.asarray(src).reshape(-1, 6).shape[0]
    return dict(useful=useful, score=useful / S if S else 0.0, margin=a["margin"], ties=a["ties"])


# ---- ICP -----------------------------------------------------------------------------------------------------------------------
def so3_exp(w):
    """tools.hpp:51-66."""
    w = np.asarray(w, dtype=np.float64)
    a = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if not a >= 1e-11:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (np.outer(k, k) - np.eye(3))


def retract(pose, dx):
    P = np.asarray(pose, dtype=np.float64).reshape(12)
    R = P[:9].reshape(3, 3).T @ so3_exp(dx[:3])
    return np.concatenate([R.T.reshape(9), P[9:] + dx[3:]])


def jac_rows(pose, src, tn):
    P = np.asarray(pose, dtype=np.float64).reshape(12)
    pl = np.asarray(src, dtype=np.float32).reshape(-1, 6)[:, :3].astype(np.float64)
    u = np.stack([(P[3 * c] * tn[:, 0] + P[3 * c + 1] * tn[:, 1]) + P[3 * c + 2] * tn[:, 2] for c in range(3)], axis=1)      # R^T n_t
    return np.concatenate([np.cross(pl, u), tn], axis=1)


def advance(st, match_num, dx, step_tol, max_iter):
    """The state machine after the sums of one iteration (vxlr::icp_advance).  st: dict(iter, done, is_converge, failed).  Returns True when the
    step is to be applied."""
    st["iter"] += 1
    if match_num < 6 or not np.all(np.isfinite(dx)):
        st.update(done=1, failed=1, is_converge=0)
        return False
    nr, nt = np.linalg.norm(dx[:3]), np.linalg.norm(dx[3:])
    small = nr < step_tol and nt < step_tol
    was = st["is_converge"]
    if (small and was) or st["iter"] >= max_iter:
        st["done"] = 1
    st["is_converge"] = 1 if small else was
    return True


def icp(src, tar, pose, max_iter=20, gates0=GATES0, gates1=GATES1, step_tol=1e-3, icp_eigval=14.0):
    """icp_normal with the library's rules where the reference is undefined.  Returns dict(pose, accept, is_converge, iterations, match_num, eig,
    resi, failed, trace (one dict per iteration), margin (smallest verdict margin over points and iterations), raw (4,), step_margin (smallest
    |step norm - step_tol|), ties)."""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 6); tar = np.asarray(tar, dtype=np.float32).reshape(-1, 6)
    P = np.array(pose, dtype=np.float64).reshape(12)
    st = dict(iter=0, done=0, is_converge=0, failed=0)
    trace = []
    margin, step_margin, ties, raw = np.inf, np.inf, 0, np.full(4, np.inf)
    norm = np.zeros((3, 3)); resi = 0.0; match = 0
    while not st["done"]:
        g = gates1 if st["is_converge"] else gates0
        a = associate(src, tar, P, g)
        margin = min(margin, a["margin"]); ties += a["ties"]; raw = np.minimum(raw, a["raw"])
        m = a["matched"]
        match = int(m.sum())
        J = jac_rows(P, src[m], a["tn"][m]); rr = a["rr"][m]; tn = a["tn"][m]
        H = J.T @ J; JT = J.T @ rr
        resi = float(0.5 * (rr * rr).sum()); norm = tn.T @ tn
        dx = np.full(6, np.nan)
        if match >= 6:
            try:
                with np.errstate(all="ignore"):
                    dx = np.linalg.solve(H, -JT)
            except np.linalg.LinAlgError:
                pass
        apply = advance(st, match, dx, step_tol, max_iter)
        if apply:
            nr, nt = np.linalg.norm(dx[:3]), np.linalg.norm(dx[3:])
            step_margin = min(step_margin, abs(nr - step_tol), abs(nt - step_tol))
            P = retract(P, dx)
        trace.append(dict(match_num=match, resi=resi, dx=dx.copy(), pose=P.copy(), is_converge=st["is_converge"], nn=a["nn"], matched=m))
    eig = np.linalg.eigvalsh(norm)
    accept = bool(eig[0] > icp_eigval and st["is_converge"] == 1 and not st["failed"])
    return dict(pose=P, accept=accept, is_converge=int(st["is_converge"]), iterations=st["iter"], match_num=match, eig=eig, resi=resi, failed=int(st["failed"]),
                trace=trace, margin=margin, raw=raw, step_margin=step_margin, ties=ties, eig_margin=abs(float(eig[0]) - icp_eigval))


# ---- helpers of the tests --------------------------------------------------------------------------------------------------------
def pose_of(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64).T.reshape(9), np.asarray(t, dtype=np.float64).reshape(3)])


def pose_diff(a, b):
    """(translation difference [m], rotation angle between [rad]) of two pose records."""
    a = np.asarray(a, dtype=np.float64).reshape(12); b = np.asarray(b, dtype=np.float64).reshape(12)
    Ra, Rb = a[:9].reshape(3, 3).T, b[:9].reshape(3, 3).T
    E = Ra.T @ Rb
    k = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.linalg.norm(a[9:] - b[9:])), float(np.arctan2(np.linalg.norm(k), 0.5 * (np.trace(E) - 1.0)))
