"""The checker of the pose-graph optimiser (vxba_pgo_*, voxel_slam_amd.vxba.PoseGraph): plain numpy, f64.

* residuals and analytic Jacobians of the two factor kinds (include/vxba.h), batched over factors;
* ``dense_lm``: Levenberg-Marquardt with the library's damping schedule (lm_decide) around a dense Cholesky solve of
  (H + u diag H) dx = -g -- the optimum the GPU result is held against;
* ``CgModel``: an executable model of the device's block-Jacobi CG (csrc/vxba_pgo.hip pgo_solve_kernel) with its summation structure --
  per-node gathers in CSR order, dot products as per-lane partials over the 80 node slots, an xor butterfly inside each 64-lane wave and
  the 8 wave sums added in order -- in the tradition of test_solve4_model.py.  It predicts iteration counts; fused multiply-adds keep
  it from being bit-identical to the kernel.

Layouts as in the ABI: pose records [R column-major 9 | p 3]; factor records [Zr row-major 9 | zt 3]; tangent [dphi; dp], R <- R Exp(dphi)."""
import numpy as np

DEFAULT_U0 = 1e-6


# ---- SO(3), batched over the leading axis ------------------------------------------------------------------------------------
def hat(w):
    w = np.asarray(w, dtype=np.float64)
    H = np.zeros(w.shape[:-1] + (3, 3))
    H[..., 0, 1], H[..., 0, 2] = -w[..., 2], w[..., 1]
    H[..., 1, 0], H[..., 1, 2] = w[..., 2], -w[..., 0]
    H[..., 2, 0], H[..., 2, 1] = -w[..., 1], w[..., 0]
    return H


def so3_exp(w):
    w = np.asarray(w, dtype=np.float64)
    a2 = np.sum(w * w, axis=-1)
    small = a2 < 1e-4
    a = np.sqrt(np.where(small, 1.0, a2))
    A = np.where(small, 1 - a2 * (1 / 6 - a2 * (1 / 120 - a2 / 5040)), np.sin(a) / a)
    B = np.where(small, 0.5 - a2 * (1 / 24 - a2 * (1 / 720 - a2 / 40320)), (1 - np.cos(a)) / np.where(small, 1.0, a2))
    H = hat(w)
    return np.eye(3) + A[..., None, None] * H + B[..., None, None] * (H @ H)


def so3_log(R):
    """atan2(|k|, (tr - 1) / 2) with k the vector of the skew part; th / sin(th) by its series below 1e-6 rad.  Angles near pi: out of scope."""
    R = np.asarray(R, dtype=np.float64)
    k = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    s = np.linalg.norm(k, axis=-1)
    th = np.arctan2(s, 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1))
    small = th < 1e-6
    f = np.where(small, 1 + th * th / 6, th / np.where(small, 1.0, s))
    return f[..., None] * k


def so3_jr_inv(w):
    w = np.asarray(w, dtype=np.float64)
    a2 = np.sum(w * w, axis=-1)
    small = a2 < 1e-4
    a = np.sqrt(np.where(small, 1.0, a2))
    c = np.where(small, 1 / 12 + a2 * (1 / 720 + a2 / 30240), 1 / np.where(small, 1.0, a2) - (1 + np.cos(a)) / (2 * a * np.sin(a)))
    H = hat(w)
    return np.eye(3) + 0.5 * H + c[..., None, None] * (H @ H)


def unpack(P):
    P = np.asarray(P, dtype=np.float64).reshape(-1, 12)
    return np.transpose(P[:, :9].reshape(-1, 3, 3), (0, 2, 1)).copy(), P[:, 9:].copy()


def pack(R, p):
    out = np.empty((R.shape[0], 12))
    out[:, :9] = np.transpose(R, (0, 2, 1)).reshape(-1, 9)
    out[:, 9:] = p
    return out


def retract(P, dx):
    R, p = unpack(P)
    dx = np.asarray(dx, dtype=np.float64).reshape(-1, 6)
    return pack(R @ so3_exp(dx[:, :3]), p + dx[:, 3:])


# ---- factors -----------------------------------------------------------------------------------------------------------------
def between_lin(Pi, Pj, Z):
    """e (F, 6), Ji, Jj (F, 6, 6) of between factors: pose records (F, 12) of both ends, measurement records (F, 12)."""
    Ri, pi = unpack(Pi); Rj, pj = unpack(Pj)
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 12)
    Zr, zt = Z[:, :9].reshape(-1, 3, 3), Z[:, 9:]
    ZrT, RiT = np.transpose(Zr, (0, 2, 1)), np.transpose(Ri, (0, 2, 1))
    M = RiT @ Rj
    er = so3_log(ZrT @ M)
    d = np.einsum("fab,fb->fa", RiT, pj - pi)
    et = np.einsum("fab,fb->fa", ZrT, d - zt)
    Jr = so3_jr_inv(er)
    F = er.shape[0]
    Ji, Jj = np.zeros((F, 6, 6)), np.zeros((F, 6, 6))
    Jj[:, :3, :3] = Jr
    Ji[:, :3, :3] = -Jr @ np.transpose(M, (0, 2, 1))
    Ji[:, 3:, :3] = ZrT @ hat(d)
    Ji[:, 3:, 3:] = -ZrT @ RiT
    Jj[:, 3:, 3:] = ZrT @ RiT
    return np.concatenate([er, et], axis=1), Ji, Jj


def prior_lin(Pi, Z):
    Ri, pi = unpack(Pi)
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 12)
    Zr, zt = Z[:, :9].reshape(-1, 3, 3), Z[:, 9:]
    ZrT = np.transpose(Zr, (0, 2, 1))
    er = so3_log(ZrT @ Ri)
    et = np.einsum("fab,fb->fa", ZrT, pi - zt)
    J = np.zeros((er.shape[0], 6, 6))
    J[:, :3, :3] = so3_jr_inv(er)
    J[:, 3:, 3:] = ZrT
    return np.concatenate([er, et], axis=1), J


def invert_measurement(data18):
    """The record of the same between factor seen from the other end: Z^-1 = (Zr^T, -Zr^T zt).  The variances stay with their residual entries
    only to first order (e' = -Ad e), so equality of the two optima is exact only for isotropic rotation / translation variances."""
    d = np.asarray(data18, dtype=np.float64).reshape(-1, 18)
    Zr = d[:, :9].reshape(-1, 3, 3)
    out = d.copy()
    out[:, :9] = np.transpose(Zr, (0, 2, 1)).reshape(-1, 9)
    out[:, 9:12] = -np.einsum("fba,fb->fa", Zr, d[:, 9:12])
    return out


class Graph:
    """Factors in the order they were added (the order of the device's CSR rows): fi, fj (-1: prior), Z (F, 12), w = 1 / v6 (F, 6)."""

    def __init__(self, n_nodes):
        self.K = int(n_nodes)
        self.fi, self.fj = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        self.Z, self.w = np.zeros((0, 12)), np.zeros((0, 6))

    def add_edges(self, edge_ij, edge_data, node_offset_i=0, node_offset_j=0):
        ij = np.asarray(edge_ij, dtype=np.int64).reshape(-1, 2)
        d = np.asarray(edge_data, dtype=np.float64).reshape(-1, 18)
        self.fi = np.concatenate([self.fi, ij[:, 0] + node_offset_i]); self.fj = np.concatenate([self.fj, ij[:, 1] + node_offset_j])
        self.Z = np.concatenate([self.Z, d[:, :12]]); self.w = np.concatenate([self.w, 1.0 / d[:, 12:]])
        return self

    def add_priors(self, nodes, poses12, v6):
        nodes = np.atleast_1d(np.asarray(nodes, dtype=np.int64))
        R, p = unpack(poses12)
        v6 = np.broadcast_to(np.asarray(v6, dtype=np.float64).reshape(-1, 6), (nodes.size, 6))
        self.fi = np.concatenate([self.fi, nodes]); self.fj = np.concatenate([self.fj, np.full(nodes.size, -1)])
        self.Z = np.concatenate([self.Z, np.concatenate([R.reshape(-1, 9), p], axis=1)]); self.w = np.concatenate([self.w, 1.0 / v6])
        return self

    @property
    def F(self):
        return self.fi.size

    def residuals(self, X):
        X = np.asarray(X, dtype=np.float64).reshape(-1, 12)
        e = np.zeros((self.F, 6))
        b = self.fj >= 0
        if b.any():
            e[b] = between_lin(X[self.fi[b]], X[self.fj[b]], self.Z[b])[0]
        if (~b).any():
            e[~b] = prior_lin(X[self.fi[~b]], self.Z[~b])[0]
        return e

    def cost(self, X):
        e = self.residuals(X)
        return 0.5 * float(np.sum(e * e * self.w))

    def linearize(self, X):
        """D (K, 6, 6), g (K, 6) summed per node in factor order, B (F, 6, 6) = J_i^T W J_j (zero for priors), cost."""
        X = np.asarray(X, dtype=np.float64).reshape(-1, 12)
        F, K = self.F, self.K
        e = np.zeros((F, 6)); Ji = np.zeros((F, 6, 6)); Jj = np.zeros((F, 6, 6))
        b = self.fj >= 0
        if b.any():
            e[b], Ji[b], Jj[b] = between_lin(X[self.fi[b]], X[self.fj[b]], self.Z[b])
        if (~b).any():
            e[~b], Ji[~b] = prior_lin(X[self.fi[~b]], self.Z[~b])
        WJi, WJj = self.w[:, :, None] * Ji, self.w[:, :, None] * Jj
        D = np.zeros((K, 6, 6)); g = np.zeros((K, 6))
        np.add.at(D, self.fi, np.einsum("fka,fkb->fab", Ji, WJi)); np.add.at(g, self.fi, np.einsum("fka,fk->fa", WJi, e))
        np.add.at(D, self.fj[b], np.einsum("fka,fkb->fab", Jj[b], WJj[b])); np.add.at(g, self.fj[b], np.einsum("fka,fk->fa", WJj[b], e[b]))
        B = np.einsum("fka,fkb->fab", Ji, WJj)
        return D, g, B, 0.5 * float(np.sum(e * e * self.w))

    def dense_hessian(self, D, B):
        K = self.K
        H = np.zeros((K, 6, K, 6))
        H[np.arange(K), :, np.arange(K), :] = D
        b = np.nonzero(self.fj >= 0)[0]
        np.add.at(H, (self.fi[b], slice(None), self.fj[b], slice(None)), B[b])
        np.add.at(H, (self.fj[b], slice(None), self.fi[b], slice(None)), np.transpose(B[b], (0, 2, 1)))
        return H.reshape(6 * K, 6 * K)

    def free_nodes(self):
        used = np.zeros(self.K, dtype=bool)
        used[self.fi] = True; used[self.fj[self.fj >= 0]] = True
        return ~used


def lm_update(u, v, cost0, cost1, q1):
    """lm_decide (csrc/vxba_kernels.hip): accept when the cost fell; u *= max(1/3, 1 - (2 rho - 1)^3), v = 2; else u *= v, v *= 2."""
    q = cost0 - cost1
    if q > 0:
        gf = 1 - (2 * (q / q1) - 1) ** 3
        return True, u * (gf if gf > 1 / 3 else 1 / 3), 2.0
    return False, u * v, 2 * v


def dense_solve(graph, D, g, B, u):
    """(H + u diag H) dx = -g by Cholesky; nodes without factors get a zero step."""
    K = graph.K
    H = graph.dense_hessian(D, B)
    H[np.diag_indices(6 * K)] *= 1 + u
    free = np.repeat(graph.free_nodes(), 6)
    H[free, free] = 1.0
    L = np.linalg.cholesky(H)
    y = np.linalg.solve(L, -g.reshape(-1))          # (numpy has no triangular solve; the factorisation still proves H positive definite)
    return np.linalg.solve(L.T, y).reshape(K, 6)


def predicted_decrease(D, g, x, r, u):
    """-g.x - x.H x / 2 written with the residual r = -g - (H + u diag H) x of the damped system, as the device does."""
    diag = np.einsum("kaa->ka", D)
    return 0.5 * float(np.sum(x * (-g + r + u * diag * x)))


def dense_lm(graph, X0, max_iter=6, rel_cost_tol=1e-6, u0=DEFAULT_U0, v0=2.0, solver=None):
    """The device's outer loop with ``solver(D, g, B, u) -> (dx, r, info)`` (default: dense Cholesky, r = 0).  Returns dict(poses, report, grad):
    ``grad`` = the largest entry of the block-Jacobi scaled gradient D^-1 g at the returned poses, in metres / radians."""
    X = np.asarray(X0, dtype=np.float64).reshape(-1, 12).copy()
    u, v = float(u0), float(v0)
    report = []
    cost = None
    for it in range(max_iter):
        D, g, B, c0 = graph.linearize(X)
        if cost is None:
            cost = c0
        if solver is None:
            dx, r, info = dense_solve(graph, D, g, B, u), np.zeros_like(g), {}
        else:
            dx, r, info = solver(D, g, B, u)
        q1 = predicted_decrease(D, g, dx, r, u)
        Xt = retract(X, dx)
        free = graph.free_nodes()
        Xt[free] = X[free]
        c1 = graph.cost(Xt)
        accept, un, vn = lm_update(u, v, cost, c1, q1)
        report.append(dict(cost_before=cost, cost_after=c1, accepted=accept, u=u, predicted_decrease=q1, step=float(np.abs(dx).max()), **info))
        rel = abs((cost - c1) / cost) if cost != 0 else np.nan
        if accept:
            X, cost = Xt, c1
        u, v = un, vn
        if rel < rel_cost_tol:
            break
    D, g, B, _ = graph.linearize(X)
    used = ~graph.free_nodes()
    sg = np.zeros_like(g)
    sg[used] = np.linalg.solve(D[used], g[used][..., None])[..., 0]
    return dict(poses=X, report=report, grad=float(np.abs(sg).max()))


# ---- the device's CG, modelled ----------------------------------------------------------------------------------------------------
class CgModel:
    WAVES, SLOTS_PER_WAVE = 8, 10

    def __init__(self, graph):
        self.g = graph
        K, F = graph.K, graph.F
        # CSR rows in factor order: (node, factor, side, other)
        rows = [[] for _ in range(K)]
        for f in range(F):
            i, j = int(graph.fi[f]), int(graph.fj[f])
            if j >= 0:
                rows[i].append((f, 0, j)); rows[j].append((f, 1, i))
        self.maxdeg = max((len(r) for r in rows), default=0)
        self.steps = []                     # the q-th between entry of every node that has one: (nodes, factors, sides, others)
        for q in range(self.maxdeg):
            sel = [(n, *rows[n][q]) for n in range(K) if len(rows[n]) > q]
            a = np.asarray(sel, dtype=np.int64)
            self.steps.append((a[:, 0], a[:, 1], a[:, 2].astype(bool), a[:, 3]))
        slots = self.WAVES * self.SLOTS_PER_WAVE
        node = np.arange(K)
        slot = node % slots
        self.rounds = [node[node // slots == t] for t in range((K + slots - 1) // slots)]
        self.wave = slot // self.SLOTS_PER_WAVE
        self.lane0 = (slot % self.SLOTS_PER_WAVE) * 6

    def block_sum(self, v):
        """v (K, 6) per-element terms -> the workgroup sum as the kernel forms it."""
        part = np.zeros((self.WAVES, 64))
        for nodes in self.rounds:                                     # a lane adds its rounds in order
            for r in range(6):
                part[self.wave[nodes], self.lane0[nodes] + r] += v[nodes, r]
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[:, lanes ^ off]
        s = 0.0
        for w in range(self.WAVES):
            s += part[w, 0]
        return float(s)

    def apply(self, D, B, u, p):
        """(H + u diag H) p as the kernel forms it: per factor (B p_j) and (B^T p_i), each summed over its six columns from zero; per node the
        damped diagonal term, the diagonal block's six columns, then the factors' contributions in CSR order."""
        diag = np.einsum("kaa->ka", D)
        y = u * diag * p
        for c in range(6):
            y = y + D[:, :, c] * p[:, c:c + 1]
        for nodes, fs, sides, others in self.steps:
            Bq = np.where(sides[:, None, None], np.transpose(B[fs], (0, 2, 1)), B[fs])
            con = np.zeros((nodes.size, 6))
            for c in range(6):
                con = con + Bq[:, :, c] * p[others, c:c + 1]
            y[nodes] = y[nodes] + con
        return y

    def solve(self, D, g, B, u, tol=1e-8, cap=None):
        """Returns (x, r, dict(cg_iterations, cg_capped))."""
        K = self.g.K
        cap = max(200, 12 * K) if cap is None else cap
        used = ~self.g.free_nodes()
        Dd = D.copy()
        Dd[np.arange(K)[:, None], np.arange(6), np.arange(6)] *= 1 + u
        Minv = np.zeros_like(D)
        Minv[used] = np.linalg.inv(Dd[used])
        pre = lambda r: np.einsum("kab,kb->ka", Minv, r)
        x = np.zeros((K, 6)); r = -g.copy(); z = pre(r); p = z.copy()
        rz = self.block_sum(r * z); rz0 = rz
        it, capped = 0, False
        if rz0 > 0:
            while True:
                Ap = self.apply(D, B, u, p)
                alpha = rz / self.block_sum(p * Ap)
                x = x + alpha * p; r = r - alpha * Ap
                z = pre(r)
                rzn = self.block_sum(r * z)
                it += 1
                if not rzn > tol * tol * rz0:
                    break
                if it >= cap:
                    capped = True
                    break
                p = z + (rzn / rz) * p
                rz = rzn
        return x, r, dict(cg_iterations=it, cg_capped=capped)

    def solver(self, tol=1e-8, cap=None):
        return lambda D, g, B, u: self.solve(D, g, B, u, tol, cap)


class RefPoseGraph:
    """The checker behind the methods of ``vxba.PoseGraph`` that the drivers in ``voxel_slam_amd.hba`` use (their ``graph_cls`` hook)."""

    def __init__(self):
        self.g, self.X = None, None

    def set_poses(self, poses):
        self.X = np.asarray(poses, dtype=np.float64).reshape(-1, 12).copy()
        if self.g is None:
            self.g = Graph(self.X.shape[0])

    def add_edges(self, edge_ij, edge_data, node_offset_i=0, node_offset_j=0):
        self.g.add_edges(edge_ij, edge_data, node_offset_i, node_offset_j)

    def add_priors(self, nodes, poses12, v6):
        self.g.add_priors(nodes, poses12, v6)

    def optimize(self, options=None, **kw):
        if options is not None:
            kw = dict(max_iter=options.max_iter or 6, rel_cost_tol=1e-6 if options.rel_cost_tol < 0 else options.rel_cost_tol, u0=options.u0 or DEFAULT_U0, v0=options.v0 or 2.0)
        out = dense_lm(self.g, self.X, **kw)
        self.X = out["poses"]
        return out

    def close(self):
        pass
