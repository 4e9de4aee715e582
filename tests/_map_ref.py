"""Plain restatement of the incremental local map (csrc/vxba_map.hip; voxel_map.hpp:969-1333, 1545-1671, voxelslam.cpp:1313-1453, 1683-1687)
as Python objects, with no device idioms.  Test infrastructure only; tests/test_map_cpu.py pins it to the oracle's LocalMap and to the golden.

It evaluates in two ways.

Sequential float64, unfused, in the reference's push order (`RefMap`): everything the device promises bit for bit -- the point clusters,
the per-scan local clusters and cov_add of every push, push_fix and subdivision, child centres ((double)((float)(+-1) * ql)), node ids,
layers, flags, counts, the stored points and their order.  A Python float `acc + a * b` is the unfused operation, so no tolerance applies.

200-bit mpmath (`eig_exact`, `transform_exact`, `plane_update_exact`): what is only equal to rounding -- cluster_cov, the
eigen-decomposition, PointCluster::transform with the sums margi builds from it, plane_update.  Each has a twin on absolute values with every
subtraction an addition: the magnitude.  The exact replay of a stage starts from the float64 values the side under test exported (clusters,
cov_add, eigen-pairs, poses), so the error of one stage is not charged to the next.

The real-valued decisions of the tree (lam0 < min_eigen_value, lam0 / lam2 < thre[L], lam0 / lam1 > 0.12) are taken on the exact eigenvalues
of the float64 sums; `RefMap.margins` records how far each was from its threshold, in units of u M (the eigenvalue criterion's scale), so that a
case can be held to decisions no rounding can flip.  `RefMap.census` records which path of the device code each leaf takes at each stage.

`RefMap(..., variant=NAME)` switches on one degraded variant (see VARIANTS): what tests/test_map_cpu.py must reject."""
import numpy as np
import mpmath as mp
from mpmath import mpf

PREC = 200
U = 2.0 ** -53
SUB_TILE = 128          # map_subdivide_wave_kernel stages points through LDS in tiles of 128
FIX_TILE = 64           # map_fix_push_kernel: 64; map_push_kernel: 64-lane blocks
F32 = np.float32

VARIANTS = ("drop_remainder_tile", "second_tile_first", "unstable_rebucket", "fix_region_order", "octant_ge", "fused_to_world",
            "gate_min_point", "gate_max_points", "gate_num_step", "gate_last_num", "gate_isexist")
VALUE_VARIANTS = ("tr_cross", "pv_nc_transposed", "pv_centre_scale", "pv_gap_sign", "radius_double")     # degraded arithmetic of the 200-bit pieces


def voxel_index(w, voxel_size):
    """cut_voxel's float-typed index (voxel_map.hpp:1553-1560): the quotient rounds to float, a negative one steps down by one, the cast truncates."""
    loc = F32(w / voxel_size)
    if loc < F32(0.0):
        loc = F32(loc - F32(1.0))
    return int(loc)


def to_world(Rp, x, fused=False):
    """xx.R * pv.pnt + xx.p, unfused: ((R(r,0) x + R(r,1) y) + R(r,2) z) + p(r); Rp = R column-major | p."""
    if fused:
        with mp.workprec(PREC):
            return tuple(float(mpf(Rp[r]) * mpf(x[0]) + mpf(Rp[3 + r]) * mpf(x[1]) + mpf(Rp[6 + r]) * mpf(x[2]) + mpf(Rp[9 + r])) for r in range(3))
    return tuple(((Rp[r] * x[0] + Rp[3 + r] * x[1]) + Rp[6 + r] * x[2]) + Rp[9 + r] for r in range(3))


def cl_push(c, x):
    """PointCluster::push (tools.hpp:326-331) on [Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N]."""
    c[9] += 1.0
    c[0] += x[0] * x[0]; c[1] += x[0] * x[1]; c[2] += x[0] * x[2]
    c[3] += x[1] * x[1]; c[4] += x[1] * x[2]; c[5] += x[2] * x[2]
    c[6] += x[0]; c[7] += x[1]; c[8] += x[2]


def cov_add_point(acc, x, V):
    """cov_add += Bf_var(pv, vec) (voxel_map.hpp:91-106); acc 9 x 9, V the point's 3 x 3 variance, both as matrices (row, column)."""
    Bi = np.array([[2 * x[0], 0, 0], [x[1], x[0], 0], [x[2], 0, x[0]], [0, 2 * x[1], 0], [0, x[2], x[1]], [0, 0, 2 * x[2]]], dtype=np.float64)
    up = (Bi[:, 0:1] * V[0:1, :] + Bi[:, 1:2] * V[1:2, :]) + Bi[:, 2:3] * V[2:3, :]            # Biup[r][k] = sum_j Bi[r][j] V(j, k), left to right
    acc[:6, :6] += (up[:, 0:1] * Bi[:, 0][None, :] + up[:, 1:2] * Bi[:, 1][None, :]) + up[:, 2:3] * Bi[:, 2][None, :]
    acc[:6, 6:] += up
    acc[6:, :6] += up.T
    acc[6:, 6:] += V


def octant_of(w, c, ge=False):
    if ge:
        return 4 * (w[0] >= c[0]) + 2 * (w[1] >= c[1]) + (w[2] >= c[2])
    return 4 * (w[0] > c[0]) + 2 * (w[1] > c[1]) + (w[2] > c[2])


# ---- 200-bit pieces ---------------------------------------------------------------------------------------------------------------------
def _sym(c):
    return [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]


def cluster_cov_exact(cl):
    """P / N - vb vb^T of a float64 cluster, exact; and its magnitude |P| / N + |vb| |vb|^T (largest entry: the M of the eigen criteria)."""
    with mp.workprec(PREC):
        c = [mpf(float(v)) for v in cl]
        N = c[9]
        P = _sym(c)
        vb = [c[6] / N, c[7] / N, c[8] / N]
        C = mp.matrix(3, 3)
        M = mpf(0)
        for r in range(3):
            for q in range(3):
                C[r, q] = P[r][q] / N - vb[r] * vb[q]
                M = max(M, abs(P[r][q]) / N + abs(vb[r] * vb[q]))
        return C, float(M)


def eig_exact(cl):
    """Eigenvalues (ascending, mpf) and unit eigenvectors (columns, mpf) of the cluster's covariance, and M."""
    with mp.workprec(PREC):
        C, M = cluster_cov_exact(cl)
        E, Q = mp.eigsy(C)
        order = sorted(range(3), key=lambda k: E[k])
        lam = [E[k] for k in order]
        vec = [[Q[r, k] for r in range(3)] for k in order]
        return lam, vec, M


def transform_exact(cl, Rp, variant=None):
    """PointCluster::transform (tools.hpp:357-363) of a float64 cluster under a float64 pose: values (mpf) and magnitudes (float)."""
    with mp.workprec(PREC):
        out = []
        for sg in (1, 0):
            f = (lambda v: mpf(float(v))) if sg else (lambda v: abs(mpf(float(v))))
            c = [f(v) for v in cl]
            R = [[f(Rp[3 * q + r]) for q in range(3)] for r in range(3)]
            p = [f(Rp[9 + r]) for r in range(3)]
            P, v, N = _sym(c), c[6:9], c[9]
            Rv = [R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2] for r in range(3)]
            RP = [[sum(R[r][k] * P[k][q] for k in range(3)) for q in range(3)] for r in range(3)]
            W = [[sum(RP[r][k] * R[q][k] for k in range(3)) + Rv[r] * p[q] + (Rv[r] * p[q] if variant == "tr_cross" else Rv[q] * p[r]) + N * p[r] * p[q] for q in range(3)] for r in range(3)]
            out.append([W[0][0], W[0][1], W[0][2], W[1][1], W[1][2], W[2][2]] + [Rv[r] + N * p[r] for r in range(3)] + [N])
        return out[0], [float(x) for x in out[1]]


def plane_update_exact(cl, lam, evec, cov_add, variant=None):
    """OctoTree::plane_update (voxel_map.hpp:1118-1146) from float64 inputs -- the merged cluster, the eigenvalues, the eigenvectors as stored
    (evec[3 k + r] = component r of eigenvector k) and cov_add (9 x 9 matrix): centre (3), plane_var (6 x 6, rows / columns normal | centre),
    each as (values mpf, magnitudes float).  1 / (lam0 - lamk) enters the magnitude to first order: (1 / |d|) (|lam0| + |lamk|) / |d|."""
    with mp.workprec(PREC):
        res = []
        for sg in (1, 0):
            f = (lambda v: mpf(float(v))) if sg else (lambda v: abs(mpf(float(v))))
            s = 1 if sg else -1                      # a subtraction is an addition in the twin
            N = f(cl[9])
            nv = 1 / N
            c = [f(cl[6 + k]) / N for k in range(3)]
            Uv = [[f(evec[3 * k + r]) for r in range(3)] for k in range(3)]
            CA = [[f(cov_add[r][q]) for q in range(9)] for r in range(9)]
            ul = Uv[0]
            u_c = [[mpf(0)] * 9 for _ in range(3)]
            for k in (1, 2):
                uk = Uv[k]
                kc = sum(uk[j] * c[j] for j in range(3)); lc = sum(ul[j] * c[j] for j in range(3))
                fkl = [uk[0] * ul[0], uk[1] * ul[0] + uk[0] * ul[1], uk[2] * ul[0] + uk[0] * ul[2], uk[1] * ul[1], uk[1] * ul[2] + uk[2] * ul[1], uk[2] * ul[2],
                       -s * (kc * ul[0] + lc * uk[0]), -s * (kc * ul[1] + lc * uk[1]), -s * (kc * ul[2] + lc * uk[2])]
                d = mpf(float(lam[0])) - mpf(float(lam[k]))
                if variant == "pv_gap_sign":
                    d = -d
                inv = 1 / d if sg else (1 / abs(d)) * (abs(mpf(float(lam[0]))) + abs(mpf(float(lam[k])))) / abs(d)
                sc = nv * inv
                for r in range(3):
                    for q in range(9):
                        u_c[r][q] = u_c[r][q] + sc * uk[r] * fkl[q]
            Jc = [[sum(u_c[r][k] * CA[k][q] for k in range(9)) for q in range(9)] for r in range(3)]      # Jc[r][q] = sum_k u_c[r][k] cov_add(k, q)
            PV = [[mpf(0)] * 6 for _ in range(6)]
            for r in range(3):
                for q in range(3):
                    PV[r][q] = sum(Jc[r][k] * u_c[q][k] for k in range(9))
                    jn = nv * Jc[r][6 + q]
                    if variant == "pv_nc_transposed":
                        jn = nv * Jc[q][6 + r]
                    PV[r][3 + q] = jn; PV[3 + q][r] = jn
                    PV[3 + r][3 + q] = (nv if variant == "pv_centre_scale" else nv * nv) * CA[6 + r][6 + q]
            res.append((c, PV))
        (c, PV), (cm, PVm) = res
        return (c, [float(x) for x in cm]), (PV, [[float(x) for x in row] for row in PVm])


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------
class Node:
    def __init__(self, layer, W):
        self.layer, self.W = layer, W
        self.state = 0
        self.child = [None] * 8
        self.center = [0.0, 0.0, 0.0]
        self.ql = F32(0)
        self.isexist = self.has_sw = self.is_plane = False
        self.last_num, self.opt_state = 0, -1
        self.pcr_add, self.pcr_fix = [0.0] * 10, [0.0] * 10
        self.cov_add = np.zeros((9, 9))
        self.pcrs_local = None        # [slot][10]
        self.points = None            # [slot] -> indices into that slot's scan
        self.point_fix = []           # (world point (3 floats), variance 3 x 3)
        self.fix_cap = 0              # the device's region size (census only)
        self.eig = None               # (lam mpf[3], vec mpf[3][3], M) of the last decomposition
        self.key = self.path = 0
        self.updated = False          # plane_update ran in the last margi
        self.margi_path = None
        self.judged = -1              # the stage of the last eigen-decomposition by recut
        self.N_add = self.N_fix = 0.0

    def sw_open(self):
        if not self.has_sw:
            self.has_sw = True
            self.pcrs_local = [[0.0] * 10 for _ in range(self.W)]
            self.points = [[] for _ in range(self.W)]

    def sw_release(self):
        self.has_sw, self.pcrs_local, self.points = False, None, None

    @property
    def node_id(self):
        return (self.key << 16) | (self.path << 7) | self.layer


class RefMap:
    def __init__(self, voxel_size=1.0, max_layer=2, min_point=(5, 5, 5, 5), min_eigen_value=0.0025, plane_eigen_value_thre=(0.25, 0.25, 0.25, 0.25),
                 max_points=100, win_size=10, thread_num=5, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.voxel_size, self.max_layer, self.min_point, self.min_eigen_value = float(voxel_size), int(max_layer), tuple(min_point), float(min_eigen_value)
        self.thre, self.max_points, self.win_size, self.thread_num = tuple(plane_eigen_value_thre), int(max_points), int(win_size), int(thread_num)
        self.variant = variant
        self.mp = list(range(self.win_size))
        self.roots, self.root_order, self.slide_order = {}, [], []
        self.scans = [None] * self.win_size          # per ring slot: (pnt_body (n, 3), var (n, 3, 3))
        self.census, self.margins = [], []
        self.stage = 0

    def _v(self, name):
        return self.variant == name

    # -- nodes
    def _root(self, w, create=True):
        loc = tuple(voxel_index(w[k], self.voxel_size) for k in range(3))
        n = self.roots.get(loc)
        if n is None and create:
            n = Node(0, self.win_size)
            n.center = [(0.5 + loc[k]) * self.voxel_size for k in range(3)]
            n.ql = F32(self.voxel_size / 4.0)
            n.key = ((loc[0] + 32768) << 32) | ((loc[1] + 32768) << 16) | (loc[2] + 32768)
            self.roots[loc] = n
            self.root_order.append(loc)
            return n, loc, True
        return n, loc, False

    def _child_for(self, n, w):
        o = int(octant_of(w, n.center, ge=self._v("octant_ge")))
        if n.child[o] is None:
            c = Node(n.layer + 1, self.win_size)
            xyz = ((o >> 2) & 1, (o >> 1) & 1, o & 1)
            c.center = [n.center[k] + float(F32(2 * xyz[k] - 1) * n.ql) for k in range(3)]
            c.ql = F32(n.ql / F32(2))
            c.key, c.path = n.key, n.path | (o << (3 * (2 - n.layer)))
            n.child[o] = c
        return n.child[o]

    def _push(self, n, slot, idx, x, V, w):
        n.sw_open()
        n.isexist = True
        if n.layer < self.max_layer:
            n.points[slot].append(idx)
        cl_push(n.pcrs_local[slot], x)
        cl_push(n.pcr_add, w)
        cov_add_point(n.cov_add, w, V)

    def _push_fix(self, n, w, V, novar):
        if n.layer < self.max_layer:
            n.point_fix.append((w, V))
        cl_push(n.pcr_fix, w)
        cl_push(n.pcr_add, w)
        if not novar:
            cov_add_point(n.cov_add, w, V)

    # -- cut_voxel_multi (voxel_map.hpp:1545-1639)
    def cut_voxel(self, ord_, pnt_body, var, pwld):
        self.stage += 1
        pnt = np.asarray(pnt_body, dtype=np.float64).reshape(-1, 3); var = np.asarray(var, dtype=np.float64).reshape(-1, 3, 3); pw = np.asarray(pwld, dtype=np.float64).reshape(-1, 3)
        slot = self.mp[ord_]
        self.scans[slot] = (pnt, var)
        groups, touched = {}, []
        for i in range(pnt.shape[0]):
            w = tuple(float(v) for v in pw[i])
            n, loc, new = self._root(w)
            if not new:
                n.isexist = True
            if loc not in self.slide_order:
                self.slide_order.append(loc)
            if loc not in groups:
                groups[loc] = []; touched.append(loc)
            groups[loc].append((i, w))
        if len(touched) < self.thread_num:
            return
        runs = {}
        for loc in touched:
            for i, w in groups[loc]:
                n = self.roots[loc]
                while n.state != 0:
                    n = self._child_for(n, w)
                self._push(n, slot, i, tuple(float(v) for v in pnt[i]), var[i], w)
                runs[id(n)] = (n, runs.get(id(n), (n, 0))[1] + 1)
        for n, ln in runs.values():
            self.census.append(dict(stage=self.stage, op="push", node=n.node_id, run=ln))

    # -- cut_voxel, fix form (voxel_map.hpp:1641-1671, allocate_fix :1048-1072, push_fix_novar :1007-1013)
    def cut_voxel_fix(self, pnt_world, var=None, jour=0.0):
        self.stage += 1
        pw = np.asarray(pnt_world, dtype=np.float64).reshape(-1, 3)
        vv = np.zeros((pw.shape[0], 3, 3)) if var is None else np.asarray(var, dtype=np.float64).reshape(-1, 3, 3)
        runs = {}
        for i in range(pw.shape[0]):
            w = tuple(float(v) for v in pw[i])
            n, _, _ = self._root(w)
            while n.state != 0:
                n = self._child_for(n, w)
            if id(n) not in runs:
                runs[id(n)] = [n, 0, len(n.point_fix)]
            runs[id(n)][1] += 1
            self._push_fix(n, w, vv[i], novar=True)
        for n, ln, fc in runs.values():
            grown = False
            if n.layer < self.max_layer:
                need = fc + ln
                grown = need > n.fix_cap
                fill = "exact" if need == n.fix_cap else ("room" if need < n.fix_cap else "grown")
                if grown:
                    n.fix_cap = 2 * need
                self.census.append(dict(stage=self.stage, op="fix_push", node=n.node_id, run=ln, had=fc, fill=fill, moved=grown and fc > 0))
            else:
                self.census.append(dict(stage=self.stage, op="fix_push", node=n.node_id, run=ln, had=fc, fill="nostore", moved=False))

    # -- recut (voxel_map.hpp:1148-1194) + tras_opt (:1308-1333), as multi_recut drives them
    def _decide(self, n, what, value, threshold, scale):
        """A real-valued decision on exact eigenvalues; the margin in units of u * scale."""
        self.margins.append(dict(stage=self.stage, node=n.node_id, what=what, margin=float(abs(value - threshold) / (U * scale))))
        return value < threshold

    def _recut(self, n, win_count, poses):
        if n.state == 0:
            n.opt_state = -1
            N, mpt = n.pcr_add[9], self.min_point[n.layer] + (1 if self._v("gate_min_point") else 0)
            self.census.append(dict(stage=self.stage, op="judge", node=n.node_id, N=int(N), min_point=self.min_point[n.layer], layer=n.layer))
            if N <= mpt:
                n.is_plane = False
                return
            if not n.isexist or not n.has_sw:
                return
            lam, vec, M = eig_exact(n.pcr_add)
            n.eig = (lam, vec, M)
            n.judged = self.stage
            with mp.workprec(PREC):
                a = self._decide(n, "min_eigen_value", lam[0], mpf(self.min_eigen_value), M)
                # lam0 / lam2 < thre  <=>  lam0 - thre lam2 < 0; its error scale is that of an eigenvalue
                b = self._decide(n, "thre", lam[0] / lam[2], mpf(self.thre[n.layer]), M / float(lam[2])) if a else False
            n.is_plane = bool(a and b)
            if n.is_plane or n.layer >= self.max_layer:
                return
            self._split(n, win_count, poses)
        for c in n.child:
            if c is not None:
                self._recut(c, win_count, poses)

    def _tiles(self, seq):
        """The order in which the device folds a range: tile after tile; the degraded variants change it."""
        seq = list(seq)
        if len(seq) <= SUB_TILE:
            return seq
        tiles = [seq[k:k + SUB_TILE] for k in range(0, len(seq), SUB_TILE)]
        if self._v("drop_remainder_tile") and len(tiles[-1]) < SUB_TILE:
            tiles = tiles[:-1]
        if self._v("second_tile_first"):
            tiles[0], tiles[1] = tiles[1], tiles[0]
        return [x for t in tiles for x in t]

    def _split(self, n, win_count, poses):
        keep = (n.layer + 1) < self.max_layer
        if n.pcr_fix[9] != 0:
            fc = len(n.point_fix)
            self.census.append(dict(stage=self.stage, op="sub_fix", node=n.node_id, fc=fc, keep=keep, layer=n.layer,
                                    path="none" if fc == 0 else ("tile" if fc <= SUB_TILE else ("serial" if keep else "multi_nokeep"))))
            for w, V in self._tiles(n.point_fix):
                self._push_fix(self._child_for(n, w), w, V, novar=False)
            for c in n.child:
                if c is not None:
                    c.fix_cap = len(c.point_fix)
            n.point_fix, n.fix_cap = [], 0
        for i in range(win_count):
            slot = self.mp[i]
            pnt, var = self.scans[slot]
            idxs = n.points[slot]
            if idxs:
                self.census.append(dict(stage=self.stage, op="sub_scan", node=n.node_id, pc=len(idxs), keep=keep, layer=n.layer, scan=i,
                                        path="tile" if len(idxs) <= SUB_TILE else ("rebucket" if keep else "multi_nokeep")))
            for idx in self._tiles(idxs):
                x = tuple(float(v) for v in pnt[idx])
                w = to_world(poses[i], x, fused=self._v("fused_to_world"))
                self._push(self._child_for(n, w), slot, idx, x, var[idx], w)
            if self._v("unstable_rebucket") and len(idxs) > SUB_TILE:
                for c in n.child:
                    if c is not None and c.has_sw and c.points[slot]:
                        c.points[slot] = c.points[slot][::-1]
        n.sw_release()
        n.state = 1

    def _tras_opt(self, n, counter):
        if n.state == 0:
            if n.isexist and n.is_plane and n.has_sw:
                lam, _, M = n.eig
                with mp.workprec(PREC):
                    thin = self._decide(n, "ratio_0.12", lam[0] / lam[1], mpf(0.12), M / float(lam[1]))
                    thin = thin or lam[0] / lam[1] == mpf(0.12)          # `> 0.12` returns
                if not thin:
                    return
                n.opt_state = counter[0]
                counter[0] += 1
        else:
            for c in n.child:
                if c is not None:
                    self._tras_opt(c, counter)

    def recut(self, win_count, poses):
        """multi_recut; returns the number of voxels tras_opt pushes."""
        self.stage += 1
        poses = [[float(v) for v in p] for p in np.asarray(poses, dtype=np.float64).reshape(-1, 12)[:win_count]]
        if len(self.slide_order) < self.thread_num:
            return 0
        for loc in self.slide_order:
            self._recut(self.roots[loc], win_count, poses)
        counter = [0]
        for loc in self.slide_order:
            self._tras_opt(self.roots[loc], counter)
        return counter[0]

    # -- margi (voxel_map.hpp:1196-1305) with mgsize = 1, as multi_margi drives it
    def _margi(self, n, win_count, poses):
        if n.state == 0:
            if not n.isexist or not n.has_sw:
                return
            m0 = self.mp[0]
            adopt = n.opt_state >= 0
            n.opt_state = -1
            Nadd = n.pcr_fix[9] + sum(n.pcrs_local[self.mp[i]][9] for i in range(win_count))
            l0 = list(n.pcrs_local[m0])
            Nfix0 = n.pcr_fix[9]
            n.margi_path = dict(adopt=adopt, l0=l0, fix_before=list(n.pcr_fix), locals=[list(n.pcrs_local[self.mp[i]]) for i in range(win_count)], empty_oldest=l0[9] == 0)
            n.pcr_add = None           # to rounding only: see transform_exact
            n.N_add = Nadd
            n.updated = False
            mpts = self.max_points + (1 if self._v("gate_max_points") else 0)
            step, few = 5 + (1 if self._v("gate_num_step") else 0), 10 + (1 if self._v("gate_last_num") else 0)
            ev = dict(stage=self.stage, op="margi", node=n.node_id, adopt=adopt, empty_oldest=l0[9] == 0, Nfix=int(Nfix0), Nadd=int(Nadd), last_num=n.last_num, is_plane=n.is_plane,
                      capped=not (Nfix0 < self.max_points), move="none", diff=int(Nadd) - n.last_num)
            if Nfix0 < mpts and n.is_plane:
                if int(Nadd) - n.last_num >= step or n.last_num <= few:
                    n.updated = True
                    n.last_num = int(Nadd)
            ev["updated"] = n.updated
            Nadd_after = Nadd
            if Nfix0 < mpts:
                if l0[9] != 0:
                    n.pcr_fix = None; n.N_fix = Nfix0 + l0[9]
                    pnt, var = self.scans[m0]
                    pc0, fc = len(n.points[m0]), len(n.point_fix)
                    if pc0 > 0:
                        heavy = fc + pc0 > n.fix_cap
                        ev["move"] = "heavy" if heavy else "light"
                        ev["fill"] = fc + pc0 - n.fix_cap
                        new = [(to_world(poses[0], tuple(float(v) for v in pnt[idx]), fused=self._v("fused_to_world")), var[idx]) for idx in n.points[m0]]
                        if heavy:
                            n.fix_cap = 2 * (fc + pc0)
                            if self._v("fix_region_order") and fc > 0:
                                n.point_fix = new + n.point_fix
                                new = []
                        n.point_fix = n.point_fix + new
                else:
                    n.N_fix = Nfix0
            else:
                n.N_fix = Nfix0
                if l0[9] != 0:
                    Nadd_after = Nadd - l0[9]
                n.point_fix, n.fix_cap = [], 0
            if l0[9] != 0:
                n.pcrs_local[m0] = [0.0] * 10
                n.points[m0] = []
            n.N_add = Nadd_after
            ev["isexist_gap"] = int(Nadd_after - n.N_fix)
            n.isexist = not (n.N_fix >= Nadd_after + (1 if self._v("gate_isexist") else 0))
            self.census.append(ev)
        else:
            n.isexist = False
            for c in n.child:
                if c is not None:
                    self._margi(c, win_count, poses)
                    n.isexist = n.isexist or c.isexist

    def margi(self, win_count, poses):
        self.stage += 1
        poses = [[float(v) for v in p] for p in np.asarray(poses, dtype=np.float64).reshape(-1, 12)[:win_count]]
        if len(self.slide_order) < self.thread_num:
            return
        keep = []
        for loc in self.slide_order:
            self._margi(self.roots[loc], win_count, poses)
        for loc in self.slide_order:
            r = self.roots[loc]
            if r.isexist:
                keep.append(loc)
            else:
                for n in self._walk(r, leaves_only=False):
                    if n.has_sw:
                        n.sw_release()
        self.slide_order = keep

    def drop_root(self, w):
        """The release of one root voxel (the one that holds world point w) with its subtree; it must not be under the window."""
        loc = tuple(voxel_index(float(w[k]), self.voxel_size) for k in range(3))
        assert loc in self.roots and loc not in self.slide_order
        del self.roots[loc]
        self.root_order.remove(loc)

    def slide(self, mgsize=1):
        self.mp = [(m + mgsize) % self.win_size for m in self.mp]

    # -- views
    def _walk(self, n, leaves_only=True):
        if n.state == 0 or not leaves_only:
            yield n
        if n.state != 0:
            for c in n.child:
                if c is not None:
                    yield from self._walk(c, leaves_only)

    def leaf_nodes(self):
        out = [n for loc in self.root_order for n in self._walk(self.roots[loc])]
        return sorted(out, key=lambda n: n.node_id)

    def leaves(self):
        """The bit-for-bit part of a leaf table, sorted by node id (fields as vxba.LocalMap.leaves; clusters margi has rebuilt are NaN except N)."""
        ns = self.leaf_nodes()
        W = self.win_size
        slide_keys = {self.roots[loc].key for loc in self.slide_order}
        nan10 = lambda N: [np.nan] * 9 + [N]
        out = dict(node_id=np.array([n.node_id for n in ns], dtype=np.uint64), layer=np.array([n.layer for n in ns]), isexist=np.array([n.isexist for n in ns], dtype=bool),
                   is_plane=np.array([n.is_plane for n in ns], dtype=bool), has_sw=np.array([n.has_sw for n in ns], dtype=bool), last_num=np.array([n.last_num for n in ns]),
                   n_point_fix=np.array([len(n.point_fix) for n in ns]), in_slide=np.array([n.key in slide_keys for n in ns], dtype=bool),
                   opt_state=np.array([n.opt_state for n in ns]),
                   pcr_add=np.array([n.pcr_add if n.pcr_add is not None else nan10(n.N_add) for n in ns], dtype=np.float64).reshape(-1, 10),
                   pcr_fix=np.array([n.pcr_fix if n.pcr_fix is not None else nan10(n.N_fix) for n in ns], dtype=np.float64).reshape(-1, 10),
                   cov_add=np.array([n.cov_add for n in ns]).reshape(-1, 9, 9),
                   pcrs_local=np.array([[n.pcrs_local[self.mp[s]] for s in range(W)] if n.has_sw else np.zeros((W, 10)) for n in ns], dtype=np.float64).reshape(-1, W, 10),
                   n_points=np.array([[len(n.points[self.mp[s]]) for s in range(W)] if n.has_sw else [0] * W for n in ns], dtype=np.int64).reshape(-1, W),
                   center=np.array([n.center for n in ns]).reshape(-1, 3))
        return out

    def leaf_points(self, node, which):
        """(n, 3), (n, 3, 3): which = -1 the fix points (world), which = i the window's i-th scan (body), in stored order."""
        if which < 0:
            P = [w for w, _ in node.point_fix]; V = [v for _, v in node.point_fix]
        else:
            idx = node.points[self.mp[which]] if node.has_sw else []
            pnt, var = self.scans[self.mp[which]] if idx else (None, None)
            P = [pnt[i] for i in idx]; V = [var[i] for i in idx]
        return np.array(P, dtype=np.float64).reshape(-1, 3), np.array(V, dtype=np.float64).reshape(-1, 3, 3)
