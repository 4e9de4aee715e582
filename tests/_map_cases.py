"""Cases, criteria and measured constants for the local map on its own (csrc/vxba_map.hip) against tests/_map_ref.py.  Test infrastructure only.

A case is a parameter set and a list of operations -- ("fix", world points, variances, jour), ("scan", body points, variances, pose),
("release", jour_now, min_age, root) -- that `run` drives through the reference and through a side under test (the oracle's LocalMap on the
CPU, vxba.LocalMap on the GPU) in lockstep.  A scan is cut_voxel -> recut (+ tras_opt into the side's factor) and, once the window is full,
evaluate_only_residual at the same poses (the optimiser's cache, no BA: the poses are the case's) -> margi -> ring shift.  After every stage:

  bit for bit   node ids, layers, flags, counts, last_num, the window clusters, cov_add, pcr_add / pcr_fix until margi rebuilds them (their N
                always), the stored points of every leaf in order (fix points and each window scan), plane centre, normal and radius as
                functions of the exported cluster and eigen-pairs (one division, a copy, one float rounding)
  to rounding   eigenvalues, eigenvectors, margi's transformed sums, plane_var -- each replayed in 200-bit arithmetic from the float64 values the
                side exported in front of that stage, judged per entry / per 3 x 3 block against its own magnitude (u = 2^-53):
      eigenvalues          |dlam|                 <= C_EIG u M            M = largest entry of |P| / N + |vb| |vb|^T
      normal (up to sign)  |dn|_inf               <= C_VEC u M / (lam1 - lam0)
      other eigenvectors   each up to sign, |du1|_inf <= C_VEC1 u M / min(lam1 - lam0, lam2 - lam1), |du2|_inf <= C_VEC2 u M / (lam2 - lam1);
                           where lam2 - lam1 < 1e3 u M only the projector of the pair, u1 u1^T + u2 u2^T against I - n n^T, at
                           C_PROJ u M / (lam1 - lam0) (judged everywhere, which gives C_PROJ its measurement)
      margi's sums         |d pcr|                <= (C_TR + number of additions) u mag
      plane_var            per block (normal-normal, normal-centre, centre-centre)  <= C_PV[block] u max(mag[block])
  margi's adopt branch (the optimiser's cache taken over): the factor's merged cluster, read in front of margi, is held to the same exact sum as
                the recomputed one and its eigen-pairs to the exact decomposition of it; the leaf must end with exactly those values (less the
                exact oldest scan, to rounding, where max_points caps it).

The constants K_* are the largest errors, in those units, of CPU reference code against mpmath over the cases of this module -- the oracle's
LocalMap on the window-form cases and, for every case (the fix form included), the float64 restatement `HostSide` -- measured by `python -m tests._map_cases --calibrate` and never on the device.  Criteria use C = 4 K (contraction and another
association); tests/test_map_cpu.py holds the oracle to 2 K.

Tile seams the ladders straddle: 128 points per LDS tile in map_subdivide_wave_kernel (fold, `tmp` re-bucketing, the serial fix copy above one
tile), 64 in map_fix_push_kernel and map_push_kernel."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import mpmath as mp

from tests import _map_ref as R

U = R.U
ORIGIN = np.array([3.0, -2.0, 0.0])
BASE = dict(voxel_size=1.0, max_layer=2, min_point=(20, 20, 15, 10), min_eigen_value=0.02, plane_eigen_value_thre=(0.25, 0.25, 0.25, 0.25), max_points=100, thread_num=1)
IDENT = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])

# measured by --calibrate: the largest error, in units of u x magnitude and rounded up, of CPU reference code against mpmath over all cases -- the
# oracle's LocalMap on the window-form cases (it has no fix form) and the host restatement (HostSide) on every case; the measured digits stand beside each
K_EIG = 1.26                     # 1.257  (pc127_three, the adopted cache behind margi)
K_VEC = 0.54                     # 0.535  (pc257_three, the adopted cache)
K_VEC1, K_VEC2 = 0.53, 0.53      # 0.526, 0.526  (margi, recut)
K_PROJ = 0.54                    # 0.535
K_TR = 2.61                      # 2.607  (pc65_three, pcr_fix behind margi; the one addition already taken off)
K_PV = (0.82, 1.77, 2.24)        # normal-normal 0.811, normal-centre 1.764 (host restatement, pc127_three; the oracle 1.288), centre-centre 2.239
FACTOR_DEVICE, FACTOR_CPU = 4.0, 2.0
HONEST = 100.0          # every real-valued decision clears its threshold by 100 x the eigenvalue criterion


def small_pose(k):
    """Rotation of a few degrees about a tilted axis and a translation of centimetres, different per scan; R column-major | p."""
    a = np.deg2rad(1.5 + 0.7 * k)
    ax = np.array([0.3, -0.5, 0.8]); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    return np.concatenate([Rm.T.reshape(9), np.array([0.02 * k, -0.015, 0.01 * (k % 3)])])


def variances(n, rng):
    """Exactly symmetric positive variances of about (1 cm)^2."""
    a = rng.normal(size=(n, 3, 3)) * 0.01
    v = np.einsum("nij,nkj->nik", a, a)
    v = np.triu(v) + np.transpose(np.triu(v, 1), (0, 2, 1))
    return v + np.eye(3) * 1e-5


def patch(rng, n, plane, lo=(0.05, 0.05), hi=(0.95, 0.95), origin=ORIGIN, noise=0.005, vs=1.0):
    """n world points on the plane z = 0.3 ("z") or x = 0.6 ("x") of the voxel at `origin` (units of the voxel), 5 mm noise."""
    a = rng.uniform(lo[0], hi[0], n); b = rng.uniform(lo[1], hi[1], n); e = rng.normal(0, noise, n)
    loc = np.stack([a, b, 0.3 + e], 1) if plane == "z" else np.stack([0.6 + e, a, b], 1)
    return origin + vs * loc


def body_of(pose, world):
    """Body points whose unfused world image under `pose` is what the case then uses (not necessarily `world` to the last bit)."""
    Rm = pose[:9].reshape(3, 3).T
    return (world - pose[9:12]) @ Rm


def scan_op(rng, world, pose=IDENT):
    body = np.ascontiguousarray(body_of(pose, world)) if pose is not IDENT else np.ascontiguousarray(world)
    return ("scan", body, variances(body.shape[0], rng), np.asarray(pose, dtype=np.float64))


def two_planes(rng, n, conc=False, **kw):
    """The basic construction: n points in one root voxel, half on z = 0.3 and half on x = 0.6: not a plane at layer 0, splits into 4 to 6 children and on
    to layer 2.  conc: four fifths of them inside the octant (1, 0, 0), so that one child at layer 1 holds more than half of them and splits again."""
    nz = n // 2
    if not conc:
        return np.concatenate([patch(rng, nz, "z", **kw), patch(rng, n - nz, "x", **kw)])
    mz, mx = (4 * nz) // 5, (4 * (n - nz)) // 5
    return np.concatenate([patch(rng, mz, "z", lo=(0.55, 0.05), hi=(0.95, 0.45), **kw), patch(rng, nz - mz, "z", **kw),
                           patch(rng, mx, "x", lo=(0.05, 0.05), hi=(0.45, 0.45), **kw), patch(rng, n - nz - mx, "x", **kw)])


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
PC_LADDER = (21, 63, 64, 65, 127, 128, 129, 257)
FC_LADDER = (1, 64, 127, 128, 129, 257)
FIX_RUNS = (1, 63, 64, 65, 129)


def case_pc_single(n, vs=1.0):
    rng = np.random.default_rng(1000 + n)
    prm = dict(BASE, win_size=1, voxel_size=vs)
    return dict(name=f"pc{n}_single_vs{vs}", prm=prm, ops=[scan_op(rng, two_planes(rng, n, conc=n >= 257, origin=ORIGIN * vs, vs=vs, noise=0.005 * vs))])


def case_pc_three(n):
    """Three scans in the window when the leaf splits: n coplanar points, then one (pc = 1 as the leaf's second scan), then n on the other plane."""
    rng = np.random.default_rng(2000 + n)
    ops = [scan_op(rng, patch(rng, max(n, 21), "z"), small_pose(0)), scan_op(rng, patch(rng, 1, "z"), small_pose(1)),
           scan_op(rng, patch(rng, n, "x", lo=(0.05, 0.05), hi=(0.95, 0.95)), small_pose(2))]
    return dict(name=f"pc{n}_three", prm=dict(BASE, win_size=3), ops=ops)


def case_fc(fc, max_layer):
    """fc coplanar fix points, a coplanar scan (a plane: the leaf stays), a scan on the other plane (it splits: fix_divide of fc points)."""
    rng = np.random.default_rng(3000 + 10 * fc + max_layer)
    ops = [("fix", patch(rng, fc, "z"), variances(fc, rng), 1.0), scan_op(rng, patch(rng, 25, "z")), scan_op(rng, patch(rng, max(40, fc), "x"))]
    return dict(name=f"fc{fc}_ml{max_layer}", prm=dict(BASE, win_size=3, max_layer=max_layer), ops=ops)


def case_fc0():
    """fc = 0 with pcr_fix.N != 0: a leaf capped by max_points whose region was reset, then split."""
    rng = np.random.default_rng(3999)
    ops = [scan_op(rng, patch(rng, 40, "z")), scan_op(rng, patch(rng, 25, "z")), scan_op(rng, patch(rng, 40, "x"))]
    return dict(name="fc0_capped", prm=dict(BASE, win_size=1, max_points=30), ops=ops)


def _roots(k):
    return [ORIGIN + np.array([2.0 * i, 0.0, 0.0]) for i in range(k)]


def case_fix_runs():
    """cut_voxel_fix runs of 1, 63, 64, 65, 129 points per leaf; a second call that fills the region exactly / leaves room / outgrows it (the move with
    run_dst >= 0); a third that outgrows every region; then a window on every leaf and a split, so that the moved points are folded."""
    rng = np.random.default_rng(4000)
    org = _roots(len(FIX_RUNS))
    def call(lens, jour):
        w = np.concatenate([patch(rng, n, "z", origin=o) for n, o in zip(lens, org)])
        o = rng.permutation(w.shape[0])              # runs interleaved in the input: the sort has to gather them
        return ("fix", w[o], variances(w.shape[0], rng), jour)
    ops = [call(FIX_RUNS, 1.0), call((1, 30, 64, 66, 129), 2.0), call((3, 100, 129, 1, 259), 3.0)]
    ops.append(scan_op(rng, np.concatenate([patch(rng, 25, "z", origin=o) for o in org])))
    ops.append(scan_op(rng, np.concatenate([patch(rng, n, "x", origin=o) for n, o in zip((40, 200, 260, 140, 520), org)])))
    return dict(name="fix_runs", prm=dict(BASE, win_size=3), ops=ops)


PUSH_RUNS = (63, 1, 1, 64, 2, 65, 21)      # sorted run heads at 0, 63, 64, 65, 129, 131, 196: lanes 63 / 0 / 1 of a 64-lane block, a run of 64 across a boundary, one of 65


def case_push_seams():
    """map_push_kernel: the roots are made one call at a time (node indices in that order), then ONE scan whose runs put heads on the seams."""
    rng = np.random.default_rng(5000)
    org = _roots(len(PUSH_RUNS))
    ops = [("fix", patch(rng, 1, "z", origin=o), None, 0.0) for o in org]
    w = np.concatenate([patch(rng, n, "z", origin=o) for n, o in zip(PUSH_RUNS, org)])
    o = rng.permutation(w.shape[0])
    ops.append(scan_op(rng, w[o], small_pose(1)))
    ops.append(scan_op(rng, np.concatenate([patch(rng, 30, "x", origin=o_) for o_ in org]), small_pose(2)))
    return dict(name="push_seams", prm=dict(BASE, win_size=3), ops=ops)


def case_window16():
    """win_size = MAXW = 16, 22 scans: every ring slot is reused and mp has wrapped; at scan 19 a second plane arrives and the leaf splits with sixteen
    scans in its window."""
    rng = np.random.default_rng(6000)
    ops = []
    for k in range(22):
        w = patch(rng, 3 + (k % 4), "z")
        if k == 18:
            w = np.concatenate([w, patch(rng, 60, "x")])
        ops.append(scan_op(rng, w, small_pose(k)))
    return dict(name="window16", prm=dict(BASE, win_size=16, max_points=40), ops=ops)


MARGI_A = (2, 1, 1, 1, 1, 2, 3, 1, 0, 0, 2, 0, 0)     # points per scan in leaf A: fix_count + pc0 one below, equal to and one above fix_cap; N = min_point and min_point + 1 in judge;
#                                                      Nfix max_points - 1 and max_points; fix.N equal to add.N and one apart
MARGI_B = (4, 3, 3, 1, 1, 3, 1, 0, 2, 0, 1, 0, 0)     # leaf B: last_num 0 -> 10 -> 11 (the `<= 10` side and the `> 10` side), then steps of 4 (no update) and 5 (update)
MARGI_C = (13, 10, 9, 0, 7, 0, 0, 5, 0, 0, 0, 0, 3)   # leaf C: a thick plane (lam0 / lam2 < thre, lam0 / lam1 > 0.12): never in the factor, recomputed by margi; Nfix 0 -> 13 > max_points


def case_margi():
    """Three plane leaves in three roots fed a chosen number of points per scan, window 3, max_points 12, min_point 5: every branch of margi and every
    integer gate on both sides (the census of tests/test_map_cpu.py says which)."""
    rng = np.random.default_rng(7000)
    oa, ob, oc = _roots(3)
    ops = []
    for k, (a, b, c) in enumerate(zip(MARGI_A, MARGI_B, MARGI_C)):
        parts = [patch(rng, a, "z", origin=oa), patch(rng, b, "z", origin=ob)]
        box = np.stack([rng.uniform(0.1, 0.9, c), 0.3 + rng.uniform(-0.08, 0.08, c), 0.3 + rng.uniform(-0.035, 0.035, c)], 1)
        parts.append(oc + box)
        ops.append(scan_op(rng, np.concatenate(parts), small_pose(k)))
    return dict(name="margi", prm=dict(BASE, win_size=3, max_points=12, min_point=(5, 5, 5, 5)), ops=ops)


def case_edges():
    """Geometry decided exactly: a coordinate equal to a node centre at each layer (`>` is false), exact positive and negative integers, a coordinate
    just below an integer whose float quotient rounds up into the next voxel, -0.0."""
    rng = np.random.default_rng(8000)
    w = two_planes(rng, 129)
    w[0] = ORIGIN + [0.5, 0.3, 0.3]            # x on the root's centre
    w[1] = ORIGIN + [0.6, 0.5, 0.5]            # y and z on the root's centre
    w[2] = ORIGIN + [0.75, 0.25, 0.3]          # x, y on a layer-1 centre
    w[3] = ORIGIN + [0.6, 0.25, 0.25]          # y, z on a layer-1 centre
    w[4] = ORIGIN + [0.5, 0.5, 0.5]
    w[5] = ORIGIN + [0.0, 0.3, 0.3]            # x = 3 exactly
    w[6] = ORIGIN + [0.6, 0.0, 0.3]            # y = -2 exactly: the negative quotient steps down a voxel
    w[7] = ORIGIN + [0.6, 1.0, 0.3]            # y = -1 exactly
    w[8] = np.array([4.0 - 1e-9, -1.7, 0.3])   # float(3.999999999) = 4: the next voxel
    w[9] = np.array([3.6, -1.7, -0.0])
    w[10] = np.array([3.6, -1.7, 0.0])
    w[11] = np.array([-1e-9, -1e-9, 0.3])      # float(-1e-9) < 0: voxel -1
    return dict(name="edges", prm=dict(BASE, win_size=1), ops=[scan_op(rng, w)])


def case_pool_moves(compact):
    """The fix ladder's 129 rung with a neighbouring root released in between (node pool and fix pool compacted)."""
    rng = np.random.default_rng(9000)
    nb = ORIGIN + np.array([0.0, 4.0, 0.0])
    ops = [("fix", patch(rng, 70, "z", origin=nb), variances(70, rng), 0.0), ("fix", patch(rng, 129, "z"), variances(129, rng), 100.0),
           ("fix", patch(rng, 140, "z"), variances(140, rng), 100.0), ("release", 100.0, 50, nb), scan_op(rng, patch(rng, 25, "z")), ("release", 100.0, 50, None),
           scan_op(rng, patch(rng, 270, "x"))]
    return dict(name=f"pool_moves_{'compact' if compact else 'plain'}", prm=dict(BASE, win_size=3), ops=ops, env=dict(VXBA_MAP_FIX_COMPACT_AT="100") if compact else {})


def all_cases():
    out = [case_pc_single(n) for n in PC_LADDER] + [case_pc_single(129, vs=0.5)] + [case_pc_three(n) for n in PC_LADDER[1:]]
    out += [case_fc(fc, ml) for fc in FC_LADDER for ml in (2, 1)] + [case_fc0(), case_fix_runs(), case_push_seams(), case_window16(), case_margi(), case_edges()]
    out += [case_pool_moves(False), case_pool_moves(True)]
    return out


CASE_NAMES = [c["name"] for c in all_cases()]


def get_case(name):
    return next(c for c in all_cases() if c["name"] == name)


# ---- sides under test -----------------------------------------------------------------------------------------------------------------
def by_id(lv):
    o = np.argsort(lv["node_id"], kind="stable")
    return {k: (v[o] if isinstance(v, np.ndarray) and v.shape[:1] == o.shape else v) for k, v in lv.items()}


class OracleSide:
    """The oracle's LocalMap (no fix form, no release: cases with those operations are not for it)."""
    name = "oracle"

    def __init__(self, prm):
        from tests import _oracle as O
        self.m, self.f = O.LocalMapOracle(**prm), O.Oracle(prm["win_size"])

    def leaves(self):
        return by_id(self.m.leaves())

    def cache(self, poses):
        if self.f.size() > 0:
            self.f.evaluate_only_residual(poses)

    def close(self):
        pass


class DeviceSide:
    name = "device"

    def __init__(self, vx, prm):
        self.m, self.f = vx.LocalMap(**prm), vx.LidarFactor(prm["win_size"])

    def leaves(self):
        return self.m.leaves()

    def cache(self, poses):
        if self.f.size() > 0:
            self.f.evaluate_only_residual(poses)

    def close(self):
        self.m.close(); self.f.close()


_HOSTLIB = None


def hostlib():
    """csrc/vxba_map_math.hpp (and the eigen-solver of csrc/vxba_math.hpp) built for the host with g++ -ffp-contract=off."""
    global _HOSTLIB
    if _HOSTLIB is None:
        here = os.path.dirname(os.path.abspath(__file__))
        src, so = os.path.join(here, "hostmath", "map_hostcheck.cpp"), os.path.join(here, "hostmath", "libmap_hostcheck.so")
        hdrs = [os.path.join(here, "..", "voxel-slam_amd", "csrc", h) for h in ("vxba_map_math.hpp", "vxba_lio_math.hpp", "vxba_lio_ctl.hpp", "vxba_math.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
        lib = C.CDLL(so)
        lib.maph_push.argtypes = [C.c_longlong, f64p, f64p, f64p, f64p, f64p, f64p]
        lib.maph_to_world.argtypes = [C.c_longlong, f64p, f64p, f64p]
        lib.maph_octant.argtypes = [C.c_longlong, f64p, f64p, np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")]
        lib.maph_voxel_index.argtypes = [C.c_longlong, f64p, C.c_double, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
        lib.maph_eig.argtypes = [f64p, f64p, f64p]
        lib.maph_transform.argtypes = [f64p, f64p, f64p]
        lib.maph_plane_update.argtypes = [f64p, f64p, f64p, f64p, f64p, f64p]
        _HOSTLIB = lib
    return _HOSTLIB


class HostSide:
    """The float64 restatement of what is only equal to rounding, for every case (the oracle has no fix form): a second RefMap carries the
    structure and the sequential sums, and the kernels' own arithmetic built for the host fills in the rest the way the device code does --
    the eigen-pairs of judge, the factor's cache (merged cluster and its eigen-pairs at the poses), margi's sums in the kernel's order,
    plane_update.  It stands where the device stands in `run`; its factor is the list of leaves tras_opt took."""
    name = "host"

    def __init__(self, prm):
        self.hm, self.ref = hostlib(), R.RefMap(**prm)
        self.m, self.f = self, self
        self.vox, self._cache = [], None

    # -- arithmetic
    def _eig(self, cl):
        ev, evec = np.zeros(3), np.zeros(9)
        self.hm.maph_eig(np.ascontiguousarray(cl, dtype=np.float64), ev, evec)
        return ev, evec

    def _tr(self, cl, pose):
        out = np.zeros(10)
        self.hm.maph_transform(np.ascontiguousarray(cl, dtype=np.float64), np.ascontiguousarray(pose, dtype=np.float64), out)
        return out

    def _rec(self, n):
        if not hasattr(n, "h"):
            n.h = dict(eig_val=np.zeros(3), eig_vec=np.zeros(9), center=np.zeros(3), normal=np.zeros(3), radius=0.0, plane_var=np.zeros((6, 6)))
        return n.h

    # -- the map
    def cut_voxel_fix(self, w, v, jour):
        self.ref.cut_voxel_fix(w, v, jour)

    def cut_voxel(self, ord_, body, var, pw):
        self.ref.cut_voxel(ord_, body, var, pw)

    def release(self, jour_now, min_age):
        return None

    def drop_root(self, root):
        self.ref.drop_root(root)

    def recut(self, wc, poses, f):
        n_f = self.ref.recut(wc, poses)
        for n in self.ref.leaf_nodes():
            if n.judged == self.ref.stage:
                h = self._rec(n)
                h["eig_val"], h["eig_vec"] = self._eig(n.pcr_add)
        self.vox = sorted((n for n in self.ref.leaf_nodes() if n.opt_state >= 0), key=lambda n: n.opt_state)
        assert len(self.vox) == n_f

    def cache(self, poses):
        self._cache = []
        for n in self.vox:
            s = np.array(n.pcr_fix, dtype=np.float64)
            for j in range(len(poses)):
                l = n.pcrs_local[self.ref.mp[j]]
                if l[9] != 0:
                    s = s + self._tr(l, poses[j])
            self._cache.append((s,) + self._eig(s))

    def margi(self, wc, poses, f):
        ref = self.ref
        cached = {id(n): c for n, c in zip(self.vox, self._cache or [])}
        ref.margi(wc, poses)
        for n in ref.leaf_nodes():
            mpth = n.margi_path
            if mpth is None or mpth.get("host") == "done":
                continue
            mpth["host"] = "done"
            h = self._rec(n)
            fix = np.array(mpth["fix_before"], dtype=np.float64)
            w0 = self._tr(mpth["l0"], poses[0]) if mpth["l0"][9] != 0 else None
            if mpth["adopt"]:
                add, h["eig_val"], h["eig_vec"] = cached[id(n)]
                add = add.copy()
            else:
                add = fix.copy()
                for j, l in enumerate(mpth["locals"]):
                    if l[9] != 0:
                        add = add + self._tr(l, poses[j])
                if n.is_plane:
                    h["eig_val"], h["eig_vec"] = self._eig(add)
            if n.updated:
                cen, pv = np.zeros(3), np.zeros(36)
                self.hm.maph_plane_update(np.ascontiguousarray(n.cov_add.T).reshape(81), np.ascontiguousarray(add), np.ascontiguousarray(h["eig_vec"]),
                                          np.ascontiguousarray(h["eig_val"]), cen, pv)
                h["center"], h["normal"], h["radius"], h["plane_var"] = cen, h["eig_vec"][0:3].copy(), float(np.float32(h["eig_val"][2])), pv.reshape(6, 6).T.copy()
            if fix[9] < ref.max_points:
                if w0 is not None:
                    fix = fix + w0
            elif w0 is not None:
                add = add - w0
            n.pcr_add, n.pcr_fix = [float(v) for v in add], [float(v) for v in fix]

    def slide(self, k):
        self.ref.slide(k)

    def leaf_points(self, node_id, which):
        n = next(x for x in self.ref.leaf_nodes() if x.node_id == node_id)
        return self.ref.leaf_points(n, which)

    def leaves(self):
        lv = self.ref.leaves()
        ns = self.ref.leaf_nodes()
        for key, shape in (("eig_val", (3,)), ("eig_vec", (9,)), ("center", (3,)), ("normal", (3,)), ("plane_var", (6, 6))):
            lv[key] = np.array([self._rec(n)[key] for n in ns], dtype=np.float64).reshape((-1,) + shape)
        lv["radius"] = np.array([self._rec(n)["radius"] for n in ns], dtype=np.float64)
        return lv

    # -- the factor
    def clear(self):
        self.vox, self._cache = [], None

    def size(self):
        return len(self.vox)

    def read_cache(self):
        return (np.array([c[1] for c in self._cache]), np.array([c[2] for c in self._cache]), np.array([c[0] for c in self._cache]))

    def close(self):
        pass


def oracle_can_run(case):
    return all(op[0] == "scan" for op in case["ops"])


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
class Errors:
    """Largest error per criterion, in units of u x magnitude, with where it occurred."""

    def __init__(self):
        self.worst = {}

    def add(self, kind, ratio, where):
        if kind not in self.worst or ratio > self.worst[kind][0]:
            self.worst[kind] = (float(ratio), where)

    def merge(self, other):
        for k, (r, w) in other.worst.items():
            self.add(k, r, w)

    def get(self, kind):
        return self.worst.get(kind, (0.0, None))[0]


EXACT = ("centre", "normal", "radius", "adopt")      # promised bit for bit: the ratio is 0 or infinite, the limit 0


def limits(factor):
    out = dict(eig=factor * K_EIG, vec=factor * K_VEC, vec1=factor * K_VEC1, vec2=factor * K_VEC2, proj=factor * K_PROJ, tr=factor * K_TR,
               pv_nn=factor * K_PV[0], pv_nc=factor * K_PV[1], pv_cc=factor * K_PV[2])
    out.update({k: 0.0 for k in EXACT})
    return out


def missed(err, factor):
    """The criteria the errors miss: kind -> (ratio, where)."""
    lim = limits(factor)
    return {k: v for k, v in err.worst.items() if v[0] > lim[k]}


def check_errors(err, factor, label=""):
    bad = missed(err, factor)
    assert not bad, (label, bad, limits(factor))


def _exact(err, kind, ok, where):
    err.add(kind, 0.0 if ok else float("inf"), where)


def same_bits(ref, side, stage):
    """Everything that is promised bit for bit, the stored points included."""
    a, b = ref.leaves(), side.leaves()
    assert np.array_equal(a["node_id"], b["node_id"]), (stage, "leaf set")
    for key in ("layer", "isexist", "is_plane", "has_sw", "last_num", "n_point_fix", "in_slide"):
        assert np.array_equal(np.asarray(a[key]).astype(np.int64), np.asarray(b[key]).astype(np.int64)), (stage, key, a[key], b[key])
    assert np.array_equal(a["opt_state"] >= 0, b["opt_state"] >= 0), (stage, "factor set")
    assert np.array_equal(a["n_points"], b["n_points"]), (stage, "n_points")
    assert np.array_equal(a["pcrs_local"], b["pcrs_local"]), (stage, "pcrs_local")
    assert np.array_equal(a["cov_add"], b["cov_add"]), (stage, "cov_add")
    for key in ("pcr_add", "pcr_fix"):
        known = ~np.isnan(a[key])
        assert np.array_equal(a[key][known], b[key][known]), (stage, key)
    nodes = ref.leaf_nodes()
    for k, n in enumerate(nodes):
        for which in [-1] + list(range(ref.win_size)):
            cnt = len(n.point_fix) if which < 0 else int(a["n_points"][k, which])
            if cnt == 0:
                continue
            pr, vr = ref.leaf_points(n, which)
            ps, vs_ = side.m.leaf_points(int(n.node_id), which)
            assert np.array_equal(pr, ps) and np.array_equal(vr, vs_), (stage, "stored points", hex(n.node_id), which)
    return a, b


def _f(x):
    return np.array([float(v) for v in x])


def check_eigen(err, b, k, where):
    """The exported eigen-pairs of leaf row k against the exact decomposition of the exported pcr_add."""
    return check_eigen_of(err, b["pcr_add"][k], b["eig_val"][k], b["eig_vec"][k], where)


def _vec_err(got, exact):
    return min(np.abs(got - exact).max(), np.abs(got + exact).max())


def check_eigen_of(err, cl, eig_val, eig_vec, where):
    """Eigenvalues and eigenvectors (eig_vec[3 k + r] = component r of eigenvector k) against the exact decomposition of the float64 cluster cl:
    every eigenvector up to sign with the smaller of its adjacent gaps; where lam1 and lam2 are closer than 1e3 u M the two are not separable
    and only their projector is judged (it is judged everywhere, with the normal's gap: it costs nothing and gives its constant a measurement)."""
    lam, vec, M = R.eig_exact(cl)
    with mp.workprec(R.PREC):
        for j in range(3):
            err.add("eig", abs(mp.mpf(float(eig_val[j])) - lam[j]) / (U * M), where)
        g01, g12 = float(lam[1] - lam[0]), float(lam[2] - lam[1])
    E = np.asarray(eig_vec, dtype=np.float64).reshape(3, 3)                # rows: eigenvectors
    ex = [_f(v) for v in vec]
    err.add("vec", _vec_err(E[0], ex[0]) * g01 / (U * M), where)
    if g12 >= 1e3 * U * M:
        err.add("vec1", _vec_err(E[1], ex[1]) * min(g01, g12) / (U * M), where)
        err.add("vec2", _vec_err(E[2], ex[2]) * g12 / (U * M), where)
    proj = E[1][:, None] * E[1][None, :] + E[2][:, None] * E[2][None, :]
    err.add("proj", np.abs(proj - (np.eye(3) - np.outer(ex[0], ex[0]))).max() * g01 / (U * M), where)
    return g12 / (U * M)


def check_plane_record(err, b, k, where, variant=None):
    """Centre, normal and radius are exact functions of what the leaf exports; plane_var per block against the exact replay from those values."""
    cl, lam, ev = b["pcr_add"][k], b["eig_val"][k], b["eig_vec"][k]
    _exact(err, "centre", np.array_equal(b["center"][k], cl[6:9] / cl[9]), where)
    _exact(err, "normal", np.array_equal(b["normal"][k], ev[0:3]), where)
    _exact(err, "radius", b["radius"][k] == (float(lam[2]) if variant == "radius_double" else float(np.float32(lam[2]))), where)
    (_, _), (PV, PVm) = R.plane_update_exact(cl, lam, ev, b["cov_add"][k], variant=variant)
    got = b["plane_var"][k]
    with mp.workprec(R.PREC):
        for name, rs, cs in (("pv_nn", range(3), range(3)), ("pv_nc", range(3), range(3, 6)), ("pv_nc", range(3, 6), range(3)), ("pv_cc", range(3, 6), range(3, 6))):
            mag = max(PVm[r][c] for r in rs for c in cs)
            e = max(abs(mp.mpf(float(got[r, c])) - PV[r][c]) for r in rs for c in cs)
            err.add(name, e / (U * mag), where)


def check_margi_sums(err, ref, node, b, k, poses, where, variant=None, cache=None):
    """pcr_add / pcr_fix after margi against the exact sums of exactly transformed clusters, from the float64 values in front of the stage.
    On the adopt branch `cache` = (eig_val, eig_vec, merged) of the leaf's voxel as the side's factor held them in front of margi: the merged
    cluster is held to the same exact sum, its eigen-pairs to the exact decomposition of it, and the leaf must end with exactly those values
    (the merged cluster less the exact oldest scan, to rounding, where the leaf is capped)."""
    mpth = node.margi_path
    with mp.workprec(R.PREC):
        tr = [R.transform_exact(l, poses[j], variant=variant) if l[9] != 0 else None for j, l in enumerate(mpth["locals"])]
        fix0 = [mp.mpf(v) for v in mpth["fix_before"]]
        capped = not (mpth["fix_before"][9] < ref.max_points)
        w0 = tr[0]
        val = list(fix0); mag = [abs(v) for v in fix0]; adds = 0
        for t in tr:
            if t is not None:
                val = [a + c for a, c in zip(val, t[0])]; mag = [a + c for a, c in zip(mag, t[1])]; adds += 1
        got = b["pcr_add"][k]
        if mpth["adopt"]:
            ev, evec, merged = cache
            for e in range(9):
                if mag[e] > 0:
                    err.add("tr", abs(mp.mpf(float(merged[e])) - val[e]) / (U * mag[e]) - adds, where + ("merged", e))
            _exact(err, "adopt", merged[9] == float(val[9]) and np.array_equal(b["eig_val"][k], ev) and np.array_equal(b["eig_vec"][k], evec), where)
            check_eigen_of(err, merged, ev, evec, where + ("cache",))
            if capped and w0 is not None:
                for e in range(9):
                    m_ = abs(mp.mpf(float(merged[e]))) + w0[1][e]
                    if m_ > 0:
                        err.add("tr", abs(mp.mpf(float(got[e])) - (mp.mpf(float(merged[e])) - w0[0][e])) / (U * m_) - 1, where + ("pcr_add", e))
                _exact(err, "adopt", got[9] == merged[9] - mpth["l0"][9], where)
            else:
                _exact(err, "adopt", np.array_equal(got, merged), where)
        else:
            if capped and w0 is not None:
                val = [a - c for a, c in zip(val, w0[0])]; mag = [a + c for a, c in zip(mag, w0[1])]; adds += 1
            for e in range(9):
                if mag[e] > 0:
                    err.add("tr", abs(mp.mpf(float(got[e])) - val[e]) / (U * mag[e]) - adds, where + ("pcr_add", e))
            assert got[9] == float(val[9]), where
        if capped or w0 is None:
            assert np.array_equal(b["pcr_fix"][k], mpth["fix_before"]), (where, "pcr_fix untouched")
        else:
            for e in range(9):
                m_ = abs(fix0[e]) + w0[1][e]
                if m_ > 0:
                    err.add("tr", abs(mp.mpf(float(b["pcr_fix"][k, e])) - (fix0[e] + w0[0][e])) / (U * m_) - 1, where + ("pcr_fix", e))
            assert b["pcr_fix"][k, 9] == float(fix0[9] + w0[0][9]), where


def exact_margi_sums(ref, node, poses, variant=None):
    """(pcr_add, pcr_fix) margi leaves behind, the exact sums rounded once: what the reference continues from when it runs alone."""
    mpth = node.margi_path
    with mp.workprec(R.PREC):
        tr = [R.transform_exact(l, poses[j], variant=variant)[0] if l[9] != 0 else None for j, l in enumerate(mpth["locals"])]
        fix = [mp.mpf(v) for v in mpth["fix_before"]]
        add = list(fix)
        for t in tr:
            if t is not None:
                add = [a + c for a, c in zip(add, t)]
        if tr[0] is not None:
            if mpth["fix_before"][9] < ref.max_points:
                fix = [a + c for a, c in zip(fix, tr[0])]
            else:
                add = [a - c for a, c in zip(add, tr[0])]
        return [float(v) for v in add], [float(v) for v in fix]


def snapshot(ref):
    """The bit-for-bit part of the reference's state: the leaf table and every leaf's stored points."""
    lv = ref.leaves()
    pts = [[ref.leaf_points(n, which) for which in range(-1, ref.win_size)] for n in ref.leaf_nodes()]
    return lv, pts


def same_snapshot(a, b):
    (la, pa), (lb, pb) = a, b
    if not np.array_equal(la["node_id"], lb["node_id"]):
        return False
    for key in la:
        if key != "opt_state" and not np.array_equal(la[key], lb[key], equal_nan=True):
            return False
    if not np.array_equal(la["opt_state"] >= 0, lb["opt_state"] >= 0):
        return False
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for n1, n2 in zip(pa, pb) for x, y in zip(n1, n2))


def run(case, side, ref=None, old=None, variant=None, snaps=None):
    """Drives the case through the reference and `side` in lockstep; returns (ref, Errors).  `old`: a list that receives, per plane record, the
    figures the whole-array tolerances of tests/test_gpu_map.py would have looked at.  `variant`: one of R.VALUE_VARIANTS, degrading the exact replay
    (an honest side must then miss the criteria: the criteria tell the two apart).  side = None: the reference alone (it continues behind margi
    from the exact sums rounded once); `snaps` then receives its snapshot after every stage."""
    prm = case["prm"]
    ref = ref or R.RefMap(**prm)
    err = Errors()
    W = prm["win_size"]
    xs, wc = [], 0

    def stage(tag):
        if side is not None:
            return same_bits(ref, side, tag)
        if snaps is not None:
            snaps.append(snapshot(ref))
        return None, None

    for step, op in enumerate(case["ops"]):
        tag = (case["name"], step, op[0])
        if op[0] == "fix":
            _, w, v, jour = op
            ref.cut_voxel_fix(w, v, jour)
            if side is not None:
                side.m.cut_voxel_fix(w, v, jour)
            stage(tag)
            continue
        if op[0] == "release":
            _, jour_now, min_age, root = op
            if side is not None:
                got = side.m.release(jour_now, min_age)
                if got is None:                      # a side without journeys: it drops the root it is told to
                    if root is not None:
                        side.m.drop_root(root)
                else:
                    assert got["roots"] == (1 if root is not None else 0), (tag, got)
            if root is not None:
                ref.drop_root(root)
            stage(tag)
            continue
        _, body, var, pose = op
        xs.append(pose); wc += 1
        poses = np.stack(xs)
        pl = [[float(v) for v in p] for p in poses]
        pw = np.array([R.to_world([float(v) for v in pose], [float(v) for v in x]) for x in body])
        ref.cut_voxel(wc - 1, body, var, pw)
        if side is not None:
            side.f.clear()
            side.m.cut_voxel(wc - 1, body, var, pw)
        stage(tag + ("cut",))
        nref = ref.recut(wc, poses)
        if side is not None:
            side.m.recut(wc, poses, side.f)
            assert side.f.size() == nref, tag
        a, b = stage(tag + ("recut",))
        if side is not None:
            for k, n in enumerate(ref.leaf_nodes()):
                if n.judged == ref.stage:
                    check_eigen(err, b, k, tag + ("recut", hex(n.node_id)))
        if wc < W:
            continue
        ref.margi(wc, poses)
        ref.slide(1)
        caches = {}
        if side is not None:
            side.cache(poses)
            if side.f.size() > 0:
                ev_c, evec_c, mg_c = side.f.read_cache()
                caches = {int(i): (ev_c[o], evec_c[o], mg_c[o]) for i, o in zip(b["node_id"].tolist(), b["opt_state"].tolist()) if o >= 0}
            if hasattr(side.m, "set_journey"):
                side.m.set_journey(100.0)
            side.m.margi(wc, poses, side.f)
            side.m.slide(1)
        a, b = stage(tag + ("margi",))
        for k, n in enumerate(ref.leaf_nodes()):
            if n.margi_path is None or n.margi_path.get("stage") == "done":
                continue
            n.margi_path["stage"] = "done"
            if side is None:
                n.pcr_add, n.pcr_fix = exact_margi_sums(ref, n, pl)
                continue
            where = tag + ("margi", hex(n.node_id))
            check_margi_sums(err, ref, n, b, k, pl, where, variant=variant, cache=caches.get(int(n.node_id)))
            capped = not (n.margi_path["fix_before"][9] < ref.max_points)
            if not n.margi_path["adopt"] and n.is_plane and not capped:
                check_eigen(err, b, k, where)
            if n.updated:
                check_plane_record(err, b, k, where, variant=variant)
                if old is not None:
                    old.append(("pv", b, k, SimpleNamespace(margi_path=dict(n.margi_path)), pl))
            if old is not None and not n.margi_path["adopt"]:
                old.append(("tr", b, k, SimpleNamespace(margi_path=dict(n.margi_path)), pl))
            n.pcr_add, n.pcr_fix = [float(v) for v in b["pcr_add"][k]], [float(v) for v in b["pcr_fix"][k]]
        xs = xs[1:]; wc -= 1
    return ref, err


# ---- calibration ----------------------------------------------------------------------------------------------------------------------
def calibrate():
    total = Errors()
    for case in all_cases():
        for side in ([OracleSide(case["prm"])] if oracle_can_run(case) else []) + [HostSide(case["prm"])]:
            _, err = run(case, side)
            total.merge(err)
            print(f"{case['name']:24s} {side.name:7s}", {k: round(v[0], 2) for k, v in err.worst.items() if k not in EXACT})
    print("largest over the cases (units of u x magnitude):")
    for k, (r, w) in sorted(total.worst.items()):
        print(f"  {k:6s} {r:8.3f}   at {w}")


if __name__ == "__main__":
    if "--calibrate" in sys.argv:
        calibrate()
