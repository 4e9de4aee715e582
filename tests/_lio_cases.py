"""The cases on which the odometry update (csrc/vxba_lio.hip: lio_sweep_kernel, lio_ekf_kernel<0>, lio_var_init_kernel,
lio_pvec_update_kernel) is compared with exact arithmetic (tests/_lio_ref.py), the criteria, and the measured constants.

Test infrastructure only; tests/test_lio_cpu.py checks the cases, the criteria and a list of degraded variants without a GPU,
tests/test_gpu_lio_exact.py applies the criteria to the kernels.

Size ladder (`ladder`).  One map, synth.make_plane_map(n_roots=60, extent=2, max_layer=2, seed=5100) (voxel_size 1: voxel_size / 4 and its
halves are exact in float, so every face, descent centre and leaf box lies on the grid of step 1/4), one master scan of 262 145 rows; a scan
of size n is its first n rows, n in LADDER_N.  The launch is min(ceil8(ceil(n / 512)), 256) workgroups of 512 lanes: 1 is one lane, 63 / 64 /
65 a wave boundary, 511 / 512 / 513 a workgroup boundary (and 7 or 6 workgroups that exist only because of the round-up to 8 and hold no
point), 4096 / 4097 the step from 8 to 16 workgroups, 131 071 / 131 072 / 131 073 the first row any lane meets in a second pass of its loop,
262 145 two full passes plus one row of a third.  Two poses, A = the scan's propagated guess, B = its true pose; the sweeps are reset at A,
cached at B, reset at B.  Rows 0..4096 have exact (mpmath) terms, the rows above the float64 restatement's with math.fsum.

Honesty of the ladder.  A candidate row is dropped when at either pose a coordinate lies within GRID_MARGIN = 1e-6 (relative to max(|w|,
voxel_size)) of a plane of that grid, or when in any of the sweeps it is tested in (the three above and the reset sweep at A under the
mixed-scale covariance of the EKF cases) a gate comparison it reaches clears equality by less than GATE_MARGIN = 1e-6 relative.  Both are
1e-6 and not smaller because the index and both gates are float-typed (voxel_map.hpp:1340-1365, 1678-1685): a float rounds at 6e-8, and a row
that exact arithmetic decides one way with a 1e-6 margin is decided the same way by the float-typed code of either side.  The margins are
evaluated in float64 on quantities whose float64 error is below 1e-12 relative to the scales used, and again on the exact values of rows
0..4096 by the CPU test.  The share dropped must stay below 1 % (`Ladder.dropped`).

d(n), the longest chain of additions the kernel puts on one of the 34 sums (csrc/vxba_lio.hip).  A lane adds its terms into a register that
starts at 0.0: `passes` = ceil(n / (grid 512)) additions.  wave_reduce_scatter: one addition per butterfly step, 6 steps.  The 8 wave totals:
`t = red[0]; t += red[q]`, 7 additions.  Then the partials: the host path starts at 0.0 and adds `grid` of them, the first exactly: grid - 1;
lio_ekf_kernel adds up to 37 of them per chain from 0.0 (36 rounded) and then the 7 chains (6): 42.  d = passes + 6 + 7 + (grid - 1 | 42).
Every addition of non-negative-magnitude numbers loses at most u times the magnitude of its result, so d u A bounds the summation and
C_T u A the terms themselves (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).

Constants.  K_T, K_SIG: the largest error of the float64 restatement of a term / of sigma against mpmath, in units of u x magnitude, over
the exact rows of the ladder's four sweeps and the gate-edge scans.  K_EKF_STATE, K_EKF_COV: the largest error of the oracle's EKF
(oracle/vxo_lio.hpp) and of the host path's algebra with dm_inverse (tests/_lio_ref.ekf_f64, the float64 operations of
vxba_lio_state_estimation) against the exact replay, on the state and on the covariance, in units of u kappa_s mag, over EKF_CASES.  K_EIG: the oracle's smallest eigenvalue of nnt against the exact one, in units of u ||nnt||_2.
K_VI_*, K_PV_*: the oracle's var_init / pvec_update against mpmath over VARINIT_N.  All produced by
    python -m tests._lio_cases --calibrate
on CPU reference code, never on the device; every criterion uses C = 4 K, the factor 4 standing for contraction into FMA and another
association.  The figures are those of one toolchain (compiler of the oracle, libm, numpy); tests/test_lio_cpu.py asserts that the reference
code still measures at most SELF_CHECK K = 2 K, half of what the criteria allow, so that another toolchain's last digits do not fail it.

Magnitudes.  A term's magnitude is the same expression evaluated on absolute values with every subtraction an addition; 1 / (0.0005 + sigma)
enters with its first-order magnitude (1 / x)(sum |terms of x| / x).  In the EKF, mag_i = sum_j |K*_ij| |HTz_j| + vmag_i + sum_j |G*_ij| vmag_j
in exact quantities, summed over the iterations and multiplied by the condition number of the Jacobi-scaled S, with vmag the magnitude of
vec = x_prop [-] x_curr in the same sense as everywhere else: |x_prop_i| + |x_curr_i| for a vector component (one rounded subtraction of two
stored numbers; it also covers the rounded addition x_curr_i + solution_i), and for a rotation component
f (sum_k |R_ka| |R'_kb| + |R_kb| |R'_ka|), the two dot products whose difference Log takes.  The bias components start at zero, so their vmag
is |vec_i| itself.  With the VALUE |vec_i| in that place (ekf_exact(..., literal=True)) the oracle and the host algebra measure 342 and 376
u kappa mag on the two cases that start 3 cm off, 3 and 4 under the mixed covariance, and 9539 on the case that starts at the true pose, every
time on a velocity component: the velocity is stored at 0.5 m/s and rounded at u 0.5 by every x_curr [+]= solution, while its |vec| is the
1e-6 .. 1e-4 the update moves it, so that figure is the stored size over the step of the case and says nothing about the algebra.  With vmag
the same runs measure 0.04 .. 0.11 on all five cases, and the state has its own constant (K_EKF_STATE) beside the covariance's (K_EKF_COV)."""
import functools
import math
import sys

import numpy as np

from tests import _lio_ref as R
from voxel_slam_amd import synth

U = R.U64
MARGIN = 4.0

# ---- measured on CPU reference code: python -m tests._lio_cases --calibrate ---------------------------------------------------------------
K_T = 3.95                    # measured 3.948 (ladder, sweep at A)
K_SIG = 1.89                  # 1.889
# The covariance: 739.8 on (131073, scan), 253 on (4097, scan), 7 .. 14 on the mixed-scale covariance, on the off-diagonal of the pose block of
# (I - G) cov: G = K HTH is formed there from products of size 1 that cancel to 1e-4, so G carries u, not u |G|, and |G*| |cov| in the criterion's
# magnitude is 1e4 times smaller than what any float64 evaluation rounds.  The oracle and the host algebra show the same figure (739.7 / 739.8).
# The state: 0.1098 (host algebra on (131073, mixed)); 0.04 .. 0.10 elsewhere.
K_EKF_STATE = 0.11
K_EKF_COV = 740.0
K_EIG = 1.78                  # 1.778
K_VI_PNT, K_VI_VAR = 2.84, 6.77        # 2.836, 6.76
K_PV_PNT, K_PV_VAR = 2.45, 2.53        # 2.444, 2.528
C_T, C_SIG, C_EKF_STATE, C_EKF_COV, C_EIG = MARGIN * K_T, MARGIN * K_SIG, MARGIN * K_EKF_STATE, MARGIN * K_EKF_COV, MARGIN * K_EIG
SELF_CHECK = 2.0
C_VI_PNT, C_VI_VAR, C_PV_PNT, C_PV_VAR = MARGIN * K_VI_PNT, MARGIN * K_VI_VAR, MARGIN * K_PV_PNT, MARGIN * K_PV_VAR

LADDER_N = (1, 2, 63, 64, 65, 511, 512, 513, 4096, 4097, 131071, 131072, 131073, 262145)
N_MASTER = 262145
N_EXACT = 4097
N_RAW = 266000
BLOCK, MAX_GRID, NSUM = 512, 256, 34
EDGE_LANES = (0, 63, 64, 511, 512)
VARINIT_N = (1, 63, 64, 65, 257)
EKF_CASES = tuple((n, c) for n in (4097, 131073) for c in ("scan", "mixed")) + ((4097, "near"),)      # "near": from the true pose, out after two iterations
SCHEDULE_MARGIN = 1e-6


def grid_of(n):
    return min((-(-n // BLOCK) + 7) // 8 * 8, MAX_GRID)


def d_of(n, chain=False):
    g = grid_of(n)
    return -(-n // (g * BLOCK)) + 6 + 7 + (42 if chain else g - 1)


def mixed_cov():
    """Diagonals 1e-6, 1e-4, 1e-2, 1e-10, 1e-7 for rot, pos, vel, bg, ba and 0.3 correlations: D^1/2 (0.7 I + 0.3 1 1^T) D^1/2, symmetric
    positive definite by construction."""
    d = np.sqrt(np.repeat([1e-6, 1e-4, 1e-2, 1e-10, 1e-7], 3))
    C = 0.7 * np.eye(15) + 0.3 * np.ones((15, 15))
    cov = d[:, None] * C * d[None, :]
    return 0.5 * (cov + cov.T)


@functools.lru_cache(maxsize=None)
def plane_map():
    return synth.make_plane_map(n_roots=60, extent=2, max_layer=2, seed=5100)


def sym(var):
    return 0.5 * (var + np.transpose(var, (0, 2, 1)))


class Ladder:
    """pm, pnt (N_MASTER, 3), var (N_MASTER, 3, 3) exactly symmetric, state_a / state_b, cov, cov_mixed; leaf[k], sweep[k] for k = 0 (reset at A),
    1 (cached at B), 2 (reset at B), 3 (reset at A under cov_mixed); kept (the cache after sweep 0), dropped (share of candidate rows)."""

    def __init__(self):
        from tests import _oracle as O
        pm = self.pm = plane_map()
        self.index = mi = R.MapIndex(pm)
        assert mi.exact_grid()
        sc = synth.make_lio_scan(pm, n_points=N_RAW, seed=5101)
        o = O.LioOracle(pm.voxel_size, pm.max_layer); o.var_init(sc.xyz)
        pnt, var = o.read_points()
        var = sym(var)
        self.state_a, self.state_b, self.cov, self.cov_mixed = sc.state_init.copy(), sc.state_gt.copy(), sc.cov.copy(), mixed_cov()
        wa, wb = R.world(pnt, self.state_a), R.world(pnt, self.state_b)        # rows are independent: one pass over the candidates
        bad = (mi.grid_margin(wa) < R.GRID_MARGIN) | (mi.grid_margin(wb) < R.GRID_MARGIN)
        for s in self._sweeps(pnt, var, wa, wb, 0)[1]:
            bad |= s.margin < R.GATE_MARGIN
        first = np.nonzero(~bad)[0][:N_MASTER]
        assert first.size == N_MASTER
        self.dropped = float(1.0 - N_MASTER / (first[-1] + 1))
        self.pnt, self.var = np.ascontiguousarray(pnt[first]), np.ascontiguousarray(var[first])
        self.wa, self.wb = R.world(self.pnt, self.state_a), R.world(self.pnt, self.state_b)
        self.leaf, self.sweep = self._sweeps(self.pnt, self.var, self.wa, self.wb, N_EXACT)

    def _sweeps(self, p, v, wa, wb, n_exact):
        pm, mi = self.pm, self.index
        l0 = mi.lookup(wa)
        s0 = R.Sweep(pm, p, v, self.state_a, self.cov, l0, n_exact)
        self.kept = np.where(s0.flag, l0, -1)
        l1, self.still_inside = mi.cache_leaf(self.kept, wb)
        s1 = R.Sweep(pm, p, v, self.state_b, self.cov, l1, n_exact)
        l2 = mi.lookup(wb)
        s2 = R.Sweep(pm, p, v, self.state_b, self.cov, l2, n_exact, exact_from=s1)
        s3 = R.Sweep(pm, p, v, self.state_a, self.cov_mixed, l0, n_exact)
        return (l0, l1, l2, l0), (s0, s1, s2, s3)

    def k_constants(self):
        return max(s.k_term for s in self.sweep), max(s.k_sigma for s in self.sweep)


@functools.lru_cache(maxsize=None)
def ladder():
    return Ladder()


def make_pair(vx, pm, pnt, var, gpu=True):
    """(oracle, device estimator) loaded with the map and the ready points."""
    from tests import _oracle as O
    o = O.LioOracle(pm.voxel_size, pm.max_layer); o.map_update(*pm.args()); o.set_points(pnt, var)
    g = None
    if gpu:
        g = vx.LioEstimator(pm.voxel_size, pm.max_layer); g.map_update(*pm.args()); g.set_points(pnt, var)
    return o, g


# ---- gate edges ---------------------------------------------------------------------------------------------------------------------------
def edge_map():
    """One root (0, 0, 0) that is one plane: voxel_size 4, normal exactly (0, 0, 1), centre (2, 2, 2), radius 0.25, plane_var zero but
    [5][5] = 2^-10 (J[5] = -n_z = -1: the plane's part of sigma is 2^-10 whatever the point)."""
    pv = np.zeros((1, 6, 6)); pv[0, 5, 5] = 2.0 ** -10
    return synth.PlaneMapData(4.0, 0, np.zeros((1, 3), dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32),
                              np.full((1, 3), 2.0), np.array([[0.0, 0.0, 1.0]]), pv, np.array([0.25]), np.full((1, 3), 2.0), np.array([2.0]))


# name -> (offset of the point from the centre, variance diagonal, verdict).  sigma = 2^-10 + var_zz.
# range gate: dis_to_center - dis_to_plane^2 = dx^2 + dy^2 against 9 radius = 2.25 (`<=`); 1.5^2 = 2.25, and 2.25 + (2^-11)^2 is the next float.
# 3-sigma gate: var_zz = 3 2^-10 makes sigma = 2^-8 = 4^-4 and 3 sqrt(sigma) = 0.1875 (strict `<`).  |resi| = 0.1875 - 2^-30 is one step of
# 2^-30 inside in exact arithmetic; dis_to_plane is a float (voxel_map.hpp:1343), whose spacing at 0.1875 is 2^-26, so the reference's own code
# rounds that row back onto the boundary and rejects it.  The row stays, with the verdict the reference's typing gives it, and
# `sigma_in_f32` (one float step, 2^-26, inside) is the nearest row that passes.
EDGES = {
    "range_on": ((1.5, 0.0, 0.0), (2.0 ** -6, 2.0 ** -6, 2.0 ** -10), True),
    "range_up": ((1.5, 2.0 ** -11, 0.0), (2.0 ** -6, 2.0 ** -6, 2.0 ** -10), False),
    "sigma_on": ((0.25, 0.5, 0.1875), (2.0 ** -6, 2.0 ** -6, 3 * 2.0 ** -10), False),
    "sigma_in": ((0.25, 0.5, 0.1875 - 2.0 ** -30), (2.0 ** -6, 2.0 ** -6, 3 * 2.0 ** -10), False),
    "sigma_in_f32": ((0.25, 0.5, -(0.1875 - 2.0 ** -26)), (2.0 ** -6, 2.0 ** -6, 3 * 2.0 ** -10), True),
}
EDGE_NAMES = tuple(EDGES)
EDGE_STATE = np.concatenate([np.eye(3).reshape(9), np.zeros(12), [0.0, 0.0, -9.8]])


def edge_cov():
    cov = np.zeros((15, 15)); cov[6:, 6:] = np.eye(9) * 1e-4        # zero rot / tsl blocks
    return cov


@functools.lru_cache(maxsize=None)
def edge_scan(shift):
    """513 rows on the edge map: good rows (dyadic offsets well inside both gates) with an edge row at each lane position of EDGE_LANES,
    row EDGE_LANES[j] holding edge (j + shift) mod 5.  Returns (pnt, var, verdicts, names per row or None)."""
    n = 513
    a = np.arange(n)
    off = np.stack([((a % 17) - 8) / 16.0, ((a % 13) - 6) / 16.0, ((a % 5) - 2) / 64.0], axis=1)
    vd = np.tile([2.0 ** -6, 2.0 ** -6, 2.0 ** -10], (n, 1))
    verdict = np.ones(n, dtype=bool)
    names = [None] * n
    for j, lane in enumerate(EDGE_LANES):
        nm = EDGE_NAMES[(j + shift) % len(EDGE_NAMES)]
        off[lane], vd[lane], verdict[lane] = EDGES[nm]
        names[lane] = nm
    var = np.zeros((n, 3, 3)); var[:, 0, 0], var[:, 1, 1], var[:, 2, 2] = vd[:, 0], vd[:, 1], vd[:, 2]
    return 2.0 + off, var, verdict, names


@functools.lru_cache(maxsize=None)
def edge_sweep(shift):
    pm = edge_map()
    pnt, var, verdict, names = edge_scan(shift)
    leaf = R.MapIndex(pm).lookup(R.world(pnt, EDGE_STATE))
    return R.Sweep(pm, pnt, var, EDGE_STATE, edge_cov(), leaf, n_exact=513)


# ---- rows that must contribute nothing ------------------------------------------------------------------------------------------------------
NOTHING = ("nan", "+inf", "-inf", "3e6", "1e30", "-0.0", "nan_var")
FAR = 1000.0        # inside the index range of the map's table, outside the map


def nothing_scan(shift):
    """The ladder's first 513 rows with a special row at positions 0, 63, 64, 511 and 512 = n - 1 (kind (j + shift) mod 7 at the j-th), and the
    same scan with every such row replaced: by the finite point (FAR, FAR, FAR) with a unit variance, which matches nothing, or for "-0.0"
    by the same row with +0.0 (a zero's sign must not matter; that row is an ordinary point and may match).  (pnt, var, pnt_sub, var_sub, kinds)."""
    L = ladder()
    pnt, var = L.pnt[:513].copy(), L.var[:513].copy()
    base = int(np.nonzero(L.sweep[0].flag[:513] & ~np.isin(np.arange(513), EDGE_LANES))[0][0])     # a row that matches at pose A
    pnt[list(EDGE_LANES)], var[list(EDGE_LANES)] = pnt[base], var[base]
    ps, vs = pnt.copy(), var.copy()
    kinds = {}
    for j, row in enumerate(EDGE_LANES):
        kind = NOTHING[(j + shift) % len(NOTHING)]
        kinds[row] = kind
        ax = (j + shift) % 3
        if kind == "nan_var":
            var[row, ax, ax] = np.nan
        else:
            pnt[row, ax] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "3e6": 3e6, "1e30": 1e30, "-0.0": -0.0}[kind]
        if kind == "-0.0":
            ps[row, ax] = 0.0
        else:
            ps[row] = FAR; vs[row] = np.eye(3)
    return pnt, var, ps, vs, kinds


# ---- the node cache on a shared face -------------------------------------------------------------------------------------------------------
def face_case():
    """Two roots (0,0,0) and (1,0,0) of voxel_size 4, each one plane with normal (0, 0, 1): the lower with radius 0.25, the upper with radius 1.
    One point (3, 2, 2) under three translations, identity rotation: sweep 1 (reset) puts it at (3, 2, 2), inside the lower leaf and matched;
    sweep 2 (cached) at (4, 2, 2.5), ON the shared face -- OctoTree::inside is closed, so the lower leaf is tested, and |resi| = 0.5 fails;
    sweep 3 (cached) at (4, 2, 2): the reference still holds the lower leaf (`oc` is written on a match only) and its range gate fails
    (4 > 2.25), while a fresh lookup -- the float-typed index of x = 4 is 1 -- would test the upper leaf and match (4 <= 9).
    Returns (pm, pnt, var, [state 1, 2, 3], cov, verdicts (True, False, False))."""
    pv = np.zeros((2, 6, 6)); pv[:, 5, 5] = 2.0 ** -10
    c = np.array([[2.0, 2.0, 2.0], [6.0, 2.0, 2.0]])
    pm = synth.PlaneMapData(4.0, 0, np.array([[0, 0, 0], [1, 0, 0]], dtype=np.int64), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.ones(2, dtype=np.int32),
                            c, np.tile([0.0, 0.0, 1.0], (2, 1)), pv, np.array([0.25, 1.0]), c.copy(), np.array([2.0, 2.0]))
    st = [EDGE_STATE.copy() for _ in range(3)]
    st[1][9:12] = [1.0, 0.0, 0.5]; st[2][9:12] = [1.0, 0.0, 0.0]
    var = np.diag([2.0 ** -6, 2.0 ** -6, 2.0 ** -10])[None]
    return pm, np.array([[3.0, 2.0, 2.0]]), var, st, edge_cov(), (True, False, False)


def cache_model(pm, pnt, var, states, cov, overwrite=False):
    """Verdicts of a reset sweep followed by cached ones, by the reference's rule (`oc` written on a match only); overwrite=True: the cache is
    set to -1 for a point that fails under the cache (a degraded variant)."""
    mi = R.MapIndex(pm)
    cache = np.full(pnt.shape[0], -1)
    out = []
    for k, st in enumerate(states):
        w = R.world(pnt, st)
        leaf = mi.lookup(w) if k == 0 else mi.cache_leaf(cache, w)[0]
        s = R.Sweep(pm, pnt, var, st, cov, leaf)
        cache = np.where(s.flag, leaf, -1 if (k == 0 or overwrite) else cache)
        out.append(s.flag.copy())
    return out


# ---- var_init / pvec_update -----------------------------------------------------------------------------------------------------------------
VI_EXT_R = synth.rodrigues(np.array([0.01, -0.02, 0.03]))
VI_EXT_P = np.array([0.04, 0.02, -0.03])
VI_ERR = (0.02, 0.05)


def varinit_scan(n):
    """n float32 sensor points; the last rows (as many as fit) are a point with z = 0, one on each axis, one 1 cm from the sensor, one at 200 m."""
    rng = np.random.default_rng(5300 + n)
    xyz = (rng.normal(size=(n, 3)) * [8.0, 8.0, 2.0]).astype(np.float32)
    special = np.array([[3.0, -4.0, 0.0], [5.0, 0.0, 0.0], [0.0, -7.0, 0.0], [0.0, 0.0, 2.5], [0.006, -0.007, 0.004], [120.0, -150.0, 55.0]], dtype=np.float32)
    k = min(n, len(special))
    start = (n % len(special)) if n < len(special) else 0
    xyz[n - k:] = np.roll(special, -start, axis=0)[:k]
    return xyz


@functools.lru_cache(maxsize=None)
def varinit_reference(n):
    """Exact var_init of varinit_scan(n) and exact pvec_update of ITS float64 rounding at the ladder's pose A, with magnitudes:
    dict(pnt, var, wld, wvar: each (hi, lo, mag))."""
    xyz = varinit_scan(n)
    with R.mp.workprec(R.PREC):
        vp, vv, norms = R.var_init_terms(xyz, VI_EXT_R, VI_EXT_P, *VI_ERR)
        mp_, mv_, _ = R.var_init_terms(xyz, VI_EXT_R, VI_EXT_P, *VI_ERR, norms=norms)
        ep, ev, _ = R.var_init_terms(xyz, VI_EXT_R, VI_EXT_P, *VI_ERR, exact=True)
        out = dict(pnt=R.split_hi_lo(ep) + (mp_,), var=R.split_hi_lo(ev) + (mv_,), f64=(vp, vv))
    return out


def pvec_pose():
    sc_state = np.concatenate([synth.rodrigues(np.array([0.02, -0.03, 0.4])).T.reshape(9), [0.3, -0.2, 0.1], [0.5, 0.1, 0.0], np.zeros(6), [0.0, 0.0, -9.8]])
    return sc_state, mixed_cov() + np.eye(15) * 1e-5


def pvec_reference(pnt, var):
    """Exact pvec_update of the GIVEN points (what the side under test itself holds after var_init): dict(wld, wvar: (hi, lo, mag))."""
    st, cov = pvec_pose()
    with R.mp.workprec(R.PREC):
        ew, ev = R.pvec_terms(pnt, var, st, cov, exact=True)
        mw, mv = R.pvec_terms(pnt, var, st, cov, mag=True)
        return dict(wld=R.split_hi_lo(ew) + (mw,), wvar=R.split_hi_lo(ev) + (mv,))


def ratio(x, ref):
    hi, lo, mag = ref
    return float(R.err_units(np.asarray(x, dtype=np.float64), hi, lo, mag).max())


def check_varinit(side, n, consts=None, label=""):
    """var_init of varinit_scan(n) and pvec_update on `side` (oracle or device estimator) against mpmath; returns the four ratios."""
    c = (C_VI_PNT, C_VI_VAR, C_PV_PNT, C_PV_VAR) if consts is None else consts
    side.var_init(varinit_scan(n), VI_EXT_R, VI_EXT_P, *VI_ERR)
    pnt, var = side.read_points()
    ref = varinit_reference(n)
    k = [ratio(pnt, ref["pnt"]), ratio(sym(var), ref["var"])]
    st, cov = pvec_pose()
    wld, wvar = side.pvec_update(st, cov)
    pr = pvec_reference(pnt, sym(var))
    k += [ratio(wld, pr["wld"]), ratio(wvar, pr["wvar"])]
    if label:
        print(f"  {label} n={n}: var_init pnt {k[0]:.3g} ({c[0]:.3g}) var {k[1]:.3g} ({c[1]:.3g})  pvec_update pnt {k[2]:.3g} ({c[2]:.3g}) var {k[3]:.3g} ({c[3]:.3g})")
    for v, b, what in zip(k, c, ("var_init point", "var_init covariance", "pvec_update point", "pvec_update covariance")):
        assert v <= b, f"{what}: |err| / (u mag) = {v:.4g} > {b:.4g}"
    return k


# ---- sweep criteria -------------------------------------------------------------------------------------------------------------------------
def check_sums(s34, sw, n, d, c_t=None, label=""):
    """The 34 sums of a sweep over the first n rows against the reference sweep `sw`: count exact, a sum without terms exactly 0.0,
    |S - S*| <= (c_t + d) u A.  Returns the largest |S - S*| / (u A)."""
    c_t = C_T if c_t is None else c_t
    S, Lo, A = sw.sums(n)
    s34 = np.asarray(s34, dtype=np.float64)
    assert s34[33] == S[33], f"match_num {s34[33]:.0f}, exact {S[33]:.0f}"
    assert not np.any(s34[A == 0] != 0.0), "a sum without terms is not exactly 0.0"
    k = R.err_units(s34, S, Lo, A)
    km = float(k.max())
    if label:
        print(f"  {label}: n={n} sums {km:.3g} u A at {int(np.argmax(k))} (bound {c_t:.3g} + {d})")
    assert km <= c_t + d, f"sum {int(np.argmax(k))}: |S - S*| / (u A) = {km:.4g} > {c_t:.4g} + {d}"
    return km


def check_points(res, sw, n, c_sig=None, label=""):
    """Match mask exact, -1 / 0.0 on unmatched rows, one record per leaf, sigma within c_sig u magnitude."""
    c_sig = C_SIG if c_sig is None else c_sig
    pop, sig = res["plane_of_point"], res["sigma_of_point"]
    flag = sw.flag[:n]
    assert np.array_equal(pop >= 0, flag), f"match mask differs at rows {np.nonzero((pop >= 0) != flag)[0][:8]}"
    assert np.all(pop[~flag] == -1) and not np.any(sig[~flag] != 0.0)
    pairs = np.unique(np.stack([sw.leaf[:n][flag], pop[flag]], axis=1), axis=0) if flag.any() else np.zeros((0, 2), dtype=np.int64)
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])), "records and leaves are not one to one"
    k = R.err_units(sig, sw.sigma_hi[:n], sw.sigma_lo[:n], sw.sig_mag[:n])
    km = float(k.max()) if n else 0.0
    if label:
        print(f"  {label}: n={n} sigma {km:.3g} u M (bound {c_sig:.3g})")
    assert km <= c_sig, f"sigma_of_point: {km:.4g} u M > {c_sig:.4g} at row {int(np.argmax(k))}"
    return km


def old_check_sweep(a, b, tol=1e-10):
    """tests/test_gpu_lio.py::check_sweep as a predicate."""
    rel = lambda x, y: np.abs(x - y).max() / max(np.abs(y).max(), 1e-300)
    return bool(a["match_num"] == b["match_num"] and rel(a["HTH"], b["HTH"]) < tol and rel(a["HTz"], b["HTz"]) < 1e3 * tol and rel(a["nnt"], b["nnt"]) < tol)


def pack34(s34):
    """34 sums -> a sweep dict."""
    H = np.zeros((6, 6)); N = np.zeros((3, 3))
    for k, (r, c) in enumerate(R.TRI6):
        H[r, c] = H[c, r] = s34[k]
    for k, (r, c) in enumerate(R.TRI3):
        N[r, c] = N[c, r] = s34[27 + k]
    return dict(HTH=H, HTz=np.array(s34[21:27]), nnt=N, match_num=int(s34[33]))


# ---- numpy model of the kernel's data flow (for the degraded variants) ------------------------------------------------------------------------
def device_sums(terms, n, chain=False, variant=None):
    """The 34 sums as lio_sweep_kernel and its caller form them from per-row terms (zero rows where unmatched): lane registers over the
    passes, butterfly (strides 32 .. 1), the 8 waves in order, then the partials in index order (host path) or as 7 chains x 37 slots.
    variant: None, ("drop_partial", b), ("lane63", b, wave), "skip_pass2", ("chain_stop", slot)."""
    g = grid_of(n)
    per = g * BLOCK
    passes = -(-n // per)
    t = np.zeros((passes * per, NSUM)); t[:n] = terms[:n]
    t = t.reshape(passes, g, BLOCK, NSUM)
    lane = np.zeros((g, BLOCK, NSUM))
    for q in range(passes):
        if variant == "skip_pass2" and q == 1:
            continue
        lane = lane + t[q]
    w = lane.reshape(g, 8, 64, NSUM).copy()
    if isinstance(variant, tuple) and variant[0] == "lane63":
        w[variant[1], variant[2], 63] = 0.0
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :off] + w[:, :, off:2 * off]
    w = w[:, :, 0]
    part = w[:, 0].copy()
    for q in range(1, 8):
        part = part + w[:, q]
    if isinstance(variant, tuple) and variant[0] == "drop_partial":
        part[variant[1]] = 0.0
    if not chain:
        out = np.zeros(NSUM)
        for b in range(g):
            out = out + part[b]
        return out
    stop = variant[1] if isinstance(variant, tuple) and variant[0] == "chain_stop" else 7 * 37
    fin = np.zeros((7, NSUM))
    for q in range(37):
        for ch in range(7):
            b = ch + q * 7
            fin[ch] = fin[ch] + (part[b] if b < g and b < stop else 0.0)
    out = fin[0].copy()
    for ch in range(1, 7):
        out = out + fin[ch]
    return out


# ---- EKF ------------------------------------------------------------------------------------------------------------------------------------
def ekf_inputs(case):
    n, which = case
    L = ladder()
    if which == "near":
        return n, L.state_b, L.cov, L.sweep[2]
    return n, L.state_a, (L.cov if which == "scan" else L.cov_mixed), (L.sweep[0] if which == "scan" else L.sweep[3])


def ekf_ratios(got, ex):
    """(state, cov, min_eig) errors of an estimation result against its exact replay `ex`, in units of u kappa mag / u kappa mag / u ||nnt||."""
    es = R.state_error(got["state"], ex)
    with np.errstate(divide="ignore", invalid="ignore"):
        ks = np.where(ex["bound_state"] > 0, es / (U * ex["bound_state"]), np.where(es == 0, 0.0, np.inf))
    kc = R.err_units(got["cov"], ex["cov"], ex["cov_lo"], ex["bound_cov"])
    ke = float(abs(R.mpf(float(got["min_eig"])) - ex["min_eig"])) / (U * ex["nnt_norm"])
    return ks, kc, ke


def check_ekf(got, state, cov, c_state=None, c_cov=None, c_eig=None, label=""):
    """An estimation result (dict of LioEstimator.lio_state_estimation) against the exact replay from its own sweeps."""
    c_state = C_EKF_STATE if c_state is None else c_state
    c_cov = C_EKF_COV if c_cov is None else c_cov
    c_eig = C_EIG if c_eig is None else c_eig
    ex = R.ekf_exact(state, cov, got["sweeps"])
    assert ex["finished"] and got["iterations"] == ex["iterations"], "the exact schedule does not stop where the result did"
    assert float(ex["margin"]) >= SCHEDULE_MARGIN, f"a schedule decision has a margin of {float(ex['margin']):.3g}"
    assert got["match_num"] == got["sweeps"][-1]["match_num"] and got["ok"] == (not ex["min_eig"] < 14)
    ks, kc, ke = ekf_ratios(got, ex)
    if label:
        print(f"  {label}: iterations {ex['iterations']} rematch {ex['rematch']} kappa {max(ex['kappa']):.3g}  state {ks.max():.3g} at {int(np.argmax(ks))}  "
              f"(bound {c_state:.3g})  cov {kc.max():.3g} at {tuple(int(v) for v in np.unravel_index(np.argmax(kc), kc.shape))} (bound {c_cov:.3g})  min_eig {ke:.3g} (bound {c_eig:.3g})")
    assert ks.max() <= c_state, f"state component {int(np.argmax(ks))}: {ks.max():.4g} u kappa mag > {c_state:.4g}"
    assert kc.max() <= c_cov, f"covariance entry {np.unravel_index(np.argmax(kc), kc.shape)}: {kc.max():.4g} u kappa mag > {c_cov:.4g}"
    assert ke <= c_eig, f"min_eig: {ke:.4g} u ||nnt|| > {c_eig:.4g}"
    return float(ks.max()), float(kc.max()), ke, ex


def old_check_state(got, ref):
    """The state / covariance tolerances of tests/test_gpu_lio.py::test_state_estimation_matches_oracle as a predicate."""
    et, er = synth.pose_errors(got["state"][None, :12], ref["state"][None, :12])
    rel = np.abs(got["cov"] - ref["cov"]).max() / np.abs(ref["cov"]).max()
    return bool(et < 1e-9 and er < 1e-9 and np.allclose(got["state"][12:], ref["state"][12:], atol=1e-10) and rel < 1e-8)


# ---- calibration ----------------------------------------------------------------------------------------------------------------------------
def oracle_ekf(case):
    """The oracle's lio_state_estimation on an EKF case: (result, state, cov)."""
    n, state, cov, _ = ekf_inputs(case)
    L = ladder()
    o, _ = make_pair(None, L.pm, L.pnt[:n], L.var[:n], gpu=False)
    return o.lio_state_estimation(state, cov), state, cov


def measure():
    out = {}
    L = ladder()
    kt, ks = L.k_constants()
    for sh in range(len(EDGE_NAMES)):
        s = edge_sweep(sh)
        kt, ks = max(kt, s.k_term), max(ks, s.k_sigma)
    out["K_T"], out["K_SIG"] = kt, ks
    ke = kc_ = kg = 0.0
    for case in EKF_CASES:
        got, state, cov = oracle_ekf(case)
        ex = R.ekf_exact(state, cov, got["sweeps"])
        a, b, c = ekf_ratios(got, ex)
        h = R.ekf_f64(state, cov, got["sweeps"])
        h["min_eig"] = got["min_eig"]
        a2, b2, _ = ekf_ratios(h, ex)
        print(f"  {case}: oracle state {a.max():.4g} cov {b.max():.4g} min_eig {c:.4g}; host algebra with dm_inverse state {a2.max():.4g} cov {b2.max():.4g}; kappa {max(ex['kappa']):.4g}", flush=True)
        print(f"      iterations {ex['iterations']} rematch {ex['rematch']} margin {float(ex['margin']):.3g}; state worst at component {int(np.argmax(a))} / {int(np.argmax(a2))}")
        ke = max(ke, a.max(), a2.max()); kc_ = max(kc_, b.max(), b2.max()); kg = max(kg, c)
    out["K_EKF_STATE"], out["K_EKF_COV"], out["K_EIG"] = float(ke), float(kc_), kg
    from tests import _oracle as O
    k4 = np.zeros(4)
    for n in VARINIT_N:
        k4 = np.maximum(k4, check_varinit(O.LioOracle(), n, consts=(np.inf,) * 4))
    out["K_VI_PNT"], out["K_VI_VAR"], out["K_PV_PNT"], out["K_PV_VAR"] = (float(v) for v in k4)
    return out


def _main(argv):
    if "--calibrate" not in argv:
        return 2
    for k, v in measure().items():
        print(f"{k} = {v:.4g}")
    print(f"dropped rows: {ladder().dropped:.3%}")
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
