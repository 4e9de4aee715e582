"""IMUEKF (raw scan + raw IMU in front of the odometry), CPU side: the checker (tests/_imuekf_ref.py) against mathematics, the host build of
csrc/vxba_imuekf_math.hpp against the checker, and the honesty of every input tests/test_gpu_imuekf.py uses -- the checker alone meets each condition
that the GPU tests impose on the product."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _imuekf_ref as E
from tests._init_ref import exp_rate, so3_exp

HERE = os.path.dirname(os.path.abspath(__file__))
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
G = np.array([0.0, 0.0, -9.8])


def ready_filter(last_end=100.0, last_stamp=None, gyr=np.zeros(3), acc=np.zeros(3), **kw):
    """A checker that is initialised, by its fields."""
    f = E.ImuEkfRef(**kw)
    f.init_flag, f.init_num = True, 31
    f.last_pcl_end_time = last_end
    f.last_imu = (last_end if last_stamp is None else last_stamp, np.asarray(gyr, dtype=np.float64), np.asarray(acc, dtype=np.float64))
    return f


def state_of(R, p, v, bg=np.zeros(3), ba=np.zeros(3), g=G):
    return np.concatenate([R.T.reshape(9), p, v, bg, ba, g])


ONE_POINT = (np.ones((1, 3), dtype=np.float32), np.zeros(1, dtype=np.float32))


# ---- the checker against mathematics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 21])
def test_closed_form_motions(K):
    """Zero rate with a constant force: p = p0 + v0 T + (R a + g) T^2 / 2.  Constant rate: R = R0 Exp(w T).  Tolerance 64 K 2^-52 max(1, |x|)."""
    R0 = so3_exp(np.array([0.1, 0.2, -0.1])); p0 = np.array([0.5, -0.2, 0.1]); v0 = np.array([1.0, -0.5, 0.3])
    bg = np.array([0.01, -0.02, 0.005]); ba = np.array([0.05, 0.02, -0.03])
    a = np.array([0.3, -0.2, 9.9]); w = np.array([0.4, -0.3, 0.5])
    stamps = 100.0 + 0.1 * np.arange(1, K + 1) / K
    for end in (stamps[-1] + 0.002, stamps[-1] - 0.002):
        T = end - 100.0
        f = ready_filter(gyr=bg, acc=a + ba)
        r = f.process(state_of(R0, p0, v0, bg, ba), np.eye(15) * 1e-4, ONE_POINT, (stamps, np.tile(bg, (K, 1)), np.tile(a + ba, (K, 1))), 100.0, end)
        x = E.unpack(r["state"])
        acc_w = R0 @ a + G
        want_p = p0 + v0 * T + 0.5 * acc_w * T * T
        if end < stamps[-1]:                                               # note = -1: upstream steps back with - a dt^2 / 2 where the parabola has +; kept
            d = stamps[-1] - end
            want_p = want_p - acc_w * d * d
        assert (np.abs(x["p"] - want_p) <= E.tol(K + 1, want_p)).all()
        assert (np.abs(x["v"] - (v0 + acc_w * T)) <= E.tol(K + 1, v0 + acc_w * T)).all()
        assert np.array_equal(x["R"], R0)
        f = ready_filter(gyr=w + bg, acc=ba)
        r = f.process(state_of(R0, p0, v0, bg, ba), np.eye(15) * 1e-4, ONE_POINT, (stamps, np.tile(w + bg, (K, 1)), np.tile(ba, (K, 1))), 100.0, end)
        want_R = R0 @ exp_rate(w, T)
        assert (np.abs(E.unpack(r["state"])["R"] - want_R) <= E.tol(K + 1, want_R)).all()


def _mean_step(x, d, rate_m, acc_m, dt):
    """One step of the mean propagation from x [+] d, returned as the error state against the unperturbed step."""
    def run(dd):
        R = x["R"] @ so3_exp(dd[0:3]); p = x["p"] + dd[3:6]; v = x["v"] + dd[6:9]; bg = x["bg"] + dd[9:12]; ba = x["ba"] + dd[12:15]
        w = rate_m - bg; a = acc_m - ba
        acc_imu = R @ a + x["g"]
        return R @ exp_rate(w, dt), p + v * dt + 0.5 * acc_imu * dt * dt, v + acc_imu * dt, bg, ba
    from tests._init_ref import so3_log
    R1, p1, v1, bg1, ba1 = run(d)
    R0, p0, v0, bg0, ba0 = run(np.zeros(15))
    return np.concatenate([so3_log(R0.T @ R1), p1 - p0, v1 - v0, bg1 - bg0, ba1 - ba0])


def test_F_x_against_central_differences():
    """Every block upstream's F_x holds, against central differences of the checker's own mean step, 1e-6 relative (per block: max |diff| / max |block|).
    (0,0), (3,6), (6,0), (6,12) are exact derivatives of the step.  (0,9) = -I dt is the derivative only to first order in |rate| dt (the exact one is
    -Jr(rate dt) dt): it is compared at zero rate, where Jr = I, and at a non-zero rate it may be off by |rate| dt / 2 relative, the first neglected
    term of Jr.  The step's second-order dependencies that upstream's F_x leaves at zero (p on rot and ba, through a dt^2 / 2) are bounded likewise."""
    R = so3_exp(np.array([0.3, -0.2, 0.5]))
    x = dict(R=R, p=np.array([1.0, 2.0, 3.0]), v=np.array([0.5, -1.0, 0.2]), bg=np.array([0.01, -0.02, 0.005]), ba=np.array([0.05, 0.02, -0.03]), g=G)
    acc_m = np.array([0.4, -0.3, 9.7]); dt = 0.005; h = 1e-5
    for rate_m, first_order in ((x["bg"].copy(), False), (np.array([0.4, -0.3, 0.5]), True)):
        w, a = rate_m - x["bg"], acc_m - x["ba"]
        F, _ = E.step_matrices(R, w, a, dt, np.ones(3), np.ones(3), np.ones(3), np.ones(3))
        J = np.zeros((15, 15))
        for k in range(15):
            d = np.zeros(15); d[k] = h
            J[:, k] = (_mean_step(x, d, rate_m, acc_m, dt) - _mean_step(x, -d, rate_m, acc_m, dt)) / (2 * h)
        rel = lambda r, c: np.abs(F[r:r + 3, c:c + 3] - J[r:r + 3, c:c + 3]).max() / np.abs(J[r:r + 3, c:c + 3]).max()
        for r, c in ((0, 0), (3, 6), (6, 0), (6, 12), (3, 3), (6, 6), (9, 9), (12, 12)):
            assert rel(r, c) < 1e-6, (r, c, rel(r, c))
        if first_order:
            assert rel(0, 9) <= 0.5 * np.linalg.norm(w) * dt * 1.01
        else:
            assert rel(0, 9) < 1e-6
        assert np.abs(J[3:6, 0:3]).max() <= 0.5 * np.linalg.norm(a) * dt * dt * 1.01 and np.abs(J[3:6, 12:15]).max() <= 0.5 * dt * dt * 1.01
        Z = J.copy()
        for r, c in ((0, 0), (3, 6), (6, 0), (6, 12), (3, 3), (6, 6), (9, 9), (12, 12), (0, 9), (3, 0), (3, 12)):
            Z[r:r + 3, c:c + 3] = 0
        assert np.abs(Z).max() < 1e-9                                      # nothing else depends on anything


def test_cov_symmetric_and_exact_when_F_is_identity():
    """cov stays symmetric; a pair with dt = 0 has F = I and cov_w = 0 and leaves cov bit for bit; any step adds exactly cov_w to F cov F^T."""
    cov0 = E.moving_cov()
    f = ready_filter(gyr=[0.4, -0.3, 0.5], acc=[0.1, 0.2, 9.8])
    K = 5
    stamps = np.array([100.0, 100.0, 100.0, 100.0, 100.0])                 # every pair: cur_time = 100, dt = 0
    r = f.process(E.moving_state(G), cov0, ONE_POINT, (stamps, np.tile([0.4, -0.3, 0.5], (K, 1)), np.tile([0.1, 0.2, 9.8], (K, 1))), 100.0, 100.0)
    assert r["heads"] == K and np.array_equal(r["cov"], cov0)
    f = ready_filter(gyr=[0.4, -0.3, 0.5], acc=[0.1, 0.2, 9.8])
    c = E.make_case(3, 21, seed=3)
    r = f.process(E.moving_state(G), cov0, c["scan"], c["imus"], c["beg"], c["end"])
    assert (np.abs(r["cov"] - r["cov"].T) <= E.tol(21, r["cov"])).all()
    assert np.linalg.eigvalsh(0.5 * (r["cov"] + r["cov"].T)).min() > 0
    Rm = so3_exp(np.array([0.3, -0.2, 0.5]))
    F, W = E.step_matrices(Rm, np.array([0.4, -0.3, 0.5]), np.array([0.1, 0.2, 9.8]), 0.005, np.full(3, 0.1), np.full(3, 0.2), np.full(3, 1e-4), np.full(3, 2e-4))
    assert np.array_equal(W, W.T) or np.abs(W - W.T).max() < 1e-20
    assert np.allclose(np.diag(W)[0:3], 0.2 * 0.005 ** 2) and np.allclose(np.diag(W)[9:12], 1e-4 * 0.005 ** 2) and np.allclose(np.diag(W)[12:15], 2e-4 * 0.005 ** 2)
    assert np.allclose(W[6:9, 6:9], 0.1 * 0.005 ** 2 * np.eye(3), atol=1e-20) and not W[3:6].any()


@pytest.mark.parametrize("end_after", [True, False])
def test_skipped_pairs_clamped_time_and_note(end_after):
    """Messages before the last scan end are skipped, the first surviving head's time is clamped to it: a constant-force motion lands on the closed form
    with T measured from the last scan end, whichever side of the last message the scan ends on."""
    R0 = so3_exp(np.array([0.1, 0.2, -0.1])); p0 = np.array([0.5, -0.2, 0.1]); v0 = np.array([1.0, -0.5, 0.3]); a = np.array([0.3, -0.2, 9.9])
    f = ready_filter(last_end=100.0, last_stamp=99.99, acc=a)
    stamps = np.array([99.992, 99.996, 99.999, 100.004, 100.03, 100.05])
    end = 100.06 if end_after else 100.045
    r = f.process(state_of(R0, p0, v0), np.eye(15) * 1e-4, ONE_POINT, (stamps, np.zeros((6, 3)), np.tile(a, (6, 1))), 100.0, end)
    tab = f.pose_table()
    assert r["heads"] == 3 and tab[0, 0] == 0.0 and np.allclose(tab[1:, 0], [100.004 - 100.0, 100.03 - 100.0], atol=1e-12)      # head 0 clamped: offt = 0
    T = end - 100.0
    want = p0 + v0 * T + 0.5 * (R0 @ a + G) * T * T
    if not end_after:
        want = want - (R0 @ a + G) * (100.05 - end) ** 2                   # note = -1: upstream's - a dt^2 / 2, see test_closed_form_motions
    assert (np.abs(E.unpack(r["state"])["p"] - want) <= E.tol(4, want)).all()
    assert f.last_imu[0] == 100.05 and f.last_pcl_end_time == end and r["imus"][0][0] == 100.0 and r["imus"][0][-1] == end


def test_imu_init_recurrence_and_flag():
    """The recurrence against its closed form: the arithmetic mean of all messages so far (divisors 2, 3, ... after the first), init_num = count + 1,
    over calls; the flag flips at the call that makes init_num > 30."""
    rng = np.random.default_rng(1)
    f = E.ImuEkfRef()
    seen = []
    st = np.concatenate([np.eye(3).reshape(9), np.zeros(15)])
    t = 0.0
    for call, K in enumerate((7, 11, 11, 4, 3)):
        imus = (t + 0.01 * np.arange(1, K + 1), rng.normal(size=(K, 3)), np.array([0.0, 0.0, 1.0]) + 0.01 * rng.normal(size=(K, 3)))
        t += 0.01 * K
        was = f.init_flag
        r = f.process(st, np.eye(15), ONE_POINT, imus, t - 0.01 * K, t)
        if was:
            assert r["ready"]
            break
        seen.append(imus)
        acc = np.concatenate([s[2] for s in seen]); gyr = np.concatenate([s[1] for s in seen])
        assert not r["ready"] and f.init_num == acc.shape[0] + 1
        assert np.abs(f.mean_acc - acc.mean(axis=0)).max() < 64 * acc.shape[0] * 2.0 ** -52 and np.abs(f.mean_gyr - gyr.mean(axis=0)).max() < 64 * acc.shape[0] * 2.0 ** -52
        assert f.init_flag == (acc.shape[0] + 1 > 30)
        assert f.scale_gravity == 9.8 and np.array_equal(E.unpack(r["state"])["g"], -f.mean_acc * 9.8)
        assert f.last_pcl_end_time == t and f.last_imu[0] == imus[0][-1]
    assert [len(s[0]) for s in seen] == [7, 11, 11, 4] and f.init_flag                   # 29 messages make init_num 30 -- not yet; the fourth call flips the flag
    f2 = E.ImuEkfRef(acc_in_g=False)
    f2.process(st, np.eye(15), ONE_POINT, seen[0], 0.0, 0.07)
    assert f2.scale_gravity == 1.0
    f3 = E.ImuEkfRef()
    big = (seen[0][0], seen[0][1], seen[0][2] * 9.8)
    f3.process(st, np.eye(15), ONE_POINT, big, 0.0, 0.07)
    assert f3.scale_gravity == 1.0                                                        # |mean_acc| >= 2: metres per second squared already


def test_edited_lists_tile_time_over_three_scans():
    """The list handed to push_imu starts at the previous scan end and stops at this one: over consecutive scans the dt it forms add up to the scan
    intervals, with a message stream that neither starts nor stops on the scan boundaries (scan 1 takes one message from behind its end: note = -1)."""
    f = E.ImuEkfRef()
    st, _ = E.initialise(f, t_end=100.0, lag=E.LAG)
    state, cov = E.moving_state(st[21:24]), E.moving_cov()
    rng = np.random.default_rng(4)
    stream = 100.0 - E.LAG + 0.0101 * np.arange(1, 40)                                    # one stream, cut where the scans end
    prev_end, taken = 100.0, 0
    for s, end in enumerate((100.1, 100.2, 100.3)):
        upto = int(np.searchsorted(stream, end, side="right")) + (1 if s == 1 else 0)
        stamps = stream[taken:upto]; taken = upto
        K = stamps.shape[0]
        assert (stamps[-1] > end) == (s == 1)
        r = f.process(state, cov, ONE_POINT, (stamps, 0.1 * rng.normal(size=(K, 3)), np.array([0, 0, 1.0]) + 0.01 * rng.normal(size=(K, 3))), prev_end, end)
        ed = r["imus"]
        assert ed[0].shape[0] == K + 1 and ed[0][0] == prev_end and ed[0][-1] == end and np.array_equal(ed[0][1:-1], stamps[:-1])
        assert abs(E.push_imu_dt_sum(ed) - (end - prev_end)) < 1e-12
        assert f.last_imu[0] == stamps[-1] and f.last_pcl_end_time == end                 # the handle keeps the original stamp
        state, cov, prev_end = r["state"], r["cov"], end


def _exact_model_scan(n_times=10, seed=0):
    """A static world point seen at n_times different times under the exact-model motion (synth.make_raw_motion)."""
    from voxel_slam_amd import synth
    f = E.ImuEkfRef(ext=E.ext_default())
    st, _ = E.initialise(f, t_end=100.0, lag=E.LAG)
    truth = E.moving_state(st[21:24])
    imus, end, pose, truth_end = synth.make_raw_motion(truth, f.last_imu, 100.0, K=12, span=0.1, scale_gravity=f.scale_gravity, seed=77 + seed)
    ext = E.ext_default(); L, l = ext[:9].reshape(3, 3).T, ext[9:12]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3); w = truth[9:12] + 10.0 * d / np.linalg.norm(d)                 # 10 m away
    toff = np.sort(rng.uniform(0.004, end - 100.0, n_times)).astype(np.float32)
    xyz = np.array([L.T @ (pose(100.0 + float(t))[0].T @ (w - pose(100.0 + float(t))[1]) - l) for t in toff])
    Re, pe, _ = pose(end)
    return f, truth, imus, end, (xyz.astype(np.float32), toff), L.T @ (Re.T @ (w - pe) - l), truth_end


def test_deskew_brings_a_static_point_to_one_place():
    """Ten sightings of one world point, 10 m away, at ten times of the exact-model motion land on the one end-of-scan point: within 4 float32 ulp of a
    10 m range (the measurement is rounded to float32 once, the result once more, and the propagated pose is exact to f64 rounding)."""
    f, truth, imus, end, scan, want, truth_end = _exact_model_scan()
    r = f.process(truth, E.moving_cov(), scan, imus, 100.0, end)
    assert r["compensated"] == 10
    assert np.abs(r["state"][:15] - truth_end[:15]).max() < 1e-12                          # the filter's model IS the motion
    assert np.abs(r["scan"].astype(np.float64) - want).max() <= 4 * 2.0 ** -20            # ulp of [8, 16) m is 2^-20


def test_quirks_untouched_points_point0_and_strict_comparison():
    cases = E.gpu_cases()
    # points at or before the first head: byte-equal
    f = E.ImuEkfRef(**E.filter_options(cases["n257_K5"]))
    c, _, _, r = E.run_case(f, cases["n257_K5"])
    t0 = f.pose_table()[0, 0]
    keep = c["scan"][1].astype(np.float64) <= t0
    assert keep.sum() == 3 and r["scan"][keep].tobytes() == c["scan"][0][keep].tobytes() and r["compensated"] == 257 - 3
    assert (r["scan"][~keep] != c["scan"][0][~keep]).any(axis=1).all()
    # point 0 later than 3 heads: three applications, each on the float result of the one before
    f = E.ImuEkfRef(**E.filter_options(cases["late_first"]))
    c, _, _, r = E.run_case(f, cases["late_first"])
    tab = f.pose_table()
    assert (tab[:, 0] < float(c["scan"][1][0])).sum() == 3 and r["point0_applications"] == 3
    once = E.ImuEkfRef(**E.filter_options(cases["late_first"]))
    two = (np.concatenate([c["scan"][0][:1], c["scan"][0][:1]]), np.concatenate([c["scan"][1][:1], c["scan"][1][:1]]))    # as point 1 the same point is compensated once
    kw = dict(cases["late_first"])
    st, _ = E.initialise(once, lag=kw["lag"])
    r1 = once.process(E.moving_state(st[21:24]), E.moving_cov(), two, c["imus"], c["beg"], c["end"])
    assert r1["point0_applications"] == 3 and not np.array_equal(r1["scan"][0], r1["scan"][1])
    # toff == t_i exactly: the point belongs to head i - 1
    f = E.ImuEkfRef(**E.filter_options(cases["on_head"]))
    c, state, cov, r = E.run_case(f, cases["on_head"])
    tab = f.pose_table()
    toff = c["scan"][1].astype(np.float64)
    hit = np.nonzero(np.isin(toff, tab[1:, 0]))[0]
    assert hit.size >= 3 and np.array_equal(tab[:, 0], np.arange(5) / 128.0)
    for j in hit:
        i = int(np.nonzero(tab[:, 0] == toff[j])[0][0])
        e = tab[i - 1]
        x = E.unpack(r["state"])
        dt = toff[j] - e[0]
        R_i = e[1:10].reshape(3, 3).T @ exp_rate(e[16:19], dt)
        T = e[10:13] + e[13:16] * dt + 0.5 * e[19:22] * dt * dt - x["p"]
        P = f.L.T @ (x["R"].T @ (R_i @ (f.L @ c["scan"][0][j].astype(np.float64) + f.l) + T) - f.l)
        assert np.array_equal(P.astype(np.float32), r["scan"][j])


# ---- the host build of the product's header against the checker ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "imuekf_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libimuekf_hostcheck.so")
    hdrs = [os.path.join(HERE, "..", "voxel-slam_amd", "csrc", h) for h in ("vxba_imuekf_math.hpp", "vxba_init_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max([os.path.getmtime(src)] + [os.path.getmtime(h) for h in hdrs]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.ekh_process_init.argtypes = [f64p, C.c_int, C.c_int, f64p, f64p, f64p, C.c_double, f64p]
    L.ekh_step_matrices.argtypes = [f64p, f64p, f64p, C.c_double, f64p, f64p, f64p]
    L.ekh_motion_blur.argtypes = [f64p, f64p, C.c_int, f64p, f64p, f64p, C.c_double, C.c_double, f64p, f64p, f64p, C.POINTER(C.c_int), f64p, f64p, C.c_int64, f32p, f32p, f32p]
    return L


class HostFilter:
    """The header's filter behind the checker's interface."""

    def __init__(self, hm, cov_acc, cov_gyr, cov_bias_gyr, cov_bias_acc, ext, acc_in_g=True, point_notime=False):
        self.hm, self.filt = hm, np.zeros(17)
        self.filt[8] = 1.0
        self.noise = np.concatenate([np.full(3, cov_acc), np.full(3, cov_gyr), np.full(3, cov_bias_gyr), np.full(3, cov_bias_acc)]).astype(np.float64)
        self.ext, self.acc_in_g, self.point_notime = np.ascontiguousarray(ext, dtype=np.float64), int(acc_in_g), bool(point_notime)
        self.table = np.zeros((0, 22))

    def process(self, state, cov, scan, imus, beg, end):
        st = np.ascontiguousarray(state, dtype=np.float64).copy()
        stamps, gyr, acc = (np.ascontiguousarray(a, dtype=np.float64) for a in imus)
        K = stamps.shape[0]
        if not self.filt[0]:
            self.hm.ekh_process_init(self.filt, self.acc_in_g, K, stamps, gyr, acc, float(end), st)
            return dict(ready=False, state=st, cov=np.asarray(cov))
        cv = np.ascontiguousarray(np.asarray(cov, dtype=np.float64).T).copy()
        xyz = np.ascontiguousarray(scan[0], dtype=np.float32); toff = np.ascontiguousarray(scan[1], dtype=np.float32)
        table = np.zeros((64, 22)); M = C.c_int(); ed = np.zeros((K + 1, 7)); out = np.zeros_like(xyz)
        rc = self.hm.ekh_motion_blur(self.filt, self.noise, K, stamps, gyr, acc, float(beg), float(end), st, cv, table, C.byref(M), ed, self.ext, xyz.shape[0], xyz, toff, out)
        assert rc == 0
        self.table = table[: M.value].copy()
        return dict(ready=True, state=st, cov=cv.T.copy(), imus=(ed[:, 0].copy(), ed[:, 1:4].copy(), ed[:, 4:7].copy()), scan=xyz if self.point_notime else out, heads=M.value)


@pytest.mark.parametrize("name", sorted(E.gpu_cases()))
def test_header_against_checker_on_every_gpu_case(hm, name):
    """Every input of the GPU tests through the g++ build of the header and through the checker: integers and the edited list equal, state and cov at
    64 K 2^-52 max(1, |x|), de-skewed floats within 1 float32 ulp and at most 0.1 % of the coordinates different at all, untouched points byte-equal --
    the conditions the GPU tests impose, met without a GPU.  Also what each case is there for."""
    kw = E.gpu_cases()[name]
    opt = E.filter_options(kw)
    ref = E.ImuEkfRef(**opt)
    c, state, cov, r = E.run_case(ref, kw)
    host = HostFilter(hm, **opt)
    c2, _, _, h = E.run_case(host, kw)
    K = kw["K"]
    assert r["ready"] and h["ready"] and h["heads"] == r["heads"] == ref.pose_table().shape[0]
    assert np.array_equal(host.filt[:2], [1, 31]) and host.filt[9] == ref.last_pcl_end_time and host.filt[10] == ref.last_imu[0] and host.filt[8] == ref.scale_gravity
    for a, b in zip(h["imus"], r["imus"]):
        assert np.array_equal(a, b)
    assert (np.abs(h["state"] - r["state"]) <= E.tol(K + 1, r["state"])).all() and (np.abs(h["cov"] - r["cov"]) <= E.tol(K + 1, r["cov"])).all()
    assert (np.abs(host.table - ref.pose_table()) <= E.tol(K + 1, ref.pose_table())).all() and np.array_equal(host.table[:, 0], ref.pose_table()[:, 0])
    ulp = E.ulp_diff32(h["scan"], r["scan"])
    print(f"{name}: {int((ulp > 0).sum())} of {ulp.size} coordinates differ, max {int(ulp.max())} ulp")
    assert ulp.max() <= 1 and (ulp > 0).sum() <= 0.001 * ulp.size
    keep = c["scan"][1].astype(np.float64) <= ref.pose_table()[0, 0]
    if kw.get("point_notime"):
        assert r["scan"].tobytes() == c["scan"][0].tobytes() and r["compensated"] == 0
    else:
        assert r["scan"][keep].tobytes() == c["scan"][0][keep].tobytes() == h["scan"][keep].tobytes() and r["compensated"] == int((~keep).sum())
        assert keep.sum() == kw.get("prefix", 0)
    # what the case is for
    if name == "one_head":
        assert r["heads"] == 1 and ref.pose_table()[0, 0] == 0.0
    if name == "late_first":
        assert r["point0_applications"] == 3
    if name == "on_head":
        assert np.isin(c["scan"][1].astype(np.float64), ref.pose_table()[1:, 0]).sum() >= 3
    if kw.get("ties"):
        assert kw["n"] < 8 or (np.diff(c["scan"][1]) == 0).sum() >= 5
    assert ref.scale_gravity == (1.0 if name in ("acc_ms2", "acc_large") else 9.8)
    assert (c["end"] > c["imus"][0][-1]) == kw.get("end_after", True)


def test_filter_and_refusal_inputs_of_the_gpu_tests_are_honest():
    """The filter test's scan takes the fallback where the GPU test says it does, on the checker's own de-skewed cloud; every call the refusal test
    expects to be turned away is turned away by the checker, and leaves it able to process the good call."""
    import copy
    ref = E.ImuEkfRef(**E.filter_options(E.FILTER_CASE))
    _, _, _, r = E.run_case(ref, E.FILTER_CASE)
    for size, min_points, half in E.FILTER_PASSES:
        out, used_half = E.filter_scan(r["scan"], size, min_points)
        assert used_half == half and (out.shape[0] >= min_points or half), (size, min_points, out.shape[0])
    first = E.filter_scan(r["scan"], 3.0, 0)[0].shape[0]
    assert 100 <= first < 500 <= E.filter_scan(r["scan"], 3.0, 500)[0].shape[0]
    ref = E.ImuEkfRef(**E.filter_options(E.REFUSAL_CASE))
    c, _, _, want = E.run_case(ref, E.REFUSAL_CASE)
    nxt = E.make_case(t_end=c["end"], **E.REFUSAL_NEXT)
    calls = E.bad_calls(nxt, c["end"], 0.3 * 0.1 / 5)
    assert len(calls) == 13
    for name, (scan, imus, beg, end) in calls.items():
        f = copy.deepcopy(ref)
        with pytest.raises(E.Refused):
            f.process(want["state"], want["cov"], scan, imus, beg, end)
        assert f.last_pcl_end_time == ref.last_pcl_end_time and f.last_imu[0] == ref.last_imu[0] and f.init_num == ref.init_num, name
    assert ref.process(want["state"], want["cov"], nxt["scan"], nxt["imus"], nxt["beg"], nxt["end"])["ready"]


def test_front_inputs_of_the_gpu_tests_are_honest():
    """make_raw_odometry_step through the checker chain alone (checker -> its own filter -> LioOracle), two consecutive scans as the GPU test runs them:
    the de-skew returns the end-of-scan cloud to within the handed-in pose error's reach, the filter keeps >= 500 points without the fallback, the
    odometry converges and ends nearer the truth than the propagated state, in translation and in rotation."""
    from tests import _oracle as O
    from tests._init_ref import so3_log
    from voxel_slam_amd import synth
    pm = synth.make_plane_map(n_roots=800, extent=6, seed=17)
    ext = E.ext_default()
    ref = E.ImuEkfRef(**E.filter_options(dict()))
    st, _ = E.initialise(ref, t_end=100.0, lag=E.LAG)
    orc = O.LioOracle(pm.voxel_size, pm.max_layer); orc.map_update(*pm.args())
    step = synth.make_raw_odometry_step(pm, ref.last_imu, 100.0, st[21:24], scale_gravity=ref.scale_gravity, n_points=3000, K=20, ext=ext)

    def err(a, b):
        return float(np.linalg.norm(a[9:12] - b[9:12])), float(np.linalg.norm(so3_log(a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T)))
    state, cov = step.state_prev, step.cov
    for k in range(2):
        # from the truth the filter reproduces the motion and the de-skew the end-of-scan cloud: the scan is the inverse of the de-skew
        exact = copy_of(ref).process(step.truth_prev, cov, step.scan, step.imus, step.beg_time, step.end_time)
        assert np.abs(exact["state"][:15] - step.truth_end[:15]).max() < 1e-12
        assert np.abs(exact["scan"].astype(np.float64) - step.scan_end).max() < 8 * 2.0 ** -20          # float32 in, float32 out, ranges below 16 m
        w = ref.process(state, cov, step.scan, step.imus, step.beg_time, step.end_time)
        assert w["heads"] == 20 and w["compensated"] == 3000
        flt, half = E.filter_scan(w["scan"], 0.1)
        assert not half and flt.shape[0] >= 500
        orc.var_init(flt, ext[:9].reshape(3, 3).T, ext[9:12], 0.02, 0.05)
        o = orc.lio_state_estimation(w["state"], w["cov"])
        ep, pp = err(o["state"], step.truth_end), err(w["state"], step.truth_end)
        assert o["ok"] and ep[0] < 0.5 * pp[0] and ep[1] < 0.5 * pp[1], (ep, pp)
        if k == 0:
            step = synth.make_raw_odometry_step(pm, step.last_imu, step.end_time, st[21:24], scale_gravity=ref.scale_gravity, truth_prev=step.truth_end, n_points=3000, K=20,
                                                ext=ext, seed=synth.MASTER_SEED + 977)
            state, cov = step.state_prev, o["cov"]


def copy_of(ref):
    import copy
    return copy.deepcopy(ref)
