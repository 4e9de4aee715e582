"""The Velodyne messages without usable point times that tests/test_intake_yaw_cpu.py and tests/test_gpu_intake_yaw.py share: the smallest shapes that
reach every cell of the state table of include/vxba.h (YAW TIMES) and every seam of vxba_intake_push_yaw -- the wave (64), the workgroup (256), `cool`
(1000), the 64-special chunk of the resolver, and the second pass of the scans.

``cases()`` -> name -> dict(layout, data (the point bytes), n, pfn, blind, omega_l, x, y, z).  ``reference(name)`` is tests/_intake_yaw_ref.replay on it,
computed once per process and never changed.
"""
import functools

import numpy as np

from tests import _intake_yaw_ref as YR
from voxel_slam_amd import front, synth, vxba

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001, 1023, 1024, 1025, 2049, 4097)
FILTERS = (1, 3, 4)
OMEGAS = (3610.0, 1800.0)          # upstream's default (0.1 s = 361 degrees) and half of it (a half turn survives)
STARTS = (30.0, -179.9, 180.0, 90.0, -60.0)     # -179.9: just past the cut, the wrap comes at once; 180: on the cut, and a full turn ends on it
S = vxba.ScanLayout
LAYOUTS = {
    "velodyne22": S(22, 0, 4, 8, 18, S.TIME_F32, S.RULE_YAW, 1),        # the common Velodyne layout, its time field present, zero and ignored
    "plain16": front.layout_velodyne_yaw([("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 12, 7)], 16),
    "odd19": front.layout_velodyne_yaw([("intensity", 0, 2), ("x", 1, 7), ("ring", 5, 4), ("y", 7, 7), ("z", 13, 7)], 19),
}


def _rng(*key):
    return np.random.Generator(np.random.PCG64([20251021, *[int(k) for k in key]]))


def from_angles(deg, radius=8.0, z=0.5):
    """Points at the azimuths ``deg`` (degrees): float32 x, y, z."""
    a = np.deg2rad(np.asarray(deg, dtype=np.float64))
    r = np.broadcast_to(np.asarray(radius, dtype=np.float64), a.shape)
    return (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32), np.broadcast_to(np.asarray(z, dtype=np.float64), a.shape).astype(np.float32)


def ring_scan(n, start, jitter, seed, clockwise=True):
    """n points of a 16-ring sensor in firing order: one azimuth per column of 16, turning clockwise (the azimuth falls) from ``start`` by at most 6
    degrees a column and one turn in all, every point's azimuth off by a Gaussian ``jitter`` (degrees)."""
    rng = _rng(seed, n)
    cols = (n + 15) // 16
    step = min(360.0 / max(cols - 1, 1), 6.0)
    col = np.arange(n) // 16
    az = start + (-1.0 if clockwise else 1.0) * step * col
    if jitter == 0.0 and cols > 1 and step < 6.0:
        az[col == cols - 1] = start - 360.0                                # the last column exactly one turn on
    az = az + rng.normal(0.0, jitter, size=n) if jitter else az
    rad = rng.uniform(3.0, 30.0, size=n)
    elev = np.deg2rad(-15.0 + 2.0 * (np.arange(n) % 16))
    x, y, _ = from_angles(az, rad)
    if jitter == 0.0:                                                      # on the axes exactly, so that a start on the cut is atan2(0, -r)
        q = np.round(az / 90.0)
        on = np.abs(az - 90.0 * q) < 1e-9
        y[on & (q % 2 == 0)] = 0.0
        x[on & (q % 2 == 1)] = 0.0
    return x, y, (rad * np.tan(elev)).astype(np.float32)


def stepped(n, marks, base=-160.0, top=170.0):
    """Azimuths that rest at ``base`` (drifting down a little) and at every index of ``marks`` jump to ``top`` -- a step above 180 -- and come back in
    three steps below 180: top, top - 110, top - 220, base.  So every mark is a wrap candidate and nothing else is special."""
    az = base - 1e-3 * np.arange(n)
    for m in marks:
        for k, a in enumerate((top + 1e-3 * m, top - 110.0, top - 220.0)):
            if m + k < n:
                az[m + k] = a
    return az


def _make(layout, x, y, z, pfn, blind, omega_l, seed=0):
    lay = LAYOUTS[layout]
    xyz = np.stack([x, y, z], axis=1).astype(np.float32) if len(x) else np.zeros((0, 3), dtype=np.float32)
    times = np.zeros(len(x), dtype=np.float32) if int(lay.time_type) == S.TIME_F32 else None
    return {"layout": lay, "layout_name": layout, "data": synth.make_driver_message(xyz, times, lay, seed=4242 + seed), "n": len(x), "pfn": int(pfn), "blind": float(blind),
            "omega_l": float(omega_l), "x": xyz[:, 0].copy(), "y": xyz[:, 1].copy(), "z": xyz[:, 2].copy()}


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    names = list(LAYOUTS)

    def add(name, x, y, z, k, blind=1.0):
        """k cycles the layout, the filter and omega_l, each with its own period"""
        out[name] = _make(names[k % 3], x, y, z, FILTERS[(k // 3 + k) % 3], blind, OMEGAS[(k // 2) % 2], seed=k)

    # every size, clockwise with 0.3 degrees of jitter, the starts in turn
    for k, n in enumerate(SIZES):
        add(f"cw_n{n}", *ring_scan(n, STARTS[k % len(STARTS)], 0.3, k), k)
    # every start without jitter (180: starts on the cut and ends on it), with 0.3 and with 3 degrees, over one workgroup and a bit, and over a full turn
    for k, start in enumerate(STARTS):
        for jitter in (0.0, 0.3, 3.0):
            add(f"cw_start{start:g}_jitter{jitter:g}_n257", *ring_scan(257, start, jitter, 100 + k), k + 1)
            add(f"cw_start{start:g}_jitter{jitter:g}_n2049", *ring_scan(2049, start, jitter, 200 + k), k + 2)
    # counter-clockwise: the times are negative.  With jitter a few points of the first column survive; with a steadily rising azimuth behind a blind
    # first point nothing does, and the fallback cloud is used
    add("ccw_jitter_n257", *ring_scan(257, 30.0, 0.3, 300, clockwise=False), 0)
    for k, (n, start) in enumerate(((257, 30.0), (1025, -100.0))):
        x, y, z = from_angles(start + 0.3 * np.arange(n), np.where(np.arange(n) == 0, 0.4, 8.0))
        add(f"ccw_n{n}", x, y, z, k)
    # the first non-skipped point is blind and looks elsewhere: yaw_first is its angle all the same
    x, y, z = ring_scan(257, 30.0, 0.3, 310)
    x[0], y[0], z[0] = 0.05, 3.0, 0.0                                     # skipped
    x[1], y[1], z[1] = -0.3, 0.2, 0.0                                     # not skipped, blind, at 146 degrees
    add("first_point_blind", x, y, z, 3)
    # nothing but skipped points; nothing but blind ones
    x, y, z = ring_scan(65, 30.0, 0.3, 320)
    add("all_skipped", np.full(65, 0.05, dtype=np.float32) * np.where(np.arange(65) % 2, 1, -1).astype(np.float32), y, z, 4)
    x, y, z = from_angles(np.linspace(30.0, -200.0, 65), 0.5, 0.1)
    add("all_blind", x, y, z, 5)
    # two candidates 999, 1000 and 1001 indices apart (and a third one well behind), plain and with skipped points in between: cool counts indices
    for gap in (999, 1000, 1001):
        x, y, z = from_angles(stepped(2049, (20, 20 + gap, 1025 + gap)))
        add(f"candidates_{gap}_apart", x, y, z, gap, blind=0.5)
        keep = np.concatenate([m + np.arange(3) for m in (20, 20 + gap, 1025 + gap)])      # the candidates and their way back stay
        x2 = x.copy()
        x2[np.arange(2049) % 3 == 1] = 0.05
        x2[keep] = x[keep]
        x = x2
        add(f"candidates_{gap}_apart_skips_between", x, y, z, gap + 1, blind=0.5)
    # events at small angles, where (r - 360 (k - 1)) - 360 and r - 360 k round differently: five of them, a turn and a bit apart in indices
    x, y, z = from_angles(stepped(4097, tuple(20 + 1003 * np.arange(5)), base=-170.0, top=43.0))
    add("events_at_small_angles", x, y, z, 1)
    # q = 1 held across a workgroup boundary: a step below -180 at 250 (q = 1), quiet until a step above 180 at 262 takes it back
    az = 170.0 - 1e-3 * np.arange(513)
    az[250:262] = -170.0 - 1e-3 * np.arange(12)
    x, y, z = from_angles(az)
    add("q1_across_workgroups", x, y, z, 0, blind=4.0)
    # exactly 64 and exactly 65 specials: the azimuth flips between -160 and +170 that often, then rests
    for count in (64, 65):
        az = np.full(257, -160.0) - 1e-3 * np.arange(257)
        flips = 40 + 2 * np.arange(count)
        for t, m in enumerate(flips):
            az[m:] = (170.0 if t % 2 == 0 else -160.0) - 1e-3 * np.arange(m, 257)
        x, y, z = from_angles(az)
        add(f"specials_{count}", x, y, z, count)
    # every point a special: the azimuth flips at every index, 32 chunks of the resolver and a bit
    x, y, z = from_angles(np.where(np.arange(2049) % 2, 170.0, -160.0) - 1e-3 * np.arange(2049))
    add("all_specials_n2049", x, y, z, 2)
    # Gaussian clouds: about a quarter of the points are specials, several events, points inside the blind sphere and inside |x| < 0.1
    for k, n in enumerate((2049, 4097)):
        g = _rng(400, n).normal(0.0, 2.0, size=(n, 3)).astype(np.float32)
        add(f"gaussian_n{n}", g[:, 0], g[:, 1], g[:, 2], k)
        add(f"gaussian_n{n}_filter4", g[:, 0], g[:, 1], g[:, 2], 8 + k)
    # a squared range exactly equal to blind stays (the other handlers would drop it): blind is the 40th point's own squared range
    x, y, z = ring_scan(257, 30.0, 0.3, 330)
    z[40] = 0.0; x[40], y[40] = 2.0, 0.5                                 # 4 + 0.25 = 4.25 exactly, at 14 degrees, where column 2 of the scan looks
    out["range_equals_blind"] = _make("odd19", x, y, z, 4, 4.25, 3610.0, seed=9)
    # NaN and infinite coordinates, the very first point among them
    x, y, z = ring_scan(257, 30.0, 0.3, 340)
    x[0] = np.nan; y[5] = np.inf; z[64] = -np.inf; x[128] = np.inf; y[255] = np.nan; z[256] = np.nan
    add("non_finite", x, y, z, 6)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    c = cases()[name]
    return YR.replay(c["x"], c["y"], c["z"], c["pfn"], c["blind"], c["omega_l"])
