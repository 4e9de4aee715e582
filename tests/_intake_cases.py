"""The driver messages tests/test_intake_cpu.py and tests/test_gpu_intake.py share: the smallest shapes that reach every path of vxba_intake_push.

``cases()`` -> name -> dict(lidar_type, layout, data (the point bytes), n, pfn, blind, stamp, expect) with expect one of
  "ok"           a cloud (the fallback included)
  "all_trimmed"  survivors exist but all lie behind 0.11: VXBA_ERR_ARG after the run
  "refused"      upstream dereferences what is not there: VXBA_ERR_ARG, nothing launched
  "unsupported"  the yaw-derived Velodyne branch: VXBA_ERR_UNSUPPORTED
``reference(name)`` is the checker's result, computed once per process and never changed.
"""
import functools

import numpy as np

from tests import _intake_ref as R
from voxel_slam_amd import front, synth

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)      # around one wave, one workgroup, four workgroups; 4099: 17 workgroups, odd

# kind -> (lidar type, layout).  point_step 19 (Livox), 22 with the time at 18, 23 (odd, padded), 48; 31 and 16 on top
KINDS = {
    "livox19": (front.LIVOX, front.layout_livox()),
    "velodyne22": (front.VELODYNE, front.layout_from_fields([("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 12, 7), ("ring", 16, 4), ("time", 18, 7)], 22, front.VELODYNE)),
    "ouster48": (front.OUSTER, front.layout_from_fields([("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("intensity", 16, 7), ("t", 20, 6), ("reflectivity", 24, 4), ("ring", 26, 2),
                                                          ("ambient", 28, 4), ("range", 32, 6)], 48, front.OUSTER)),
    "hesai23": (front.HESAI, front.layout_from_fields([("x", 1, 7), ("y", 5, 7), ("z", 9, 7), ("intensity", 13, 2), ("timestamp", 14, 8), ("ring", 22, 2)], 23, front.HESAI)),
    "robosense31": (front.ROBOSENSE, front.layout_from_fields([("x", 3, 7), ("y", 7, 7), ("z", 11, 7), ("intensity", 15, 7), ("timestamp", 19, 8), ("ring", 27, 4)], 31, front.ROBOSENSE)),
    "tartanair16": (front.TARTANAIR, front.layout_from_fields([("x", 0, 7), ("y", 4, 7), ("z", 8, 7)], 16, front.TARTANAIR)),
}
HEAD = 1.7e9 + 0.123456          # Hesai / Robosense stamps: where the f64 difference, then the float rounding, matter


def _rng(*key):
    return np.random.Generator(np.random.PCG64([20250410, *[int(k) for k in key]]))


def _cloud(n, seed):
    """n points in [-1.5, 1.5]^3 (about one in six inside the unit blind sphere) and times in [0, 0.1], half of them on a 64-step grid: ties."""
    rng = _rng(seed, n)
    xyz = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    t = rng.uniform(0.0, 0.1, size=n)
    grid = rng.random(n) < 0.5
    t[grid] = np.floor(t[grid] * 640.0) / 640.0
    return xyz, t


def _case(kind, xyz, toff, pfn, blind=1.0, expect="ok", raw=None, seed=0):
    """toff: seconds (through synth.raw_times); raw: the time field's values as they are."""
    lidar, lay = KINDS[kind]
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    times = raw if raw is not None else synth.raw_times(toff, lay, HEAD)
    if lidar == front.VELODYNE and raw is None and n and expect == "ok":
        times = times.copy(); times[-1] = np.float32(0.05)               # the branch test reads the last point's time
    return {"lidar_type": lidar, "layout": lay, "data": synth.make_driver_message(xyz, times, lay, seed=777 + seed), "n": n, "pfn": int(pfn), "blind": float(blind),
            "stamp": 100.25, "expect": expect}


def squared_range(p):
    """x*x + y*y + z*z as the handlers form it: in float, left to right."""
    x, y, z = (np.float32(v) for v in p)
    return np.float32(np.float32(np.float32(x * x) + np.float32(y * y)) + np.float32(z * z))


def _blind_triplet():
    """Three points whose squared ranges are s0 - 1 ulp, s0, s0 + 1 ulp: 1.5 squared is 2.25 exactly, and a second coordinate of 0, 2^-11 and about
    2^-10.5 adds 0, 1 and (after the sum's rounding) 2 ulps of 2^-22.  Returns (below, at, above, s0)."""
    below, at, above = (1.5, 0.0, 0.0), (1.5, 2.0 ** -11, 0.0), (1.5, float(np.float32(2.0 ** -10.5)), 0.0)
    s0 = squared_range(at)
    assert squared_range(below) == np.nextafter(s0, np.float32(0)) and squared_range(above) == np.nextafter(s0, np.float32(10))
    return below, at, above, s0


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    # the grid: every size x every filtered layout x point_filter_num 1, 3, 4, n + 1
    for kind, (lidar, lay) in KINDS.items():
        for n in SIZES:
            xyz, t = _cloud(n, len(kind))
            if lidar == front.TARTANAIR:
                out[f"grid-{kind}-n{n}"] = _case(kind, xyz, t, 1)
                continue
            for pfn in (1, 3, 4, n + 1):
                expect = "refused" if n == 0 and lidar in (front.HESAI, front.ROBOSENSE) else "ok"
                out[f"grid-{kind}-n{n}-f{pfn}"] = _case(kind, xyz, t, pfn, expect=expect, seed=pfn)
    # squared range exactly blind, and its two float neighbours, on every axis; blind is s0 as a double
    below, at, above, s0 = _blind_triplet()
    pts = []
    for x, y, z in (below, at, above):
        pts += [(x, y, z), (y, x, z), (z, -y, -x)]
    filler, tf = _cloud(70, 5)
    xyz = np.concatenate([np.array(pts, dtype=np.float32), filler * np.float32(2.0)])
    t = np.concatenate([np.linspace(0.02, 0.03, 9), tf])
    for kind in ("livox19", "velodyne22", "hesai23"):
        out[f"blind-edge-{kind}"] = _case(kind, xyz, t, 1, blind=float(s0))
    # every point blind: the fallback
    xyz, t = _cloud(300, 6)
    for kind in ("livox19", "velodyne22", "ouster48", "robosense31"):
        out[f"all-blind-{kind}"] = _case(kind, xyz, t, 1, blind=1e9)
    out["all-blind-inf-livox19"] = _case("livox19", xyz, t, 3, blind=float("inf"))
    out["all-decimated-blind-hesai23"] = _case("hesai23", np.concatenate([np.zeros((1, 3), np.float32), xyz]), np.concatenate([[0.0], t]), 400)
    # times of 0.11 exactly (the float lies below the double 0.11: kept) and the floats on either side
    e = np.float32(0.11)
    edge = np.array([np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(1)), np.nextafter(np.nextafter(e, np.float32(1)), np.float32(1))], dtype=np.float32)
    xyz, t = _cloud(200, 7)
    traw = t.astype(np.float32); traw[10:14] = edge; traw[100:104] = edge[::-1]; traw[-1] = np.float32(0.05)
    out["trim-edge-velodyne22"] = _case("velodyne22", xyz, None, 1, raw=traw)
    nraw = np.rint(t * 1e9).astype(np.uint32); nraw[10:16] = [109999984, 109999992, 110000000, 110000008, 110000016, 110000024]
    out["trim-edge-livox19"] = _case("livox19", xyz, None, 1, raw=nraw)
    out["trim-edge-ouster48"] = _case("ouster48", xyz, None, 3, raw=nraw)
    draw = HEAD + t; draw[0] = HEAD; draw[10:16] = HEAD + np.array([0.1099999, 0.10999999, 0.11, 0.11000001, 0.1100001, 0.12])
    out["trim-edge-hesai23"] = _case("hesai23", xyz, None, 1, raw=draw)
    # every survivor behind 0.11
    out["all-trimmed-velodyne22"] = _case("velodyne22", xyz, None, 1, raw=np.concatenate([np.full(199, 0.115, np.float32), [np.float32(0.1150001)]]), expect="all_trimmed")
    out["all-trimmed-livox19"] = _case("livox19", xyz, None, 4, raw=np.full(200, 200000000, np.uint32), expect="all_trimmed")
    # runs of 16 and 128 equal times, an already sorted message and a reversed one
    xyz, t = _cloud(600, 8)
    tt = t.copy(); tt[40:56] = 0.031; tt[200:328] = 0.0625; tt[400:416] = 0.031
    for kind in ("livox19", "velodyne22", "ouster48", "hesai23", "robosense31"):
        out[f"ties-{kind}"] = _case(kind, xyz, tt, 1)
        out[f"ties-f3-{kind}"] = _case(kind, xyz, tt, 3)
        out[f"sorted-{kind}"] = _case(kind, xyz, np.sort(t), 1)
        out[f"reversed-{kind}"] = _case(kind, xyz, np.sort(t)[::-1], 1)
    out["all-equal-times-livox19"] = _case("livox19", xyz, np.full(600, 0.05), 1)
    # coordinates and times that are not finite; -0.0 times
    xyz, t = _cloud(300, 9)
    bad = xyz.copy()
    bad[5, 0] = np.nan; bad[6, 1] = np.nan; bad[7, 2] = np.nan; bad[8] = np.nan; bad[20, 0] = np.inf; bad[21, 1] = -np.inf; bad[22] = (np.inf, -np.inf, 2.0)
    for kind in ("livox19", "velodyne22", "hesai23", "tartanair16"):
        out[f"nonfinite-xyz-{kind}"] = _case(kind, bad, t, 1)
    traw = t.astype(np.float32)
    traw[3] = np.nan; traw[4] = np.inf; traw[5] = -np.inf; traw[30:34] = np.float32(-0.0); traw[34:38] = np.float32(0.0); traw[38:40] = np.float32(-0.0); traw[-1] = np.float32(0.05)
    out["nonfinite-and-negzero-times-velodyne22"] = _case("velodyne22", xyz, None, 1, raw=traw)
    draw = HEAD + t; draw[3] = np.nan; draw[4] = np.inf; draw[5] = -np.inf; draw[6] = 1e300
    out["nonfinite-times-hesai23"] = _case("hesai23", xyz, None, 1, raw=draw)
    out["nonfinite-times-robosense31"] = _case("robosense31", xyz, None, 3, raw=draw)
    one = np.array([[2.0, 0.0, 0.0]], dtype=np.float32)
    out["only-nan-time-velodyne22"] = _case("velodyne22", np.concatenate([one, one]), None, 1, raw=np.array([np.nan, 0.05], np.float32))
    # u32 times where the conversion to float rounds: above 2^24 inside the scan, and near 2^32 (behind the trim: the record's counts)
    nraw = np.rint(t * 1e9).astype(np.uint32)
    nraw[:12] = [16777215, 16777216, 16777217, 16777219, 33554431, 33554433, 33554435, 99999999, 100000001, 100000003, 100000005, 67108865]
    nraw[12:18] = [4294967295, 4294967167, 4294967168, 4294967169, 4294967040, 2147483777]
    out["u32-rounding-livox19"] = _case("livox19", xyz, None, 1, raw=nraw)
    out["u32-rounding-ouster48"] = _case("ouster48", xyz, None, 1, raw=nraw)
    # Hesai / Robosense: stamps around 1.7e9 s (the grid) and points before time_head: negative times
    draw = HEAD + t; draw[0] = HEAD + 0.04
    out["before-head-hesai23"] = _case("hesai23", xyz, None, 1, raw=draw)
    out["before-head-robosense31"] = _case("robosense31", xyz, None, 4, raw=draw)
    # the Velodyne branch without a usable time field
    for name, last in (("late", 0.2), ("early", 0.005), ("at-001", 0.01), ("zero", 0.0), ("nan", np.nan)):
        traw = t.astype(np.float32); traw[-1] = np.float32(last)
        out[f"unsupported-{name}-velodyne22"] = _case("velodyne22", xyz, None, 1, raw=traw, expect="unsupported")
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The checker on a case: dict(xyz, toff, record, beg_time, time_head); for the cases that end in an error, dict(error, record or None)."""
    c = cases()[name]
    try:
        return R.process(c["data"], c["layout"], c["lidar_type"], c["pfn"], c["blind"], c["stamp"])
    except R.AllTrimmed as e:
        return {"error": "all_trimmed", "record": e.record}
    except R.Refused:
        return {"error": "refused", "record": None}
    except R.Unsupported:
        return {"error": "unsupported", "record": None}


def time_head(name):
    """What front.ScanIntake reads from point 0 of a Hesai / Robosense message; 0 otherwise."""
    c = cases()[name]
    if c["lidar_type"] in (front.HESAI, front.ROBOSENSE) and c["n"]:
        return float(np.frombuffer(c["data"], dtype="<f8", count=1, offset=int(c["layout"].off_time))[0])
    return 0.0
