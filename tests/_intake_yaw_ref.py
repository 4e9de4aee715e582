"""The yaw-derived point times of the Velodyne handler (VoxelSLAM/src/feature_point.hpp:200-252) twice over, for vxba_intake_push_yaw:

``replay``    the loop as upstream wrote it -- cool, yaw_first, yaw_last, yaw_bias carried from point to point -- followed by ``pcl_handler``
              (tests/_intake_ref.py).  float32 scalars in the order of the C++ expressions, doubles where upstream has doubles.  It also records the
              margin of every decision on 180 and what vxba_intake_yaw_info counts.
``parallel``  the restated form of include/vxba.h (YAW TIMES): per point the angle and the step d from the previous active point, the class of d, and a
              walk over the specials only.  ``variant`` names one deliberate defect (DEGRADED), for tests that show the cases can tell.

The fixed choices of include/vxba.h are applied in both: the float atan2 is the correctly rounded one (float64 arctan2 rounded to float32; the CPU
suite proves with mpmath that no test point lies near enough to a rounding tie for the two to differ), and a point with a non-finite coordinate is
skipped like |x| < 0.1.  Upstream decides on ``yaw_angle - yaw_last``; the restated form decides on d = r_j - r_p.  ``replay`` is upstream's and
records how far each of its differences lies from the threshold.
"""
import numpy as np

from tests import _intake_ref as KR

F = np.float32
D = np.float64
DEG = D(57.2957)
COUNTS = ("skipped", "active", "candidates", "events")
DEGRADED = ("ge_180", "cool_in_active_points", "event_one_subtraction", "blocked_without_360", "first_from_active", "le_blind")


def atan2f(y, x):
    """The correctly rounded float atan2 (see the module text)."""
    return F(np.arctan2(D(y), D(x)))


def _range2(x, y, z):
    with np.errstate(over="ignore", invalid="ignore"):
        return F(F(F(x * x) + F(y * y)) + F(z * z))


def replay(x, y, z, point_filter_num, blind, omega_l):
    """:200-252, then pcl_handler.  dict(xyz, toff, record, kept (original indices in push order), times (their float32 times), yaw (the double
    yaw_angle of every active point, by original index; NaN elsewhere), counts (COUNTS), margins (|difference - threshold| of every decision, degrees),
    cells (the set of (class, q before, cool allows) the walk met))."""
    n = len(x)
    pl, kept, margins, cells = [], [], [], set()
    yaw_of = np.full(n, np.nan)
    skipped = active = candidates = events = 0
    first_point = True
    yaw_first = yaw_last = yaw_bias = D(0)
    r_last = D(0)           # bookkeeping for the counts only: the un-biased angle behind yaw_last, so that a candidate is d > 180 as the header counts it
    plus_last = False       # bookkeeping: yaw_last carries the += 360 of :237
    cool = 0
    omega_l = D(omega_l)
    for i in range(n):
        cool -= 1
        ax, ay, az = F(x[i]), F(y[i]), F(z[i])
        if not (np.isfinite(ax) and np.isfinite(ay) and np.isfinite(az)):       # fixed choice
            skipped += 1
            continue
        if float(np.abs(ax)) < 0.1:
            skipped += 1
            continue
        r = D(atan2f(ay, ax)) * DEG
        yaw_angle = r - yaw_bias
        if first_point:
            yaw_first = yaw_angle
            yaw_last = yaw_angle
            r_last = r
            first_point = False
        if float(_range2(ax, ay, az)) < blind:
            continue
        active += 1
        d = r - r_last
        cls = "cand" if d > 180 else ("reset" if d == 180 else ("set" if d < -180 else "ident"))
        candidates += cls == "cand"
        cells.add((cls, int(plus_last), bool(cool <= 0) if cls == "cand" and not plus_last else None))
        margins.append(abs(float((yaw_angle - yaw_last) - 180)))
        if yaw_angle - yaw_last > 180 and cool <= 0:
            yaw_bias += 360; yaw_angle -= 360; cool = 1000
            events += 1
        margins.append(abs(float(np.abs(yaw_angle - yaw_last) - 180)))
        plus_last = False
        if np.abs(yaw_angle - yaw_last) > 180:
            yaw_angle += 360
            plus_last = True
        curvature = F((yaw_first - yaw_angle) / omega_l)
        yaw_last = yaw_angle
        r_last = r
        yaw_of[i] = yaw_angle
        if curvature >= 0 and float(curvature) < 0.1:
            if i % point_filter_num == 0:
                before = len(pl)
                KR._push(pl, ax, ay, az, curvature)
                if len(pl) > before:
                    kept.append(i)
    times = np.array([p[3] for p in pl], dtype=np.float32)
    xyz, toff, rec = KR.pcl_handler(pl, n)
    return {"xyz": xyz, "toff": toff, "record": rec, "kept": np.array(kept, dtype=np.int64), "times": times, "yaw": yaw_of,
            "counts": np.array([skipped, active, candidates, events], dtype=np.int64), "margins": np.array(margins), "cells": cells}


IDENT, SET, RESET, CAND = range(4)


def classify(d, variant=None):
    """The class of d = r_j - r_p (include/vxba.h, YAW TIMES)."""
    if (d >= 180) if variant == "ge_180" else (d > 180):
        return CAND
    if d == 180:
        return RESET
    if d < -180:
        return SET
    return IDENT


def parallel(x, y, z, point_filter_num, blind, omega_l, variant=None):
    """The restated form; the same dict as :func:`replay` without margins and cells, and ``specials`` (their original indices)."""
    assert variant is None or variant in DEGRADED
    x, y, z = (np.asarray(v, dtype=np.float32) for v in (x, y, z))
    n = len(x)
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        skip = ~finite | (np.abs(x).astype(np.float64) < 0.1)
        s = ((x * x + y * y) + z * z).astype(np.float64)
        r = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32).astype(np.float64) * DEG
    blind_hit = (s <= blind) if variant == "le_blind" else (s < blind)
    act = ~skip & ~blind_hit
    idx = np.arange(n)
    yaw_of = np.full(n, np.nan)
    counts = np.array([int(skip.sum()), int(act.sum()), 0, 0], dtype=np.int64)
    pl, kept, specials = [], [], []
    if act.any():
        f = int(np.flatnonzero(act)[0]) if variant == "first_from_active" else int(np.flatnonzero(~skip)[0])
        last = np.maximum.accumulate(np.where(act, idx, -1))               # the last active point at or before i
        pred = np.concatenate([[-1], last[:-1]])
        rp = np.where(pred >= 0, r[np.maximum(pred, 0)], r[f])
        d = r - rp
        cls = np.array([classify(d[i], variant) if act[i] else IDENT for i in range(n)])
        counts[2] = int((cls == CAND).sum())
        specials = np.flatnonzero(cls != IDENT)
        # the walk over the specials: (k, event here, q) behind each
        q, k, e = 0, 0, None
        nth_active = np.cumsum(act)                                        # for the variant that counts cool in active points
        state = {}
        for j in specials:
            event = False
            if cls[j] == SET:
                q = 1
            elif cls[j] == RESET:
                q = 0
            elif q == 1:
                q = 0
            else:
                gap = None if e is None else (nth_active[j] - nth_active[e] if variant == "cool_in_active_points" else j - e)
                if gap is None or gap >= 1000:
                    k, e, event = k + 1, j, True
                else:
                    q = 0 if variant == "blocked_without_360" else 1
            state[j] = (k, event, q)
        counts[3] = k
        pos = np.cumsum(cls != IDENT)                                      # the governing special of i is number pos[i] - 1
        yaw_first = r[f]
        for i in np.flatnonzero(act):
            kk, event, qq = state[specials[pos[i] - 1]] if pos[i] else (0, False, 0)
            event = event and cls[i] != IDENT
            if event and variant != "event_one_subtraction":
                yaw = (r[i] - D(360) * D(kk - 1)) - D(360)
            else:
                yaw = r[i] - D(360) * D(kk)
            if qq:
                yaw = yaw + D(360)
            yaw_of[i] = yaw
            curvature = F((yaw_first - yaw) / D(omega_l))
            if curvature >= 0 and float(curvature) < 0.1 and i % point_filter_num == 0:
                before = len(pl)
                KR._push(pl, x[i], y[i], z[i], curvature)
                if len(pl) > before:
                    kept.append(int(i))
    times = np.array([p[3] for p in pl], dtype=np.float32)
    xyz, toff, rec = KR.pcl_handler(pl, n)
    return {"xyz": xyz, "toff": toff, "record": rec, "kept": np.array(kept, dtype=np.int64), "times": times, "yaw": yaw_of, "counts": counts,
            "specials": np.asarray(specials, dtype=np.int64)}


def same(a, b):
    """Kept indices, time bits, the double yaw of every active point, counts and the cloud: equal?"""
    return (np.array_equal(a["kept"], b["kept"]) and a["times"].tobytes() == b["times"].tobytes() and a["yaw"].tobytes() == b["yaw"].tobytes()
            and np.array_equal(a["counts"], b["counts"]) and a["xyz"].tobytes() == b["xyz"].tobytes() and a["toff"].tobytes() == b["toff"].tobytes()
            and a["record"].tobytes() == b["record"].tobytes())
