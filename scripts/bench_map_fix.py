"""Times the fixed-point entry points of the device-resident local map (vxba_map_cut_voxel_fix / vxba_map_loop_update) on the
scan-cycle workload of bench.py (`scan_cycle`: 100k-point scans, window 10), each against code the library already had, in the SAME process:

  --what fix    one keyframe-sized cloud (every fifth point of the next scan, ~20k points) into the running map: cut_voxel_fix, host and device form.
                Yardstick: vxba_map_cut_voxel (host / device form) of the same cloud into an equal map.
  --what loop   loop_update of 5 keyframe clouds + a 10-scan window, resident-scan mode and host-array mode, and its parts called one by one
                (clear / fix inserts / window re-cut / recut).  Yardstick: ten vxba_map_cut_voxel + one vxba_map_recut of the same window on an empty map.

Every repeat starts from the same map: the handles are cleared (they keep their allocations) and driven through the same scans again -- the poses are the
true ones and no BA runs, so what enters the map is the same every time.  Host clock around calls that end in a stream wait; medians and min-max of
--repeats repeats after --warmup.  One JSON line per run; nothing here asserts.

    python scripts/bench_map_fix.py --what fix --repeats 25 --out bench_out/map_fix_fix.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library is loaded, as in the other scripts: one HIP runtime in the process)

PRM = dict(voxel_size=1.0, max_layer=2, min_point=(20, 20, 15, 10), min_eigen_value=0.02, plane_eigen_value_thre=(0.25, 0.25, 0.25, 0.25))     # bench.py LOCAL_MAP_PRM
WIN, PTS = 10, 100_000


def to_world(pose, pnt):
    R = pose[:9].reshape(3, 3).T
    x, y, z = pnt[:, 0], pnt[:, 1], pnt[:, 2]
    return np.stack([(R[r, 0] * x + R[r, 1] * y + R[r, 2] * z) + pose[9 + r] for r in range(3)], axis=1)


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "n": int(a.size)}


class Workload:
    def __init__(self, S):
        from voxel_slam_amd import synth
        self.S = S
        self.xyz, self.fp, self.poses, _ = synth.make_scans(win_size=S + 1, pts_per_scan=PTS, extent=60.0, seed=synth.MASTER_SEED + 950)
        rng = np.random.default_rng(1)
        d = np.abs(rng.normal(0, 1e-3, (self.xyz.shape[0], 3))) + 1e-5
        self.var = np.zeros((self.xyz.shape[0], 3, 3)); self.var[:, 0, 0] = d[:, 0]; self.var[:, 1, 1] = d[:, 1]; self.var[:, 2, 2] = d[:, 2]
        self.world = [to_world(self.poses[k], self.scan(k)[0]) for k in range(S + 1)]

    def scan(self, k):
        s = slice(self.fp[k], self.fp[k + 1])
        return self.xyz[s], self.var[s]

    def drive(self, m, f, upto, margi_last=True):
        """clear + scans 0 .. upto - 1 through cut_voxel -> recut -> margi -> slide at the true poses; returns the scans left in the window."""
        m.clear()
        win = []
        for k in range(upto):
            win.append(k)
            xs = self.poses[win]
            f.clear()
            m.cut_voxel(len(win) - 1, *self.scan(k), self.world[k])
            m.recut(len(win), xs, f)
            if len(win) == WIN and (margi_last or k < upto - 1):
                f.evaluate_only_residual(xs)
                m.margi(len(win), xs, f)
                m.slide(1)
                win = win[1:]
        return win


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def bench_fix(vx, w, repeats, warmup):
    k = w.S                                    # the scan after the ones in the map
    pnt, var = w.scan(k)
    pnt, var, wld = np.ascontiguousarray(pnt[::5]), np.ascontiguousarray(var[::5]), np.ascontiguousarray(w.world[k][::5])
    var9 = np.ascontiguousarray(np.transpose(var, (0, 2, 1))).reshape(-1, 9)
    names = ("cut_voxel_fix", "cut_voxel_fix_device", "cut_voxel", "cut_voxel_device")
    maps = {n: vx.LocalMap(win_size=WIN, **PRM) for n in names}
    f = vx.LidarFactor(WIN)
    t_pnt, t_var, t_wld = (torch.tensor(a, device="cuda") for a in (pnt, var9, wld))
    torch.cuda.synchronize()
    n = pnt.shape[0]
    calls = {
        "cut_voxel_fix": lambda m, o: m.cut_voxel_fix(wld, var, 0.0),
        "cut_voxel_fix_device": lambda m, o: m.cut_voxel_fix_device(n, t_wld.data_ptr(), t_var.data_ptr(), 0.0),
        "cut_voxel": lambda m, o: m.cut_voxel(o, pnt, var, wld),
        "cut_voxel_device": lambda m, o: m._chk(m._L.vxba_map_cut_voxel_device(m._h, o, n, t_pnt.data_ptr(), t_var.data_ptr(), t_wld.data_ptr())),
    }
    ms = {n_: [] for n_ in names}
    order = list(names)
    counts = None
    for r in range(warmup + repeats):
        order = order[1:] + order[:1]          # alternate who goes first
        for name in order:
            win = w.drive(maps[name], f, w.S)
            counts = maps[name].counts()
            t = timed(lambda: calls[name](maps[name], len(win)))
            if r >= warmup:
                ms[name].append(t)
    out = {"what": "fix", "cloud_points": int(n), "scans_in_map": w.S, "map": counts, "fix_pool": maps["cut_voxel_fix"].fix_pool()}
    out.update({name: stats(v) for name, v in ms.items()})
    return out


def bench_loop(vx, w, repeats, warmup):
    clouds = [np.ascontiguousarray(w.world[k][::5]) for k in range(5)]
    cvars = [np.ascontiguousarray(w.scan(k)[1][::5]) for k in range(5)]
    a, b, c, d = (vx.LocalMap(win_size=WIN, **PRM) for _ in range(4))       # resident mode | host mode | the parts one by one | the yardstick
    f = vx.LidarFactor(WIN)
    ms = {k: [] for k in ("loop_update_resident", "loop_update_host", "parts_clear", "parts_fix_inserts", "parts_window_recut_host", "parts_recut", "yardstick_10_cut_voxel", "yardstick_recut")}
    counts = None
    for r in range(warmup + repeats):
        for m in (a, b, c):
            win = w.drive(m, f, w.S, margi_last=False)      # a full window of WIN scans
        assert len(win) == WIN
        poses = w.poses[win]
        scans = [w.scan(k) for k in win]
        t = {}
        t["loop_update_resident"] = timed(lambda: a.loop_update(clouds, cvars, poses, None))
        t["loop_update_host"] = timed(lambda: b.loop_update(clouds, cvars, poses, scans))
        t["parts_clear"] = timed(c.clear)
        t["parts_fix_inserts"] = timed(lambda: [c.cut_voxel_fix(p, v, 0.0) for p, v in zip(clouds, cvars)])
        t["parts_window_recut_host"] = timed(lambda: [c.cut_voxel(i, *scans[i], w.world[k]) for i, k in enumerate(win)])
        f.clear()
        t["parts_recut"] = timed(lambda: c.recut(WIN, poses, f))
        d.clear()
        t["yardstick_10_cut_voxel"] = timed(lambda: [d.cut_voxel(i, *scans[i], w.world[k]) for i, k in enumerate(win)])
        f.clear()
        t["yardstick_recut"] = timed(lambda: d.recut(WIN, poses, f))
        counts = a.counts()
        if r >= warmup:
            for k_, v in t.items():
                ms[k_].append(v)
    out = {"what": "loop", "keyframe_clouds": 5, "cloud_points": int(clouds[0].shape[0]), "window_scans": WIN, "points_per_scan": PTS, "map_after": counts}
    out.update({k_: stats(v) for k_, v in ms.items()})
    out["yardstick_total_median_ms"] = out["yardstick_10_cut_voxel"]["median_ms"] + out["yardstick_recut"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=("fix", "loop"), required=True)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scans", type=int, default=12, help="scans driven through the map before the timed call (loop: at least the window)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from voxel_slam_amd import vxba as vx
    vx.load_library()
    w = Workload(max(args.scans, WIN))
    res = (bench_fix if args.what == "fix" else bench_loop)(vx, w, args.repeats, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
