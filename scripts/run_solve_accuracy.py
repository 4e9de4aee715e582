#!/usr/bin/env python3
"""Backward error of every damped solver on the systems of tests/_solve_cases.py: the device's four-wave LDL^T (LiDAR-only and
LiDAR-inertial form), the numpy model of the same elimination, LAPACK (dsysv: Bunch-Kaufman), the host's pivoted LDL^T and the wide
windows' persistent Cholesky.  One line per case: eta in units of n 2^-53 for each solver, and the ratios device / model, device / LAPACK.

    python scripts/run_solve_accuracy.py --out profiles/solve_accuracy        # on an MI355X; writes solve_accuracy.json
    python scripts/run_solve_accuracy.py --no-gpu                              # model, LAPACK and host only
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.linalg as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _solve_cases as SC   # noqa: E402
from tests import _solve_ref as R      # noqa: E402
from voxel_slam_amd import vxba        # noqa: E402


def lapack_eta(c):
    A, b, idx = R.system(c["H"], c["J"], c["u"], c.get("E"), c.get("e"), c["dead"])
    if idx.size == 0:
        return 0.0
    return R.eta(A, b, sl.solve(A.astype(np.float64), b.astype(np.float64), assume_a="sym"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for solve_accuracy.json")
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    rows = []
    ratio, where = SC.measured_rounding_ratio()
    print(f"rounding ratio of the model's variants on the indefinite cases: {ratio:.3f} ({where}); K = {2 * ratio:.3f}")
    print(f"{'case':28s} {'device':>10s} {'model':>10s} {'lapack':>10s} {'host':>10s} {'dev/model':>10s} {'dev/lapack':>10s}   (eta / (n 2^-53))")
    for W in SC.NARROW_WINDOWS[1:]:
        for c in list(SC.narrow_cases(W)) + ([SC.li_case(W)] if W in SC.LI_WINDOWS else []):
            cap = 6 * W * R.U53
            if c["kind"] == "li":
                dev = None if args.no_gpu else vxba.debug_lm_solve(W, c["H"], c["J"], np.nan, None, li_rec=c["li_rec"], li_seq=1)["dxi"]
                host = None
            else:
                dev = None if args.no_gpu else vxba.debug_lm_solve(W, c["H"], c["J"], c["u"], c["Rp"])["dxi"]
                host = SC.case_eta(c, vxba.debug_host_damped_step(W, c["H"], c["J"], c["u"], c["Rp"])["dxi"])
            row = dict(case=f"W{W}-{c['name']}", n=6 * W, cap=cap, eta_device=None if dev is None else SC.case_eta(c, dev), eta_model=SC.case_eta(c, SC.model_dxi(c)),
                       eta_lapack=lapack_eta(c), eta_host=host)
            rows.append(row)
    for n in SC.WIDE_SIZES:
        for cond in SC.WIDE_CONDS:
            c = SC.wide_case(n, cond)
            A, b, idx = R.system(c["H"], c["J"], c["u"])
            dev = None
            if not args.no_gpu:
                got = vxba.debug_wide_solve(c["packed"], n, c["u"])
                dev = R.eta(A, b, got["dxi"][idx]) if got["info"] == 0 else float("nan")
            chol = R.eta(A, b, sl.cho_solve(sl.cho_factor(A.astype(np.float64), lower=True), b.astype(np.float64)))
            host = R.eta(A, b, vxba.debug_host_damped_step(n // 6, c["H"], c["J"], c["u"], np.tile(np.eye(3).reshape(-1).tolist() + [0, 0, 0], (n // 6, 1)))["dxi"][idx])
            rows.append(dict(case=c["name"], n=n, cap=n * R.U53, eta_device=dev, eta_model=None, eta_lapack=chol, eta_host=host))
    f = lambda v, cap: f"{v / cap:10.3g}" if v is not None else f"{'-':>10s}"
    q = lambda a, b: f"{a / b:10.3g}" if (a is not None and b) else f"{'-':>10s}"
    for r in rows:
        print(f"{r['case']:28s} {f(r['eta_device'], r['cap'])} {f(r['eta_model'], r['cap'])} {f(r['eta_lapack'], r['cap'])} {f(r['eta_host'], r['cap'])} "
              f"{q(r['eta_device'], r['eta_model'])} {q(r['eta_device'], r['eta_lapack'])}")
    dev = [r for r in rows if r["eta_device"] is not None]
    summary = dict(rounding_ratio=ratio, rounding_ratio_case=where, K=2 * ratio)
    if dev:
        summary["max_device_eta_over_cap"] = max(r["eta_device"] / r["cap"] for r in dev if "indef" not in r["case"])
        both = [r for r in dev if r["eta_model"]]
        summary["max_device_over_model"] = max(r["eta_device"] / r["eta_model"] for r in both)
        summary["max_device_over_model_indefinite"] = max(r["eta_device"] / r["eta_model"] for r in both if "indef" in r["case"])
    print(json.dumps(summary))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "solve_accuracy.json"), "w") as fh:
            json.dump(dict(summary=summary, unit="eta = ||b - A x|| / (||A|| ||x|| + ||b||), residual in longdouble; cap = n 2^-53", cases=rows), fh, indent=1)


if __name__ == "__main__":
    main()
