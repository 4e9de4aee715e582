"""Writes tests/golden/corner/corner.npz: the `small` case of tests/_corner_cases.py (its cloud) and what the numpy checker tests/_corner_ref.py makes of
it -- the corner set, the candidates and the suppression verdicts.  __graft_entry__.smoke() runs the cloud through vxba.CornerExtractor against it;
tests/test_corner_cpu.py checks that the file regenerates.  Run from the repository root: python tests/golden/corner/make_golden_corner.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "corner.npz")


def build():
    from tests import _corner_cases as CC
    case, ref = CC.get("small")
    c = ref["candidates"]
    return dict(xyz=case["xyz"], locations=ref["locations"], occupancy=ref["occupancy"], summary=ref["summary"],
                cand_ints=np.array([[k["plane"], k["cell_x"], k["cell_y"], k["count"], k["summary"]] for k in c], dtype=np.int32).reshape(-1, 5),
                cand_kept=ref["kept"], labels=ref["labels"], used=ref["used"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
    np.savez_compressed(PATH, **build())
    print(PATH, os.path.getsize(PATH), "bytes")
