"""The inputs tests/test_gpu_corner.py runs, shared with tests/test_corner_cpu.py, which shows on the CPU that each holds what it claims and that no
decision of the checker (tests/_corner_ref.py) sits closer than 1e-9 to its threshold.  Every case is a dict(xyz, params, planes (None = the whole
chain, else (centres, normals) for extract_with_planes), needs: the properties the case must reach -- asserted by the CPU test)."""
import dataclasses
import functools

import numpy as np

from tests import _corner_ref as R


def _synth():
    from voxel_slam_amd import synth
    return synth


def scene(**kw):
    kw.setdefault("extent", 16.0)
    kw.setdefault("n_poles", 14)
    return _synth().make_corner_scene(**kw)[0]


def pole(rng, x, y, z0, h, n, radius=0.12):
    ang, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, h, n)
    return np.stack([x + radius * np.cos(ang), y + radius * np.sin(ang), z0 + z], axis=1)


def floor(rng, half, n, noise=0.01):
    return np.stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), noise * rng.normal(size=n)], axis=1)


def case_standard():
    return dict(xyz=scene(), params=R.Params(), planes=None, needs=("merges", "group3", "late", "corners10", "two_planes"))


def case_high_fly():
    return dict(xyz=scene(), params=R.high_fly(), planes=None, needs=("merges", "corners1"))


def case_negative():
    """the standard scene moved by whole voxels so that every coordinate is negative"""
    xyz = scene(seed=4242) + np.array([-40.0, -30.0, -20.0])
    assert (xyz < 0).all()
    return dict(xyz=xyz, params=R.Params(), planes=None, needs=("merges", "corners10", "all_negative", "two_planes", "second_plane_corners"))


def case_anchor():
    """centres far from the data along the image axes: one image anchored at min_x = 10 (every px > 10), one at max_x = -10 (every px < -10)"""
    xyz = scene(seed=77, extent=12.0, n_poles=8)
    n = np.array([0.0, 0.0, 1.0])
    xa, ya = R.axes(n)
    c = np.array([0.0, 0.0, -0.37])
    return dict(xyz=xyz, params=dataclasses.replace(R.Params(), proj_plane_num=2), planes=(np.stack([c - 25.0 * ya, c + 25.0 * ya + 3.0 * xa]), np.stack([n, n])),
                needs=("anchored", "corners1"))


def case_no_merge():
    """three plane patches in voxels of their own with three orientations, and poles: no pair passes, the fallback plane (0, 0, 1) at the first point"""
    rng = np.random.default_rng(31)
    parts = []
    for o, u, v in (((0.2, 0.2, 0.5), (1, 0, 0), (0, 1, 0)), ((5.2, 0.2, 0.2), (0, 1, 0), (0, 0, 1)), ((0.2, 5.5, 0.2), (1, 0, 0), (0, 0, 1))):
        a, b = rng.uniform(0, 0.6, 60), rng.uniform(0, 0.6, 60)
        nrm = np.cross(u, v)
        parts.append(np.asarray(o) + a[:, None] * np.asarray(u, dtype=float) + b[:, None] * np.asarray(v, dtype=float) + 0.005 * rng.normal(size=60)[:, None] * nrm)
    for x, y in ((2.5, 2.5), (-3.5, 1.5), (1.5, -4.5), (6.5, 6.5)):
        parts.append(pole(rng, x, y, 0.0, 3.0, 600, radius=0.2))
    parts.append(np.stack([rng.uniform(-6, 8, 1500), rng.uniform(-6, 8, 1500), rng.uniform(-0.4, 0.4, 1500)], axis=1))      # a thick slab: no plane voxel
    return dict(xyz=np.concatenate(parts), params=R.Params(), planes=None, needs=("planes_exist", "no_merge", "fallback"))


def case_one_plane():
    """a floor and poles at voxel centres only: every floor voxel joins one group, the list of one passes through merge_plane; proj_plane_num = 2
    exceeds the list"""
    rng = np.random.default_rng(5)
    parts = [floor(rng, 4.9, 4000) + np.array([0.0, 0.0, -0.37])]
    for x, y, h in ((1.5, 0.5, 3.0), (-2.5, 2.5, 2.2), (2.5, -3.5, 3.6), (-3.5, -1.5, 1.4)):
        parts.append(pole(rng, x, y, -0.37, h, int(300 * h), radius=0.2))
    return dict(xyz=np.concatenate(parts), params=R.Params(), planes=None, needs=("one_projection_plane", "corners1"))


def case_opposite():
    """the second plane nearly opposite to the first: the gate skips it and uses the third"""
    xyz = scene(seed=9, extent=12.0, n_poles=8)
    c = np.array([[0.0, 0.0, -0.37], [0.0, 0.0, -0.37], [5.82, 0.0, 1.0]])
    n2 = np.array([0.02, 0.0, -1.0]); n2 /= np.linalg.norm(n2)
    return dict(xyz=xyz, params=R.Params(), planes=(c, np.stack([[0.0, 0.0, 1.0], n2, [1.0, 0.0, 0.0]])), needs=("gate_skips_second", "corners1"))


def case_few_points():
    """four points within dis_max of the first plane: it yields nothing, the second still does"""
    rng = np.random.default_rng(3)
    xyz = np.concatenate([scene(seed=9, extent=12.0, n_poles=8), np.array([0.0, 0.0, 100.0]) + rng.uniform(-1, 1, (4, 3))])
    return dict(xyz=xyz, params=R.Params(), planes=(np.array([[0.0, 0.0, 100.0], [0.0, 0.0, -0.37]]), np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])),
                needs=("first_image_invalid", "corners1"))


def _flat(seed, half=6.0, n_floor=6000):
    rng = np.random.default_rng(seed)
    return rng, [floor(rng, half, n_floor)]


def case_dis_max():
    """an axis-aligned plane z = 0 and a pole with one point at z = 5.0 exactly: dis == dis_max, bit index == cut_num: counted, no bit"""
    rng, parts = _flat(11)
    for x, y in ((1.3, 0.4), (-2.2, 2.9), (3.1, -3.3)):
        parts.append(pole(rng, x, y, 0.0, 4.9, 900))
    special = np.array([[1.3, 0.4, 5.0]])
    return dict(xyz=np.concatenate(parts + [special]), params=R.Params(), planes=(np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])), special=special[0],
                needs=("special_point_in_candidate",))


def case_border_straddle():
    """plane z = 0 through the origin: a pole beyond the floor at the smallest px (cell x = 0: its segment's winner sits on the border and is dropped), a
    pole centred on a cell edge inside a segment (two cells of equal summary: the first wins) and one centred on a segment edge (two candidates of
    equal summary within the radius: they drop each other)"""
    rng, parts = _flat(21)
    n = np.array([0.0, 0.0, 1.0])
    xa, ya = R.axes(n)
    border = pole(rng, *(-13.0 * ya[:2]), 0.0, 3.0, 900)                                 # px ~ -13: the image's min_x
    parts.append(border)
    min_x = float(((border @ ya)).min())                                                # dy = 0: px = p . y_axis
    py0 = 0.1
    for k in (2 + 5 * 4, 5 * 7):                                                         # a cell edge inside segment 4, the edge between segments 6 and 7
        ctr = (min_x + 0.5 * k) * ya + py0 * xa
        parts.append(pole(rng, ctr[0], ctr[1], 0.0, 3.0, 2400, radius=0.1))
        py0 += 2.6
    return dict(xyz=np.concatenate(parts), params=R.Params(), planes=(np.zeros((1, 3)), n[None, :]), needs=("border_drop", "straddle_first_wins", "equal_neighbours_drop"))


def case_touch():
    """the touch filter on: a pole hanging from 1 m to 3.5 m beyond the floor has none of bits 0..3"""
    rng, parts = _flat(41)
    for x, y in ((1.3, 0.4), (-2.2, 2.9), (3.1, -3.3)):
        parts.append(pole(rng, x, y, 0.0, 3.0, 900))
    parts.append(pole(rng, 8.6, 0.3, 1.0, 2.5, 900))
    parts.append(pole(rng, 11.9, 0.3, 0.0, 0.3, 200))                                    # keeps the hanging pole off the image border
    return dict(xyz=np.concatenate(parts), params=dataclasses.replace(R.Params(), touch_filter_enable=1), planes=(np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])),
                needs=("touch_drops",))


def case_cut_num_64():
    return dict(xyz=scene(seed=9, extent=12.0, n_poles=8), params=dataclasses.replace(R.Params(), proj_image_high_inc=0.125, proj_dis_max=8.0), planes=None,
                needs=("cut_num_64", "corners1"))


def case_large():
    """the first of two calls on one handle: about 20 000 points"""
    return dict(xyz=scene(seed=123, extent=18.0, n_poles=16, density=34.0), params=R.Params(), planes=None, needs=("corners10",))


def case_small():
    """the second: about 2 000"""
    return dict(xyz=scene(seed=124, extent=6.0, n_poles=3, n_boxes=1, n_walls=2, density=24.0), params=R.Params(), planes=None, needs=("merges",))


CASES = dict(standard=case_standard, high_fly=case_high_fly, negative=case_negative, anchor=case_anchor, no_merge=case_no_merge, one_plane=case_one_plane, opposite=case_opposite,
             few_points=case_few_points, dis_max=case_dis_max, border_straddle=case_border_straddle, touch=case_touch, cut_num_64=case_cut_num_64, large=case_large, small=case_small)


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, the checker's result), computed once and shared; neither is to be modified"""
    c = CASES[name]()
    c["xyz"] = np.ascontiguousarray(c["xyz"], dtype=np.float64)
    c["xyz"].setflags(write=False)
    return c, R.extract(c["xyz"], c["params"], c["planes"])


@functools.lru_cache(maxsize=None)
def stream_case():
    """The end-to-end input: six ScanPoses (win_size 3: two keyframes) of one corner scene seen twice from poses 0.45 m and 1.5 degrees apart -- a
    revisit.  dict(win, scans: [(pose, v6, body points, None)])."""
    return dict(win=3, scans=_synth().make_corner_revisit_stream(2, 3, seed=55))
