"""Corner extraction, CPU side: the numpy checker (tests/_corner_ref.py) against mathematics, the host build of the device arithmetic
(csrc/vxba_corner_math.hpp through tests/hostmath/corner_hostcheck.cpp) against the checker, and the honesty of every input the GPU suite
(tests/test_gpu_corner.py) runs: each case reaches what it claims, and no decision of the checker sits within 1e-9 of its threshold."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from tests import _corner_cases as CC
from tests import _corner_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
vp = C.c_void_p


@pytest.fixture(scope="module")
def hm():
    src = os.path.join(HERE, "hostmath", "corner_hostcheck.cpp")
    so = os.path.join(HERE, "hostmath", "libcorner_hostcheck.so")
    hdrs = [os.path.join(HERE, "..", "voxel-slam_amd", "csrc", h) for h in ("vxba_corner_math.hpp", "vxba_math.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    L = C.CDLL(so)
    L.cnh_extract.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp]
    L.cnh_counts.argtypes = [vp]
    L.cnh_read.argtypes = [vp] * 8
    L.cnh_solve.argtypes = [vp]
    L.cnh_fold.argtypes = [vp, vp]
    L.cnh_label.argtypes = [C.c_int, vp, vp]
    return L


def host_extract(L, xyz, p, planes=None):
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    prm = np.array([float(getattr(p, f.name)) for f in dataclasses.fields(p)])
    if planes is None:
        m, c, n = 0, np.zeros(3), np.zeros(3)
    else:
        c, n = np.ascontiguousarray(planes[0], dtype=np.float64), np.ascontiguousarray(planes[1], dtype=np.float64)
        m = c.shape[0]
    k = L.cnh_extract(xyz.shape[0], xyz.ctypes.data, prm.ctypes.data, m, c.ctypes.data, n.ctypes.data)
    assert k >= 0
    cnt = np.zeros(4, dtype=np.int32)
    L.cnh_counts(cnt.ctypes.data)
    P, M, Cn, K = (int(v) for v in cnt)
    out = dict(planes=np.zeros((P, 16)), labels=np.zeros(P, dtype=np.int32), proj=np.zeros((M, 16)), used=np.zeros(M, dtype=np.int32), ints=np.zeros((Cn, 6), dtype=np.int32),
               occ=np.zeros(Cn, dtype=np.uint64), loc=np.zeros((Cn, 3)), order=np.zeros(K, dtype=np.int32))
    L.cnh_read(*[out[k].ctypes.data for k in ("planes", "labels", "proj", "used", "ints", "occ", "loc", "order")])
    return out


def transcribed_labels(pred):
    """the two loops of BTC.cpp:353-382, literally, on a predicate matrix"""
    P = pred.shape[0]
    ids = [0] * P
    current_id = 1
    it = P - 1
    while it != 0:
        for it2 in range(0, it):
            if pred[it][it2]:
                if ids[it] == 0 and ids[it2] == 0:
                    ids[it] = current_id
                    ids[it2] = current_id
                    current_id += 1
                elif ids[it] == 0 and ids[it2] != 0:
                    ids[it] = ids[it2]
                elif ids[it] != 0 and ids[it2] == 0:
                    ids[it2] = ids[it]
        it -= 1
    return ids


def components(pred):
    P = pred.shape[0]
    lab = list(range(P))
    for _ in range(P):
        for i in range(P):
            for j in range(P):
                if pred[i][j] or pred[j][i]:
                    lab[i] = lab[j] = min(lab[i], lab[j])
    return lab


# ---- the checker against mathematics ------------------------------------------------------------------------------------------------
def test_translation_by_whole_voxels_moves_the_corners():
    case, ref = CC.get("standard")
    t = np.array([7.0, -12.0, 3.0])
    moved = R.extract(case["xyz"] + t, case["params"])
    assert np.array_equal(moved["labels"], ref["labels"]) and np.array_equal(moved["used"], ref["used"])
    assert np.array_equal(moved["occupancy"], ref["occupancy"]) and np.array_equal(moved["kept"], ref["kept"])
    assert np.abs(moved["locations"] - (ref["locations"] + t)).max() < 1e-9


def test_plane_records_against_eigh_and_direct_sums():
    case, ref = CC.get("standard")
    xyz, p = case["xyz"], case["params"]
    vi = R.voxel_index(xyz, p.voxel_size)
    assert np.array_equal(vi, np.floor(xyz / p.voxel_size).astype(np.int64) - ((xyz < 0) & (xyz / p.voxel_size == np.floor(xyz / p.voxel_size))))
    assert np.all(np.lexsort((ref["voxels"][:, 2], ref["voxels"][:, 1], ref["voxels"][:, 0])) == np.arange(ref["voxels"].shape[0]))      # ascending (x, y, z)
    for k in (0, 7, ref["planes"].shape[0] - 1):
        pts = xyz[np.all(vi == ref["voxels"][k], axis=1)]
        rec = ref["planes"][k]
        assert rec[9] == pts.shape[0] > p.voxel_init_num
        assert np.allclose(rec[0:3], pts.mean(axis=0), atol=1e-12)
        cov = np.cov(pts.T, bias=True)
        assert np.allclose(R.sym6_to_mat(rec[3:9]), cov, atol=1e-10)
        lam, vec = np.linalg.eigh(cov)
        assert lam[0] < p.plane_detection_thre and abs(abs(vec[:, 0] @ rec[10:13]) - 1) < 1e-9
        assert abs(rec[13] + rec[10:13] @ rec[0:3]) < 1e-12 and abs(rec[14] - np.sqrt(lam[2])) < 1e-9
        lead = np.argmax(np.abs(rec[10:13]))
        assert rec[10 + lead] > 0


def test_merged_record_is_the_record_of_the_union():
    rng = np.random.default_rng(1)
    sets = [rng.normal(size=(n, 3)) * np.array([1.0, 0.7, 0.01]) + rng.uniform(-3, 3, 3) for n in (40, 25, 60)]
    recs = []
    for s in sets:
        r = np.zeros(16); r[0:3] = s.mean(axis=0); c = np.cov(s.T, bias=True); r[3:9] = [c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]]; r[9] = s.shape[0]
        recs.append(r)
    out, sizes = R.fold_groups(np.array(recs), np.array([1, 1, 1]), False, R.Margins())
    allp = np.concatenate(sets)
    assert sizes == [3] and out[0, 9] == allp.shape[0]
    assert np.allclose(out[0, 0:3], allp.mean(axis=0), atol=1e-12) and np.allclose(R.sym6_to_mat(out[0, 3:9]), np.cov(allp.T, bias=True), atol=1e-12)
    lam, vec = np.linalg.eigh(np.cov(allp.T, bias=True))
    assert abs(abs(vec[:, 0] @ out[0, 10:13]) - 1) < 1e-9 and abs(out[0, 14] - np.sqrt(lam[2])) < 1e-12


def test_labelling_is_the_reference_loops_and_not_connected_components():
    rng = np.random.default_rng(2)
    for P, dens in ((2, 0.9), (7, 0.3), (12, 0.15), (25, 0.05)):
        for _ in range(20):
            a = rng.random((P, P)) < dens
            pred = a | a.T
            ids, _ = R.label_rows(pred)
            assert list(ids) == transcribed_labels(pred)
    # 3 - 0 and 2 - 1 take ids of their own before 1 - 0 is visited, where both are set and nothing happens: connected components would join all four
    pred = np.zeros((4, 4), dtype=bool)
    for i, j in ((3, 0), (2, 1), (1, 0)):
        pred[i, j] = pred[j, i] = True
    ids, _ = R.label_rows(pred)
    assert list(ids) == transcribed_labels(pred) == [1, 2, 2, 1]
    assert len(set(components(pred))) == 1 and len(set(ids)) == 2


def test_sign_rule_mirror_image():
    case, ref = CC.get("small")
    mirror = case["xyz"] * np.array([1.0, -1.0, 1.0]) + np.array([0.0, 0.0, 0.0])
    m = R.extract(mirror, case["params"])
    # the voxel partition of the mirrored cloud differs (y -> -y moves points across the asymmetric truncation), so compare the merged floor only
    a, b = ref["proj"][0], m["proj"][0]
    assert a[9] == b[9]
    lead = np.argmax(np.abs(a[10:13]))
    assert a[10 + lead] > 0 and b[10 + np.argmax(np.abs(b[10:13]))] > 0
    assert np.allclose(np.abs(a[10:13]), np.abs(b[10:13]), atol=1e-9)
    # a record solved twice with the opposite covariance orientation keeps the rule
    r = ref["planes"][0].copy(); R.solve(r)
    assert np.array_equal(r[10:13], ref["planes"][0][10:13])


def test_ordering_rules():
    rows = np.zeros((5, 16)); rows[:, 9] = [30, 50, 30, 50, 10]; rows[:, 0] = np.arange(5)
    assert list(R.sort_by_size(rows)[:, 0]) == [1, 3, 0, 2, 4]                             # stable ties
    summ = np.array([12, 15, 12, 15, 11, 12])
    kept = np.array([0, 1, 2, 3, 5])
    assert list(R.cut(kept, summ, 6)) == [0, 1, 2, 3, 5]                                   # useful > count: everything in order
    assert list(R.cut(kept, summ, 5)) == [1, 3, 0, 2, 5]                                   # equal: sorted, stable
    assert list(R.cut(kept, summ, 3)) == [1, 3, 0]
    _, ref = CC.get("standard")
    key = [(c["plane"], c["cell_x"] // 5, c["cell_y"] // 5) for c in ref["candidates"]]
    assert key == sorted(key) and len(set(key)) == len(key)                               # candidates in (plane, segment x, segment y) order
    loc = np.array([[0, 0, 0], [1, 0, 0], [5, 0, 0], [5.5, 0, 0]], dtype=float)
    assert list(R.suppress(loc, np.array([10, 10, 12, 11]), 2.0, R.Margins())) == [False, False, True, False]      # equal neighbours drop each other


# ---- the host build of the device arithmetic against the checker ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_host_build_equals_the_checker(hm, name):
    case, ref = CC.get(name)
    got = host_extract(hm, case["xyz"], case["params"], case["planes"])
    if case["planes"] is None:
        assert np.array_equal(got["labels"], ref["labels"])
        assert np.array_equal(got["planes"][:, 9], ref["planes"][:, 9])
        assert np.abs(got["planes"] - ref["planes"]).max(initial=0) < 1e-9
    assert np.array_equal(got["used"], ref["used"]) and np.array_equal(got["proj"][:, 9], ref["proj"][:, 9])
    assert np.abs(got["proj"] - ref["proj"]).max(initial=0) < 1e-9
    rc = ref["candidates"]
    assert got["ints"].shape[0] == len(rc)
    assert np.array_equal(got["ints"][:, :5], np.array([[c["plane"], c["cell_x"], c["cell_y"], c["count"], c["summary"]] for c in rc], dtype=np.int32).reshape(-1, 5))
    assert np.array_equal(got["occ"], np.array([c["occupancy"] for c in rc], dtype=np.uint64).reshape(-1))
    assert np.array_equal(got["ints"][:, 5].astype(bool), ref["kept"]) and np.array_equal(got["order"], ref["order"])
    assert np.abs(got["loc"] - np.array([c["location"] for c in rc]).reshape(-1, 3)).max(initial=0) < 1e-9


def test_host_pieces(hm):
    rng = np.random.default_rng(5)
    for _ in range(10):
        P = 9
        a = rng.random((P, P)) < 0.3
        pred = np.ascontiguousarray(a | a.T, dtype=np.uint8)
        ids = np.zeros(P, dtype=np.int32)
        hm.cnh_label(P, pred.ctypes.data, ids.ctypes.data)
        assert list(ids) == transcribed_labels(pred.astype(bool))
    _, ref = CC.get("small")
    a, b = ref["planes"][0].copy(), ref["planes"][1].copy()
    a2 = a.copy(); R.fold(a2, b)
    hm.cnh_fold(a.ctypes.data, b.ctypes.data)
    assert np.array_equal(a[:10], a2[:10])                                                # the fold is restated bit for bit
    R.solve(a2); hm.cnh_solve(a.ctypes.data)
    assert np.abs(a - a2).max() < 1e-12


# ---- honesty of the GPU inputs -------------------------------------------------------------------------------------------------------
MARGIN = 1e-9
SUPPRESSION_MARGIN = 1e-4       # a location within round-off of a float32 rounding boundary moves the squared distance by an ulp: ~1e-6 of radius^2


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_gpu_inputs_keep_every_decision_off_its_threshold(name):
    case, ref = CC.get(name)
    mg = ref["margins"]
    for k, v in mg.items():
        assert v > (SUPPRESSION_MARGIN if k == "suppression" else MARGIN), (k, v)
    n = case["xyz"].shape[0]
    assert 2000 <= n <= 24000
    if case["planes"] is None:
        assert ref["planes"].shape[0] <= 600
        assert all(g >= 0.05 for g in ref["used_gaps"]) or "fallback" in case["needs"]     # the used planes' normals: 1e-15 |cov| / gap radians between two solvers
        assert np.abs(case["xyz"]).max() <= 100.0
    for im in ref["images"]:
        if im["valid"]:
            assert im["cells"] <= 5000


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_gpu_inputs_reach_what_they_claim(name):
    case, ref = CC.get(name)
    needs = case["needs"]
    cands = ref["candidates"]
    for need in needs:
        if need == "merges":
            assert ref["group_sizes"] and ref["merged_first"] >= 1
        elif need == "group3":
            assert max(ref["group_sizes"]) >= 3
        elif need == "late":
            assert len(ref["late"]) >= 1
        elif need == "corners10":
            assert ref["locations"].shape[0] >= 10
        elif need == "corners1":
            assert ref["locations"].shape[0] >= 1
        elif need == "two_planes":
            assert (ref["used"] >= 0).sum() == 2 and all(im["valid"] for im in ref["images"])
        elif need == "second_plane_corners":
            assert any(cands[k]["plane"] == 1 for k in ref["order"])
        elif need == "all_negative":
            assert (case["xyz"] < 0).all()
        elif need == "anchored":
            assert ref["images"][0]["min_x"] == 10.0 and ref["images"][1]["min_x"] < -10.0
            assert ref["images"][1]["x_len"] == int((-10.0 - ref["images"][1]["min_x"]) / 0.5 + 5)       # max_x = -10: every px lies below it
        elif need == "planes_exist":
            assert ref["planes"].shape[0] >= 3
        elif need == "no_merge":
            assert not ref["group_sizes"] and ref["merged_first"] == 0 and not np.any(ref["labels"])
        elif need == "fallback":
            assert ref["proj"].shape[0] == 1 and np.array_equal(ref["proj"][0, 10:13], [0.0, 0.0, 1.0]) and np.array_equal(ref["proj"][0, 0:3], case["xyz"][0])
            assert len(cands) >= 1
        elif need == "one_projection_plane":
            assert ref["merged_first"] == 1 and ref["proj"].shape[0] == 1 and case["params"].proj_plane_num == 2 and list(ref["used"]) == [0]
        elif need == "gate_skips_second":
            assert list(ref["used"]) == [0, -1, 1]
        elif need == "first_image_invalid":
            assert not ref["images"][0]["valid"] and 0 < ref["images"][0]["kept"] <= 5 and ref["images"][1]["valid"] and all(c["plane"] == 1 for c in cands)
        elif need == "special_point_in_candidate":
            sp = case["special"]
            assert sp[2] == case["params"].proj_dis_max
            img = ref["images"][0]
            px, py = float(sp @ img["y_axis"]), float(sp @ img["x_axis"])
            cell = (int((px - img["min_x"]) / 0.5), int((py - img["min_y"]) / 0.5))
            hit = [c for c in cands if (c["cell_x"], c["cell_y"]) == cell]
            assert len(hit) == 1 and hit[0]["occupancy"] >> 50 == 0
            inside = R.extract(np.concatenate([case["xyz"][:-1], [sp - np.array([0, 0, 1e-6])]]), case["params"], case["planes"])      # the same point just inside: bit 49, same count
            twin = [c for c in inside["candidates"] if (c["cell_x"], c["cell_y"]) == cell][0]
            assert twin["count"] == hit[0]["count"] and twin["summary"] == hit[0]["summary"] + 1 and not (hit[0]["occupancy"] >> 49) & 1
        elif need == "border_drop":
            tab = ref["images"][0]["cell_table"]
            col0 = {k: v for k, v in tab.items() if k[0] == 0}
            assert col0 and max(bin(o).count("1") for _, o in col0.values()) >= case["params"].summary_min_thre and not [c for c in cands if c["cell_x"] == 0]
        elif need == "straddle_first_wins":
            tab = ref["images"][0]["cell_table"]
            first = [c for c in cands if c["cell_x"] % 5 == 1 and (c["cell_x"] + 1, c["cell_y"]) in tab]
            assert first and any(bin(tab[(c["cell_x"] + 1, c["cell_y"])][1]).count("1") == c["summary"] for c in first)
        elif need == "equal_neighbours_drop":
            pairs = [(a, b) for a in range(len(cands)) for b in range(a + 1, len(cands)) if cands[a]["summary"] == cands[b]["summary"]
                     and np.linalg.norm(cands[a]["location"] - cands[b]["location"]) < 1.0 and cands[a]["cell_x"] // 5 != cands[b]["cell_x"] // 5]
            assert pairs and all(not ref["kept"][a] and not ref["kept"][b] for a, b in pairs)
        elif need == "touch_drops":
            off = R.extract(case["xyz"], dataclasses.replace(case["params"], touch_filter_enable=0), case["planes"])
            gone = [c for c in off["candidates"] if (c["cell_x"], c["cell_y"]) not in {(k["cell_x"], k["cell_y"]) for k in cands}]
            assert gone and all(not c["occupancy"] & 15 for c in gone) and len(off["candidates"]) == len(cands) + len(gone) and len(cands) >= 1
        elif need == "cut_num_64":
            p = case["params"]
            assert int((p.proj_dis_max - p.proj_dis_min) / p.proj_image_high_inc) == 64
        else:
            raise AssertionError(f"unknown need {need}")


def test_the_checker_chain_finds_the_revisit_of_the_end_to_end_stream():
    """tests/_keyframe_ref -> tests/_corner_ref -> tests/_loopsearch_ref on the stream the end-to-end GPU test runs: the second keyframe finds the first,
    and no decision of either corner extraction sits within 1e-9 of its threshold."""
    from tests import _keyframe_ref as KR
    from tests import _loopreg_ref as LR
    from tests import _loopsearch_ref as S
    st = CC.stream_case()
    kr = KR.KeyframeRef(st["win"], 1.0)
    kfs = []
    for s in st["scans"]:
        if kr.push_scan(*s):
            kfs.append(kr.keyframe)
    assert len(kfs) == 2
    cs = [R.extract(k["full"].astype(np.float64)) for k in kfs]
    for c in cs:
        assert c["locations"].shape[0] >= 5 and all(g >= 0.05 for g in c["used_gaps"])
        for k, v in c["margins"].items():
            assert v > (SUPPRESSION_MARGIN if k == "suppression" else MARGIN), (k, v)
    sp = dataclasses.replace(S.Params(), skip_near_num=-1)
    rows = [LR.plane_cloud(k["full"].astype(np.float64))["rows"] for k in kfs]
    db = S.Database()
    db.add(S.describe(cs[0]["locations"], cs[0]["occupancy"], sp), rows[0])
    w = db.search(S.describe(cs[1]["locations"], cs[1]["occupancy"], sp), rows[1], sp)
    assert w["frame"] == 0 and w["score"] > sp.icp_threshold and w["candidates"][0]["max_vote"] >= 4
    assert np.linalg.norm(w["pose"][9:12] - np.array([0.45, 0.06, 0.0])) < 0.1            # the second visit stands 0.45 m further along x


def test_golden_regenerates():
    import importlib.util
    spec = importlib.util.spec_from_file_location("tests._make_golden_corner", os.path.join(HERE, "golden", "corner", "make_golden_corner.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = mod.build()
    with np.load(mod.PATH) as z:
        assert sorted(z.files) == sorted(want)
        for k in want:
            if k == "locations":
                assert np.abs(z[k] - want[k]).max() < 1e-12      # numpy.linalg.eigh may differ in the last bits between builds
            else:
                assert np.array_equal(z[k], want[k]), k
        assert z["locations"].shape[0] >= 3
