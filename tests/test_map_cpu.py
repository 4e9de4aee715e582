"""The local map's reference and cases held to account without a GPU (tests/_map_ref.py, tests/_map_cases.py; the GPU side is
tests/test_gpu_map_exact.py).

1. The reference is pinned: bit-identical to the oracle's LocalMap (structure, sums, stored points, after every stage) on every window-form case,
   and to the `fix0` stage of tests/golden/map_fix/map_fix_cycle.npz (the reference project's own cut_voxel fix form) on the golden's inputs.
2. The census: every path the cases were built for is taken by at least one leaf -- single / multi tile folds, the `tmp` re-bucketing, the
   serial fix copy, fc = 0 with pcr_fix.N != 0, the 64-point seams of the two push kernels, windows of 1 / 3 / 16, every branch of margi and
   each side of every integer gate -- and every real-valued decision clears its threshold by 100 x the eigenvalue criterion.
3. The oracle meets every criterion at 2 K on the window-form cases, and so does the float64 restatement (Cs.HostSide: the reference's structure
   with the kernels' own arithmetic built for the host) on every case, the fix form included.
4. Degraded variants of the reference are rejected: the bit-for-bit ones because their tables or stored points differ from the honest
   reference's (which is the oracle's, by 1), the arithmetic ones because the honest oracle then misses exactly the criterion meant for them.

The eleven bit-for-bit variants (remainder tile dropped, tile order, unstable re-bucket, region order after a move, `>=` in the octant test, fused
to_world, each integer gate off by one) all PASS the older tests (tests/test_gpu_map.py, test_gpu_map_fix.py, the goldens) as far as the tile, order
and seam variants go, because no input of those tests reaches the paths they change: a leaf there never splits with more than 51 points of one
scan or 97 fix points.  That is the larger gap; the list below is about the arithmetic variants only.

What the whole-array tolerances of tests/test_gpu_map.py make of the arithmetic variants, measured on the leaf tables of this module's
cases (15 tables behind margi, 1 to 8 updated plane leaves each; a variant counts as accepted when no table rejects it;
test_what_the_old_tolerances_accept asserts exactly this list):

    accepted:
        radius_double      radius left in double instead of rounded to float         relative step 2.1e-11 .. 4.5e-8 against `rtol 1e-6`
    rejected (smallest .. largest whole-array `rel` over the tables, against `rel(plane_var) < 1e-5` / `rel(pcr_add) < 1e-9`):
        pv_nc_transposed   the normal-centre block of plane_var transposed           2.0e-3 .. 6.5e-2
        pv_centre_scale    the centre block scaled by 1/N once instead of twice      2.2e-2 .. 5.0
        pv_gap_sign        lamk - lam0 for lam0 - lamk                               1.0e-2 .. 2.0e-1
        tr_cross           cl_transform with R v p^T for both cross terms            4.4e-2 where the pose has a translation (equal at identity)

So on tables this small, where the whole-array maximum is the leaf's own, a whole block gone wrong is caught; what `rel < 1e-5` cannot see is
an error of a few per cent of the normal-centre or centre-centre block on the large sessions, whose maximum sits in a normal-normal block 1e2
to 1e4 times larger (the blocks' sizes differ by that much here too: see K_PV's magnitudes).  The per-block criterion bounds each block at a
few u of its own magnitude.
"""
import importlib.util
import os

import numpy as np
import pytest

from tests import _map_cases as Cs
from tests import _map_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_CASES = [c["name"] for c in Cs.all_cases() if Cs.oracle_can_run(c)]


@pytest.fixture(scope="module")
def alone():
    """Every case through the reference alone: name -> (reference, snapshots)."""
    out = {}
    for case in Cs.all_cases():
        snaps = []
        ref, _ = Cs.run(case, None, snaps=snaps)
        out[case["name"]] = (ref, snaps)
    return out


@pytest.fixture(scope="module")
def on_oracle():
    """Every window-form case through the reference and the oracle in lockstep (this asserts the pin): name -> (reference, errors, old figures)."""
    out = {}
    for name in ORACLE_CASES:
        case = Cs.get_case(name)
        old = []
        ref, err = Cs.run(case, Cs.OracleSide(case["prm"]), old=old)
        out[name] = (ref, err, old)
    return out


def census(alone, op, case=None, **match):
    return [e for name, (ref, _) in alone.items() if case is None or name.startswith(case) for e in ref.census
            if e["op"] == op and all(e.get(k) == v for k, v in match.items())]


# ---- 1. the pins ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_reference_is_the_oracle_bit_for_bit_and_the_oracle_meets_the_criteria(on_oracle, name):
    _, err, _ = on_oracle[name]                      # Cs.run has compared every stage bit for bit
    Cs.check_errors(err, Cs.FACTOR_CPU, label=name)


def test_reference_reproduces_the_fix_form_golden():
    spec = importlib.util.spec_from_file_location("tests._make_golden_map_fix", os.path.join(HERE, "golden", "map_fix", "make_golden_map_fix.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from tests.test_oracle_octree import to_world
    g, inp = G.load_fixture(), G.inputs()
    ref = R.RefMap(win_size=G.WIN, **inp["kw"])
    for k in range(4):
        s = slice(inp["fp"][k], inp["fp"][k + 1])
        ref.cut_voxel_fix(np.ascontiguousarray(to_world(inp["poses_gt"][k], inp["xyz"][s])[::2]), None, float(k))
    lv = ref.leaves()
    assert np.array_equal(lv["node_id"], g["fix0_node_id"])
    assert np.array_equal(lv["pcr_fix"], g["fix0_pcr_fix"]) and np.array_equal(lv["pcr_add"], g["fix0_pcr_add"])
    for key in ("layer", "isexist", "is_plane", "has_sw", "in_slide", "last_num", "n_point_fix", "n_points"):
        assert np.array_equal(np.asarray(lv[key]).astype(np.int64), g[f"fix0_{key}"].astype(np.int64)), key


# ---- 2. census and margins --------------------------------------------------------------------------------------------------------------
def test_every_subdivision_path_is_taken(alone):
    for pc in Cs.PC_LADDER:
        want = "tile" if pc <= R.SUB_TILE else "rebucket"
        assert census(alone, "sub_scan", case=f"pc{pc}_single", pc=pc, layer=0, path=want), pc
    assert census(alone, "sub_scan", case="pc129_single_vs0.5", pc=129, path="rebucket")
    for pc in Cs.PC_LADDER[1:]:                                        # three scans in the window, the second with one point
        ev = census(alone, "sub_scan", case=f"pc{pc}_three", layer=0)
        assert sorted((e["scan"], e["pc"]) for e in ev) == [(0, max(pc, 21)), (1, 1), (2, pc)], ev
    # a child at layer 1 with more than one tile of one scan that splits again: the multi-tile fold over an already re-bucketed range.  (The `tmp`
    # re-bucketing itself cannot run a second time: children keep points only where layer + 1 < max_layer, and vxba_map_create refuses max_layer > 2.)
    assert [e for e in census(alone, "sub_scan", case="pc257", layer=1) if e["pc"] > R.SUB_TILE]
    for fc in Cs.FC_LADDER:
        assert census(alone, "sub_fix", case=f"fc{fc}_ml2", fc=fc, keep=True, path="tile" if fc <= R.SUB_TILE else "serial"), fc
        assert census(alone, "sub_fix", case=f"fc{fc}_ml1", fc=fc, keep=False), fc
    assert census(alone, "sub_fix", case="fc0_capped", fc=0, path="none")
    assert census(alone, "sub_fix", case="pool_moves_compact", fc=269, path="serial") and census(alone, "sub_fix", case="fix_runs", path="serial")


def test_the_push_kernels_meet_their_seams(alone):
    runs = census(alone, "fix_push", case="fix_runs")
    first = [e for e in runs if e["had"] == 0]
    assert sorted(e["run"] for e in first) == sorted(Cs.FIX_RUNS) and all(e["fill"] == "grown" and not e["moved"] for e in first)
    assert {e["fill"] for e in runs} == {"grown", "exact", "room"}
    assert [e for e in runs if e["moved"] and e["run"] > R.FIX_TILE] and [e for e in runs if e["moved"] and e["run"] < R.FIX_TILE]
    # map_push_kernel: node indices follow the order the roots were made in, so the sorted run heads are the running sums
    ref, _ = alone["push_seams"]
    stage = min(e["stage"] for e in ref.census if e["op"] == "push")
    lens = [e["run"] for e in sorted((e for e in ref.census if e["op"] == "push" and e["stage"] == stage), key=lambda e: e["node"])]
    assert tuple(lens) == Cs.PUSH_RUNS
    heads = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert {0, 63, 64, 65} <= set(heads.tolist())
    assert any(h // 64 != (h + n - 1) // 64 for h, n in zip(heads, lens)) and 65 in lens


def test_the_window_edges(alone):
    assert {c["prm"]["win_size"] for c in Cs.all_cases()} >= {1, 3, 16}
    case = Cs.get_case("window16")
    assert len(case["ops"]) >= 20
    ref, _ = alone["window16"]
    assert sorted(e["scan"] for e in ref.census if e["op"] == "sub_scan" and e["layer"] == 0) == list(range(16))      # sixteen scans in the window of the leaf that splits
    assert len([e for e in ref.census if e["op"] == "margi"]) >= 6


def test_every_margi_branch_and_gate(alone):
    m = lambda **kw: census(alone, "margi", case="margi", **kw)
    mp_ = Cs.get_case("margi")["prm"]["max_points"]
    assert m(adopt=True, updated=True) and m(adopt=False, is_plane=True, updated=True)          # the cache adopted; a thick plane recomputed
    assert m(adopt=False, is_plane=False)
    assert m(empty_oldest=True) and m(empty_oldest=False)
    assert m(move="light", fill=-1) and m(move="light", fill=0) and m(move="heavy", fill=1)
    assert m(Nfix=mp_ - 1, capped=False, empty_oldest=False) and m(Nfix=mp_, capped=True, empty_oldest=False) and m(Nfix=mp_ + 1, capped=True, empty_oldest=False)
    assert m(diff=4, updated=False, is_plane=True, capped=False) and m(diff=5, updated=True, is_plane=True)
    assert [e for e in m(last_num=10, updated=True) if e["diff"] < 5] and [e for e in m(last_num=11, updated=False, capped=False) if e["diff"] < 5]
    assert m(isexist_gap=0) and m(isexist_gap=1)
    j = lambda **kw: census(alone, "judge", case="margi", **kw)
    assert j(N=5, min_point=5) and j(N=6, min_point=5)
    # the thick plane never reaches the factor, the thin ones do
    ref, _ = alone["margi"]
    assert {x["what"] for x in ref.margins} == {"min_eigen_value", "thre", "ratio_0.12"}


def test_no_decision_is_within_reach_of_rounding(alone):
    """lam0 < min_eigen_value, lam0 / lam2 < thre, lam0 / lam1 > 0.12: every one, no leaf excluded."""
    n = 0
    for name, (ref, _) in alone.items():
        for x in ref.margins:
            assert x["margin"] >= Cs.HONEST * Cs.FACTOR_DEVICE * Cs.K_EIG, (name, x)
            n += 1
    assert n > 500


def test_geometry_edges_are_decided_as_the_oracle_decides_them(alone, on_oracle):
    ref, _ = alone["edges"]
    lv = ref.leaves()
    roots = sorted({int(i) >> 16 for i in lv["node_id"]})
    key = lambda x, y, z: ((x + 32768) << 32) | ((y + 32768) << 16) | (z + 32768)
    # y = -2 exactly steps down to voxel -3 and y = -1 exactly to voxel -2; float(4 - 1e-9) = 4 is the next voxel; -0.0 is voxel 0; -1e-9 is voxel -1
    assert set(roots) == {key(3, -2, 0), key(3, -3, 0), key(4, -2, 0), key(-1, -1, 0)}
    assert "edges" in on_oracle


# ---- 4. degraded variants ---------------------------------------------------------------------------------------------------------------
WHERE = {"drop_remainder_tile": "pc129_single_vs1.0", "second_tile_first": "pc129_single_vs1.0", "unstable_rebucket": "pc129_single_vs1.0", "fix_region_order": "margi",
         "octant_ge": "edges", "fused_to_world": "pc129_three", "gate_min_point": "margi", "gate_max_points": "margi", "gate_num_step": "margi", "gate_last_num": "margi",
         "gate_isexist": "margi"}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_bitwise_variants_are_rejected(alone, variant):
    case = Cs.get_case(WHERE[variant])
    snaps = []
    Cs.run(case, None, ref=R.RefMap(variant=variant, **case["prm"]), snaps=snaps)
    honest = alone[case["name"]][1]
    assert len(snaps) == len(honest) and not all(Cs.same_snapshot(a, b) for a, b in zip(snaps, honest)), variant


def test_serial_fix_copy_variants_are_rejected(alone):
    """The folds above one tile of FIX points (fix_divide) under the two tile variants."""
    for variant in ("drop_remainder_tile", "second_tile_first"):
        case = Cs.get_case("fc129_ml2")
        snaps = []
        Cs.run(case, None, ref=R.RefMap(variant=variant, **case["prm"]), snaps=snaps)
        assert not all(Cs.same_snapshot(a, b) for a, b in zip(snaps, alone["fc129_ml2"][1])), variant


TRIPS = {"tr_cross": "tr", "pv_nc_transposed": "pv_nc", "pv_centre_scale": "pv_cc", "pv_gap_sign": "pv_nc", "radius_double": "radius"}


@pytest.mark.parametrize("variant", R.VALUE_VARIANTS)
def test_arithmetic_variants_are_rejected(variant):
    """The honest oracle against a degraded replay: the run itself passes every bit-for-bit comparison, and the criterion meant for the variant --
    no other -- is the one that is missed."""
    case = Cs.get_case("margi" if variant != "tr_cross" else "pc65_three")
    _, err = Cs.run(case, Cs.OracleSide(case["prm"]), variant=variant)
    assert set(Cs.missed(err, Cs.FACTOR_DEVICE)) == {TRIPS[variant]}, (variant, err.worst)


def old_rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-300))


def test_what_the_old_tolerances_accept(on_oracle):
    """Whole-array `rel(plane_var) < 1e-5`, `radius rtol 1e-6`, `rel(pcr_add) < 1e-9` of tests/test_gpu_map.py on the degraded values, per leaf table."""
    worst = {v: 0.0 for v in R.VALUE_VARIANTS}
    for name, (ref, _, old) in on_oracle.items():
        tables = {}
        for kind, b, k, n, pl in old:
            tables.setdefault((id(b), kind), []).append((b, k, n, pl))
        for (_, kind), rows in tables.items():
            if kind == "pv":
                good = np.array([b["plane_var"][k] for b, k, _, _ in rows])
                for v in ("pv_nc_transposed", "pv_centre_scale", "pv_gap_sign"):
                    bad = np.array([[[float(x) for x in row] for row in R.plane_update_exact(b["pcr_add"][k], b["eig_val"][k], b["eig_vec"][k], b["cov_add"][k], variant=v)[1][0]]
                                    for b, k, _, _ in rows])
                    worst[v] = max(worst[v], old_rel(bad, good) / 1e-5)
                for b, k, _, _ in rows:
                    worst["radius_double"] = max(worst["radius_double"], abs(b["eig_val"][k, 2] - b["radius"][k]) / b["radius"][k] / 1e-6)
            else:
                good = np.array([b["pcr_add"][k] for b, k, _, _ in rows])
                bad = np.array([Cs.exact_margi_sums(ref, n, pl, variant="tr_cross")[0] for _, _, n, pl in rows])
                worst["tr_cross"] = max(worst["tr_cross"], old_rel(bad, good) / 1e-9)
    accepted = sorted(v for v, w in worst.items() if w < 1.0)
    assert accepted == ["radius_double"], worst


# ---- 5. the kernels' own arithmetic, built for the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hm():
    return Cs.hostlib()


@pytest.mark.parametrize("name", Cs.CASE_NAMES)
def test_host_restatement_meets_the_criteria_on_every_case(name):
    """The fix-form cases too (the oracle has none): the reference's structure with the kernels' arithmetic built for the host, held to 2 K."""
    case = Cs.get_case(name)
    _, err = Cs.run(case, Cs.HostSide(case["prm"]))
    Cs.check_errors(err, Cs.FACTOR_CPU, label=name)


def test_sequential_arithmetic_of_the_header_is_the_references_bit_for_bit(hm):
    """csrc/vxba_map_math.hpp through g++ -ffp-contract=off: to_world, voxel_index, octant_of, cl_push and cov_add_point on a scan of 129 points."""
    case = Cs.get_case("pc129_three")
    _, body, var, pose = case["ops"][0]
    n = body.shape[0]
    world = np.zeros((n, 3))
    hm.maph_to_world(n, np.ascontiguousarray(pose), body, world)
    pw = np.array([R.to_world([float(v) for v in pose], [float(v) for v in x]) for x in body])
    assert np.array_equal(world, pw)
    ref = R.RefMap(**case["prm"])
    ref.cut_voxel(0, body, var, pw)
    (root,) = ref.leaf_nodes()
    cl_l, cl_a, cov = np.zeros(10), np.zeros(10), np.zeros(81)
    hm.maph_push(n, body, world, np.ascontiguousarray(np.transpose(var, (0, 2, 1))).reshape(n, 9), cl_l, cl_a, cov)
    assert np.array_equal(cl_l, root.pcrs_local[0]) and np.array_equal(cl_a, root.pcr_add) and np.array_equal(cov.reshape(9, 9).T, root.cov_add)
    edge = Cs.get_case("edges")["ops"][0][1]
    w = np.ascontiguousarray(np.concatenate([edge.reshape(-1), [3.0, -3.0, -0.0, 0.0, 4.0 - 1e-9, -1e-9, 32767.99999, -32768.0]]))
    for vs in (1.0, 0.5):
        loc = np.zeros(w.size, dtype=np.int64)
        hm.maph_voxel_index(w.size, w, vs, loc)
        assert loc.tolist() == [R.voxel_index(float(x), vs) for x in w]
    oct_ = np.zeros(edge.shape[0], dtype=np.int32)
    ctr = np.array([3.5, -1.5, 0.5])
    hm.maph_octant(edge.shape[0], np.ascontiguousarray(edge), ctr, oct_)
    assert oct_.tolist() == [int(R.octant_of(x, ctr)) for x in edge] and len(set(oct_.tolist())) >= 5


def test_rounded_arithmetic_of_the_header_meets_the_criteria(hm, on_oracle):
    """cl_transform and plane_update's arithmetic of the header on what the oracle exported behind margi, against the 200-bit replay at 2 K."""
    import mpmath as mp
    err = Cs.Errors()
    n_tr = n_pv = 0
    for name, (ref, _, old) in on_oracle.items():
        for kind, b, k, node, poses in old:
            if kind == "tr":
                for j, l in enumerate(node.margi_path["locals"]):
                    if l[9] == 0:
                        continue
                    out = np.zeros(10)
                    hm.maph_transform(np.array(l), np.array(poses[j]), out)
                    val, mag = R.transform_exact(l, poses[j])
                    with mp.workprec(R.PREC):
                        for e in range(9):
                            if mag[e] > 0:
                                err.add("tr", abs(mp.mpf(float(out[e])) - val[e]) / (Cs.U * mag[e]), (name, k, j, e))
                    assert out[9] == l[9]
                    n_tr += 1
            else:
                cen, pv = np.zeros(3), np.zeros(36)
                hm.maph_plane_update(np.ascontiguousarray(b["cov_add"][k].T).reshape(81), np.ascontiguousarray(b["pcr_add"][k]), np.ascontiguousarray(b["eig_vec"][k]),
                                     np.ascontiguousarray(b["eig_val"][k]), cen, pv)
                rec = dict(pcr_add=b["pcr_add"][k][None], eig_val=b["eig_val"][k][None], eig_vec=b["eig_vec"][k][None], cov_add=b["cov_add"][k][None], center=cen[None],
                           normal=b["eig_vec"][k][None, 0:3], radius=np.array([float(np.float32(b["eig_val"][k, 2]))]), plane_var=pv.reshape(6, 6).T[None])
                Cs.check_plane_record(err, rec, 0, (name, k))
                n_pv += 1
    assert n_tr > 50 and n_pv > 20
    Cs.check_errors(err, Cs.FACTOR_CPU, label="vxba_map_math.hpp on the host")
