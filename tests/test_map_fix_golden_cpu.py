"""tests/golden/map_fix/*.npz without a GPU: the fixture is consistent with the inputs the GPU test regenerates (keyframe sums recomputed
sequentially in numpy, bit for bit), holds the events the scenario was chosen for, and -- where the reference is present -- is what the committed recipe
(make_golden_map_fix.py + ref_fixmap.cpp) produces from the reference's own code today."""
import importlib.util
import os
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def G():
    spec = importlib.util.spec_from_file_location("tests._make_golden_map_fix", os.path.join(HERE, "golden", "map_fix", "make_golden_map_fix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_small_and_outside_the_ba_case_glob(G):
    import glob
    assert all(os.path.dirname(p) != os.path.join(HERE, "golden") for p in G.FIXTURES)
    assert not set(G.FIXTURES) & set(glob.glob(os.path.join(HERE, "golden", "*.npz")))
    sizes = [os.path.getsize(p) for p in G.FIXTURES]
    assert max(sizes) <= 1 << 20 and sum(sizes) <= os.path.getsize(os.path.join(HERE, "golden", "localmap_cycle.npz")), sizes
    g = G.load_fixture()
    assert all(v.dtype.kind in "fiuU" for v in g.values())          # arrays and a backend string only
    assert str(g["backend"]).startswith("reference")


def test_keyframe_sums_of_step_1_are_sequential_sums_of_the_regenerated_points(G):
    """Step 1 loads four clouds into an empty map: every root is one leaf, and its pcr_fix is PointCluster::push over the points of its voxel in input
    order (float-typed voxel index, voxel_map.hpp:1645-1652).  pcr_add is pushed the same points; nothing else has touched the map."""
    from tests.test_oracle_octree import to_world
    g, inp = G.load_fixture(), G.inputs()
    assert np.array_equal(inp["poses_in"], g["poses_in"]) and np.array_equal(inp["dR"], g["dR"]) and np.array_equal(inp["dp"], g["dp"])
    xyz, fp = inp["xyz"], inp["fp"]
    pts = np.concatenate([to_world(inp["poses_gt"][k], xyz[fp[k]:fp[k + 1]])[::2] for k in range(4)])
    loc = (pts / inp["kw"]["voxel_size"]).astype(np.float32)
    loc = np.where(loc < 0, loc - np.float32(1), loc).astype(np.int64)
    ids = ((loc[:, 0] + 32768).astype(np.uint64) << np.uint64(48)) | ((loc[:, 1] + 32768).astype(np.uint64) << np.uint64(32)) | ((loc[:, 2] + 32768).astype(np.uint64) << np.uint64(16))
    assert np.array_equal(np.unique(ids), g["fix0_node_id"]) and g["fix0_node_id"].size == 329
    sums = {}
    for i, (x, y, z) in zip(ids.tolist(), pts.tolist()):
        c = sums.setdefault(i, [0.0] * 10)
        c[9] += 1.0
        c[0] += x * x; c[1] += x * y; c[2] += x * z; c[3] += y * y; c[4] += y * z; c[5] += z * z
        c[6] += x; c[7] += y; c[8] += z
    want = np.array([sums[i] for i in g["fix0_node_id"].tolist()])
    assert np.array_equal(g["fix0_pcr_fix"], want) and np.array_equal(g["fix0_pcr_add"], g["fix0_pcr_fix"])
    assert int(g["fix0_n_point_fix"].sum()) == 6000 == pts.shape[0] and int((g["fix0_pcr_fix"][:, 9] >= G.MAX_POINTS).sum()) == 16
    assert not g["fix0_has_sw"].any() and not g["fix0_in_slide"].any() and not g["fix0_isexist"].any() and not g["fix0_layer"].any()


def test_fixture_holds_the_events_the_scenario_was_chosen_for(G):
    g = G.load_fixture()
    both = lambda t: int(((g[f"{t}_pcr_fix"][:, 9] > 0) & g[f"{t}_has_sw"].astype(bool)).sum())
    kids = lambda t: int(((g[f"{t}_layer"] > 0) & (g[f"{t}_pcr_fix"][:, 9] > 0)).sum())
    assert both("w5") > 500 and both("w8") > both("w5") and kids("w5") > 400 and kids("w8") > kids("w5")      # leaves with loaded points AND a window; children that got loaded points by fix_divide
    assert g["w5_factor_ids"].size > 50 and g["w8_factor_ids"].size > g["w5_factor_ids"].size
    assert (g["w5_node_id"].size, g["kf5_node_id"].size) == (953, 960)                       # allocate_fix created children
    assert np.isin(g["w5_node_id"], g["kf5_node_id"]).all() and g["kf5_n_point_fix"].sum() > g["w5_n_point_fix"].sum()
    assert g["loop_node_id"].size == 846 and int(g["loop_is_plane"].sum()) == 184 and kids("loop") == 495
    assert np.unique(g["loop_node_id"] >> np.uint64(16)).size == 349
    kid_sw = (g["loop_layer"] > 0)[g["loop_has_sw"].astype(bool)]
    assert int((kid_sw & (np.abs(g["loop_cov_add_triu"]).sum(axis=1) > 0)).sum()) > 400    # the stored variances reached children through fix_divide
    assert g["loop_poses"].shape == (2, 12) and g["kf_poses"].shape == (5, 12)


def test_committed_fixture_is_what_the_recipe_generates_from_the_reference(G):
    if not os.path.exists(os.path.join(G.REF_SRC, "voxel_map.hpp")):
        pytest.skip("the reference is not on this machine")
    g = G.load_fixture()
    with tempfile.TemporaryDirectory() as td:
        mod, raw, backend = G.load_reference(G.compile_harness(td))
        d = G.build(mod, raw, backend)
    assert backend == str(g["backend"])
    keys = [k for k in d if k != "backend"]
    assert sorted(keys) == sorted(k for k in g if k != "backend")
    for k in keys:
        assert np.array_equal(d[k], g[k]), k
