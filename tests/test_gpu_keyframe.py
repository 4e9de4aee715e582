"""vxba_keyframe_* on the device against the numpy checker (tests/_keyframe_ref.py) and the reference's own filter (tests/golden/keyframe/keyframe.npz),
bit for bit; the two device-pointer consumers against their host routes.  tests/test_keyframe_cpu.py asserts that the inputs of
tests/_keyframe_cases.py contain what they claim."""
import os

import numpy as np
import pytest

from tests import _keyframe_cases as KC
from tests import _keyframe_ref as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_keyframe(builder, ref_kf):
    info = builder.info()
    full, down = builder.read()
    assert info["id"] == ref_kf["id"] and info["jour"] == ref_kf["jour"] and np.array_equal(info["pose"], ref_kf["pose"])
    assert info["n_full"] == ref_kf["full"].shape[0] and info["n_down"] == ref_kf["down"].shape[0]
    assert np.array_equal(bits(full), bits(ref_kf["full"]))
    assert np.array_equal(bits(down), bits(ref_kf["down"]))
    return full, down


def run_both(case, var=True):
    from voxel_slam_amd import vxba
    b = vxba.KeyframeBuilder(case["win"], case["voxel_size"])
    r = K.KeyframeRef(case["win"], case["voxel_size"])
    for pose, v6, pts, v in case["scans"]:
        assert b.push_scan(pose, v6, pts, v if var else None) == r.push_scan(pose, v6, pts, v if var else None)
    return b, r


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "keyframe", "keyframe.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_case(g):
    sp = g["scan_ptr"]
    return dict(name="golden", win=g["poses"].shape[0], voxel_size=float(g["voxel_size"]),
                scans=[(g["poses"][k], g["v6"][k], g["pnt"][sp[k]:sp[k + 1]], g["var"][sp[k]:sp[k + 1]]) for k in range(g["poses"].shape[0])])


def test_golden_keyframe(golden):
    b, r = run_both(golden_case(golden))
    full, down = same_keyframe(b, r.keyframe)
    assert full.shape == golden["full"].shape and np.array_equal(bits(full), bits(golden["full"]))
    assert down.shape == golden["down"].shape and np.array_equal(bits(down), bits(golden["down"]))
    b.close()


@pytest.mark.parametrize("case", KC.all_cases(), ids=lambda c: c["name"])
def test_shapes(case):
    b, r = run_both(case)
    same_keyframe(b, r.keyframe)
    assert b.num_buffered() == 0 and b.num_scans() == case["win"]
    b.close()


@pytest.mark.parametrize("name,bad", KC.bad_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_bad_input_is_refused_and_undone(name, bad):
    from voxel_slam_amd import vxba
    b = vxba.KeyframeBuilder(3, KC.VOXEL_SIZE)
    r = K.KeyframeRef(3, KC.VOXEL_SIZE)
    for k in range(5):
        pts = KC.lattice(4, 10 * k)
        assert b.push_scan(KC.IDENT, KC.V6, pts) == r.push_scan(KC.IDENT, KC.V6, pts)
    before = b.read()
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        b.push_scan(KC.MOVED, KC.V6, bad)
    same_keyframe(b, r.keyframe)                                     # the previous keyframe, untouched
    after = b.read()
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
    assert b.num_scans() == 5 and b.num_buffered() == 2
    good = KC.lattice(4, 60)
    assert b.push_scan(KC.MOVED, KC.V6, good) and r.push_scan(KC.MOVED, KC.V6, good)      # as if the bad push never happened
    same_keyframe(b, r.keyframe)
    assert b.info()["id"] == 5 and np.array_equal(b.scan_poses()[0], r.scan_poses()[0])
    b.close()


def test_device_route_refuses_a_nan_at_the_push_that_brings_it():
    import torch
    from voxel_slam_amd import vxba
    b = vxba.KeyframeBuilder(3, KC.VOXEL_SIZE)
    bad = KC.lattice(5); bad[2, 1] = np.nan
    t = torch.from_numpy(bad).cuda()
    with pytest.raises(vxba.VxbaError, match="VXBA_ERR_ARG"):
        b.push_scan_device(KC.IDENT, KC.V6, 5, t.data_ptr())          # a buffering push: nothing is assembled yet
    assert b.num_scans() == 0 and b.num_buffered() == 0 and b.info() is None
    b.close()


def test_null_variances_are_zeros(golden):
    case = golden_case(golden)
    zero = dict(case, scans=[(p, v6, pts, np.zeros((pts.shape[0], 9))) for p, v6, pts, _ in case["scans"]])
    a, _ = run_both(case, var=False)
    z, r = run_both(zero)
    fa, da = a.read(); fz, dz = z.read()
    assert np.array_equal(bits(fa), bits(fz)) and np.array_equal(bits(da), bits(dz)) and not da[:, 3:].any()
    same_keyframe(a, r.keyframe)
    a.close(); z.close()


def test_host_and_device_routes_and_two_runs_give_identical_bytes(golden):
    import torch
    from voxel_slam_amd import vxba
    for case in (golden_case(golden), KC.ragged(), KC.edges()):
        h1, r = run_both(case)
        h2, _ = run_both(case)                                       # repeatability
        d = vxba.KeyframeBuilder(case["win"], case["voxel_size"])
        keep = []
        for pose, v6, pts, var in case["scans"]:
            tp, tv = torch.from_numpy(np.ascontiguousarray(pts)).cuda(), torch.from_numpy(np.ascontiguousarray(var)).cuda()
            keep.append((tp, tv))
            em = d.push_scan_device(pose, v6, pts.shape[0], tp.data_ptr() if pts.shape[0] else 0, tv.data_ptr() if pts.shape[0] else 0)
        assert em
        a, b2, c = h1.read(), h2.read(), d.read()
        for x, y in ((a, b2), (a, c)):
            assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1])), case["name"]
        same_keyframe(d, r.keyframe)
        assert d.info()["jour"] == h1.info()["jour"]
        for h in (h1, h2, d):
            h.close()


def test_rule_stream_scan_poses_and_clear():
    from voxel_slam_amd import vxba
    b = vxba.KeyframeBuilder(3)
    r = K.KeyframeRef(3)
    stream = KC.rule_stream()
    assert b.info() is None
    for k, s in enumerate(stream):
        em = b.push_scan(*s)
        assert em == r.push_scan(*s) == bool(KC.RULE_EMITTED[k]), k
        assert b.num_buffered() == len(r.ring) == KC.RULE_BUFFERED[k], k
        if em:
            same_keyframe(b, r.keyframe)
            i = b.info()
            assert i["id"] == KC.RULE_IDS[k] and i["jour"] == KC.RULE_JOUR[k] and np.array_equal(i["pose"], s[0])
    P, V = b.scan_poses()
    rP, rV = r.scan_poses()
    assert b.num_scans() == 14 and np.array_equal(P, rP) and np.array_equal(V, rV)
    P2, V2 = b.scan_poses(5, 3)
    assert np.array_equal(P2, rP[5:8]) and np.array_equal(V2, rV[5:8])
    b.clear(); r.clear()
    assert b.info() is None and b.num_scans() == 0 and b.num_buffered() == 0
    for k in range(7):                                               # a stationary session: the first window emits (id 2, jour 0), the next one is dropped scan by scan
        em = b.push_scan(stream[3][0], stream[3][1], stream[k][2])
        assert em == r.push_scan(stream[3][0], stream[3][1], stream[k][2]) == (k == 2)
        assert b.num_buffered() == len(r.ring)
    same_keyframe(b, r.keyframe)
    assert b.info()["id"] == 2 and b.info()["jour"] == 0.0 and b.num_buffered() == 2
    b.close()


def test_add_keyframe_device_gives_the_host_route_plane_cloud(golden):
    from voxel_slam_amd import synth, vxba
    lp = synth.loop_pair(pts_per_scan=20000)
    cloud = np.ascontiguousarray(lp.cloud_cur)
    b = vxba.KeyframeBuilder(3, 1.0)
    third = cloud.shape[0] // 3
    for k in range(3):
        em = b.push_scan(KC.IDENT, KC.V6, cloud[k * third:(k + 1) * third])
    assert em
    full, _ = b.read()
    with vxba.LoopRegistration() as reg:
        host = reg.add_keyframe(full.astype(np.float64))
        dev = reg.add_keyframe_device(full.shape[0], b.device_ptrs()["full"])
        empty = reg.add_keyframe_device(0, 0)
        a, d = reg.read_cloud(host), reg.read_cloud(dev)
        assert a.shape[0] > 20 and a.shape == d.shape and np.array_equal(bits(a), bits(d)) and reg.cloud_size(empty) == 0
    b.close()


def same_tree(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_add_keyframes_device_and_one_pass_equal_the_host_added_session():
    import torch
    from voxel_slam_amd import synth, vxba
    xyz, fp, poses, _ = synth.make_scans(win_size=4, pts_per_scan=2000, extent=8.0, noise=0.005, seed=synth.MASTER_SEED + 8200, rot_sigma_deg=0.1, trans_sigma=0.02)
    clouds = [xyz[fp[i]:fp[i + 1]].astype(np.float32) for i in range(4)]
    coarse = vxba.VoxelizeParams(voxel_size=2.0, max_layer=2, min_points=10, min_eigen_value=0.02, eigen_ratio=(1 / 9, 1 / 9, 1 / 9, 1 / 9))
    fine = vxba.VoxelizeParams(voxel_size=1.0, max_layer=2, min_points=10, min_eigen_value=0.01, eigen_ratio=(1 / 16, 1 / 16, 1 / 9, 1 / 9))
    host, dev = vxba.HbaSession(), vxba.HbaSession()
    host.add_keyframes(clouds)
    t01 = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds[:2]))).cuda()
    t23 = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds[2:]))).cuda()
    dev.add_keyframes_device([c.shape[0] for c in clouds[:2]], t01.data_ptr())
    dev.add_keyframes_device([c.shape[0] for c in clouds[2:]], t23.data_ptr())
    assert dev.num_keyframes() == host.num_keyframes() == 4
    a = host.run_pass(poses, coarse, fine, wdsize=2, mgsize=2, top_max_iter=1, n_threads=1)
    d = dev.run_pass(poses, coarse, fine, wdsize=2, mgsize=2, top_max_iter=1, n_threads=1)
    assert len(a["edges1"]) > 0 and same_tree(a, d)
    host.close(); dev.close()


def test_launches_and_waits_do_not_depend_on_the_size():
    from voxel_slam_amd import vxba
    stats = {}
    rng = np.random.default_rng(11)
    for n in (200, 5000):
        b = vxba.KeyframeBuilder(3, 1.0)
        for rep in range(2):                                         # the second keyframe reuses every buffer
            for k in range(3):
                pose = KC.IDENT.copy(); pose[9] = rep * 1.0 + 0.01 * k
                em = b.push_scan(pose, KC.V6, rng.uniform(-3, 3, size=(n, 3)))
                if k < 2:
                    buffering = b.stats()
            assert em
        stats[n] = (b.stats(), buffering)
        b.close()
    (e200, b200), (e5k, b5k) = stats[200], stats[5000]
    assert (e200["launches"], e200["host_waits"]) == (e5k["launches"], e5k["host_waits"]) == (5, 1)
    assert (b200["launches"], b200["host_waits"]) == (b5k["launches"], b5k["host_waits"]) == (0, 1)
    assert e5k["bytes_d2h"] == e200["bytes_d2h"] and e5k["bytes_h2d"] > e200["bytes_h2d"]      # no cloud comes back; the scan goes up


def test_keyframe_stream_feeds_both_consumers():
    from voxel_slam_amd import hba, synth, vxba
    st = synth.make_scanpose_stream(12, 400, 3)
    r = K.KeyframeRef(3, 1.0)
    ref = []
    for s in st:
        if r.push_scan(*s):
            ref.append(r.keyframe)
    b = vxba.KeyframeBuilder(3, 1.0)
    ses = vxba.HbaSession()
    with vxba.LoopRegistration() as reg:
        got = hba.keyframe_stream(b, reg, ses, st)
        assert [g[0] for g in got] == [k["id"] for k in ref] and len(ref) >= 3
        assert all(np.array_equal(g[1], k["pose"]) and g[2] == k["jour"] for g, k in zip(got, ref))
        assert reg.num_clouds() == ses.num_keyframes() == len(ref)
        with vxba.LoopRegistration() as reg2:                        # the plane clouds of the checker's full clouds through the host route
            for k, kf in enumerate(ref):
                cid = reg2.add_keyframe(kf["full"].astype(np.float64))
                assert reg.cloud_size(k) == reg2.cloud_size(cid) and np.array_equal(bits(reg.read_cloud(k)), bits(reg2.read_cloud(cid)))
            assert sum(reg2.cloud_size(k) for k in range(len(ref))) > 0
    same_keyframe(b, ref[-1])
    b.clear()                                                        # the same stream by hand: the cloud counts of every keyframe the helper handed on
    counts = []
    for s in st:
        if b.push_scan(*s):
            counts.append((b.info()["n_full"], b.info()["n_down"]))
    assert counts == [(k["full"].shape[0], k["down"].shape[0]) for k in ref]
    ses.close(); b.close()
