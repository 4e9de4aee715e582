"""Numpy model of the loop search (include/vxba.h: vxba_loopsearch_*): the CHECKER of tests/test_gpu_loopsearch.py and of
tests/test_loopsearch_cpu.py, never the thing run.

Written against the text of the reference -- STDescManager::generate_std (BTC.cpp:979-1126), AddSTDescs (:258-277), candidate_selector
(:1128-1279), candidate_verify / triangle_solver (:1281-1420), SearchLoop (:205-256), binary_similarity (:70-80) -- with every quantity a
decision rests on formed by the same sequence of roundings as csrc/vxba_loopsearch_math.hpp forms it: float32 where the reference holds a
pcl::PointXYZ, float64 elsewhere, sums in the written order.  BTC.cpp cannot be compiled in the test environment (visualization_msgs,
<execution>, Eigen::EigenSolver, JacobiSVD), so the device code is pinned to this model and this model to mathematics
(tests/test_loopsearch_cpu.py): rigid-motion invariance of the descriptors, recovery of an applied rotation, the ordering rules on hand-built
arrays.  The rotation is ``numpy.linalg.svd``'s; the verify score is ``tests/_loopreg_ref.score``.

Three places where the reference's text, not a paraphrase of it, is followed: the difference of two corner coordinates is taken in float32 before
it is squared in float64 (p1.x - p2.x of two pcl::PointXYZ); triangle = side * (1 / std_side_resolution), a product; and SearchLoop's best score
starts at 0, so a candidate needs a score above max(icp_threshold, 0).

``perturb``: every real-valued argument of a truncation or a threshold test is multiplied by (1 + perturb) first -- the honesty tests run the
inputs of the GPU tests with +-1e-9 and require that no integer and no verdict changes, which is what makes the GPU tests' equalities fair.
"""
import dataclasses

import numpy as np

from tests import _loopreg_ref as LR


@dataclasses.dataclass
class Params:                      # BTC.cpp:22-34
    descriptor_near_num: int = 15
    descriptor_min_len: float = 2.0
    descriptor_max_len: float = 50.0
    std_side_resolution: float = 0.2
    skip_near_num: int = 30
    candidate_num: int = 20
    rough_dis_threshold: float = 0.01
    similarity_threshold: float = 0.7
    icp_threshold: float = 0.15
    normal_threshold: float = 0.2
    dis_threshold: float = 0.5


VERIFY_DIS = 3.0
KEY_BITS = 21


def popcount(a):
    a = np.asarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


def norm3(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def pack3(c):
    c = np.asarray(c, dtype=np.int64)
    return (c[..., 0] << (2 * KEY_BITS)) | (c[..., 1] << KEY_BITS) | c[..., 2]


# ---- 1. generate_std ---------------------------------------------------------------------------------------------------------------
def knn(xs, K):
    """xs (n, 3) float32.  (indices (n, K) of the K nearest, itself included, by float32 (dx dx + dy dy) + dz dz, ties to the lowest index;
    number of corners whose K + 1 smallest distances hold two equal ones)."""
    xs = np.asarray(xs, dtype=np.float32)
    d = xs[None, :, :] - xs[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32
    order = np.argsort(d2, axis=1, kind="stable")
    srt = np.take_along_axis(d2, order, axis=1)[:, :K + 1]
    ties = int((srt[:, 1:] == srt[:, :-1]).any(axis=1).sum())
    return order[:, :K], ties


def side(p, q):
    d = (p - q).astype(np.float32).astype(np.float64)       # the difference of two floats is a float; its square is exact in float64
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def sort_sides(a, b, c):
    """The three conditional swaps (BTC.cpp:1032-1055) with the vertex sets of the sides as bit masks (1: the corner, 2: neighbour m, 4: neighbour n).
    Returns a <= b <= c and v (..., 3): which of (corner, m, n) is A, B, C."""
    ma, mb, mc = np.full(a.shape, 3), np.full(a.shape, 5), np.full(a.shape, 6)

    def swap(s, x, y, mx, my):
        return np.where(s, y, x), np.where(s, x, y), np.where(s, my, mx), np.where(s, mx, my)
    a, b, ma, mb = swap(a > b, a, b, ma, mb)
    b, c, mb, mc = swap(b > c, b, c, mb, mc)
    a, b, ma, mb = swap(a > b, a, b, ma, mb)
    v = np.stack([ma & mb, ma & mc, mb & mc], axis=-1) >> 1
    return a, b, c, v


def describe(locations, occupancy, prm=None, perturb=0.0):
    """dict(triangle (nd, 3), centre (nd, 3), corners (nd, 3) int32, loc (nd, 3, 3) float64 locations of A, B, C, occ (nd, 3) uint64, key (nd, 3)
    int64, cell (nd, 3) int64: the AddSTDescs cell, knn_ties)."""
    prm = prm or Params()
    loc = np.asarray(locations, dtype=np.float64).reshape(-1, 3)
    occ = np.asarray(occupancy, dtype=np.uint64).reshape(-1)
    n = loc.shape[0]
    K = min(prm.descriptor_near_num, n)
    e = 1.0 + perturb
    empty = dict(triangle=np.zeros((0, 3)), centre=np.zeros((0, 3)), corners=np.zeros((0, 3), np.int32), loc=np.zeros((0, 3, 3)), occ=np.zeros((0, 3), np.uint64),
                 key=np.zeros((0, 3), np.int64), cell=np.zeros((0, 3), np.int64), knn_ties=0)
    if K < 3:
        return empty
    xs = loc.astype(np.float32)
    nb, ties = knn(xs, K)
    mn = np.array([(m, k) for m in range(1, K - 1) for k in range(m + 1, K)])          # loop order
    i1 = np.repeat(np.arange(n)[:, None], mn.shape[0], axis=1)
    i2, i3 = nb[:, mn[:, 0]], nb[:, mn[:, 1]]
    p1, p2, p3 = xs[i1], xs[i2], xs[i3]
    a, b, c = side(p1, p2), side(p1, p3), side(p3, p2)
    lo, hi = prm.descriptor_min_len, prm.descriptor_max_len
    ok = ~((a * e > hi) | (b * e > hi) | (c * e > hi) | (a * e < lo) | (b * e < lo) | (c * e < lo))
    a, b, c, v = sort_sides(a, b, c)
    ok &= ~(np.abs(c - (a + b)) * e < 0.2)
    key = np.stack([((s * 1000.0) * e).astype(np.float32).astype(np.int64) for s in (a, b, c)], axis=-1)
    idx3 = np.stack([i1, i2, i3], axis=-1)
    corners = np.take_along_axis(idx3, v, axis=-1)
    flat_ok = ok.reshape(-1)
    where = np.nonzero(flat_ok)[0]
    if where.size == 0:
        return dict(empty, knn_ties=ties)
    packed = pack3(key.reshape(-1, 3)[where])
    _, first = np.unique(packed, return_index=True)                                   # the first occurrence of every key, in loop order
    keep = where[np.sort(first)]
    corners = corners.reshape(-1, 3)[keep]
    sides3 = np.stack([a, b, c], axis=-1).reshape(-1, 3)[keep]
    scale = 1.0 / prm.std_side_resolution
    tri = scale * sides3
    f = xs[corners].astype(np.float64)                                                # (nd, 3 vertices, 3)
    centre = ((f[:, 0] + f[:, 1]) + f[:, 2]) / 3.0
    cell = ((tri + 0.5) * e).astype(np.int64)
    return dict(triangle=tri, centre=centre, corners=corners.astype(np.int32), loc=loc[corners], occ=occ[corners], key=key.reshape(-1, 3)[keep], cell=cell, knn_ties=ties)


# ---- 2-5. the database and the search --------------------------------------------------------------------------------------------------
def similarity(p, q):
    """(n, 3) uint64 each: the mean over A, B, C of 2 |p & q| / (|p| + |q|), summed (A + B) + C.  0 / 0 is NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        s = 2.0 * popcount(p & q).astype(np.float64) / (popcount(p) + popcount(q)).astype(np.float64)
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) / 3.0


def kabsch(sl, sc, rl, rc):
    """triangle_solver: sl, rl (h, 3 vertices, 3) locations, sc, rc (h, 3) centres.  Returns poses (h, 12) [R column-major | t]."""
    src = (sl - sc[:, None, :]).transpose(0, 2, 1)           # columns = vertices
    ref = (rl - rc[:, None, :]).transpose(0, 2, 1)
    cov = src @ ref.transpose(0, 2, 1)
    U, _, Vh = np.linalg.svd(cov)
    V = Vh.transpose(0, 2, 1)
    rot = V @ U.transpose(0, 2, 1)
    neg = np.linalg.det(rot) < 0
    Kf = np.diag([1.0, 1.0, -1.0])
    rot[neg] = V[neg] @ Kf @ U[neg].transpose(0, 2, 1)
    t = rc - np.einsum("hab,hb->ha", rot, sc)
    return np.concatenate([rot.transpose(0, 2, 1).reshape(-1, 9), t], axis=1)


def select_candidates(votes, candidate_num):
    """The repeated first max_element of candidate_selector: frames by (votes descending, frame ascending) while votes >= 5."""
    v = np.array(votes, dtype=np.int64)
    out = []
    for _ in range(candidate_num):
        if v.size == 0:
            break
        f = int(np.argmax(v))
        if v[f] < 5:
            break
        out.append((f, int(v[f])))
        v[f] = 0
    return out


def first_max(votes):
    """candidate_verify's running maximum (max_vote < vote, from 0): the first of the maxima; index 0 when every vote is 0."""
    v = np.asarray(votes)
    return (int(np.argmax(v)), int(v.max())) if v.size else (0, 0)


class Database:
    """The descriptors of the frames added so far and the plane cloud each frame is bound to."""

    def __init__(self):
        self.tri = np.zeros((0, 3)); self.ctr = np.zeros((0, 3)); self.loc = np.zeros((0, 3, 3)); self.occ = np.zeros((0, 3), np.uint64)
        self.frame = np.zeros(0, np.int64); self.index = np.zeros(0, np.int64); self.cellkey = np.zeros(0, np.int64)
        self.clouds = []

    @property
    def num_frames(self):
        return len(self.clouds)

    def add(self, d, cloud_rows):
        f = self.num_frames
        n = d["triangle"].shape[0]
        self.tri = np.concatenate([self.tri, d["triangle"]]); self.ctr = np.concatenate([self.ctr, d["centre"]]); self.loc = np.concatenate([self.loc, d["loc"]])
        self.occ = np.concatenate([self.occ, d["occ"]]); self.frame = np.concatenate([self.frame, np.full(n, f)]); self.index = np.concatenate([self.index, np.arange(n)])
        self.cellkey = np.concatenate([self.cellkey, pack3(d["cell"])])
        self.clouds.append(np.asarray(cloud_rows, dtype=np.float32).reshape(-1, 6))

    def matches(self, d, prm, perturb=0.0):
        """candidate_selector's match list, ordered by (query index, offset index, position in the cell): rows (query, frame, index within frame), the
        global entry index of each, and the number of (query, offset) cells visited."""
        e = 1.0 + perturb
        tri = d["triangle"]
        nd = tri.shape[0]
        inc = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], dtype=np.float64)
        cell = ((tri[:, None, :] + inc[None, :, :]) * e).astype(np.int64)                      # (nd, 27, 3)
        dist = norm3(tri[:, None, :] - (cell.astype(np.float64) + 0.5))
        visit = dist * e < 1.5
        order = np.argsort(self.cellkey, kind="stable")                                        # insertion order inside a cell
        skey = self.cellkey[order]
        qk = pack3(cell).reshape(-1)
        lo = np.searchsorted(skey, qk, side="left"); hi = np.searchsorted(skey, qk, side="right")
        cnt = np.where(visit.reshape(-1), hi - lo, 0)
        t = np.repeat(np.arange(nd * 27), cnt)                                                 # (query, offset) of every pair tested
        within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        g = order[lo[t] + within]
        q = t // 27
        ok = (self.num_frames - self.frame[g]) > prm.skip_near_num
        dis = norm3(tri[q] - self.tri[g])
        thr = norm3(tri[q]) * prm.rough_dis_threshold
        ok &= dis * e < thr
        sim = similarity(d["occ"][q], self.occ[g])
        ok &= sim * e > prm.similarity_threshold
        q, g = q[ok], g[ok]
        return np.stack([q, self.frame[g], self.index[g]], axis=1).astype(np.int32).reshape(-1, 3), g, int(visit.sum())

    def verify(self, d, q, g, cur_rows, frame, prm):
        """candidate_verify for the pairs (q, g) of one candidate, in list order.  Returns the candidate's dict; ``margin``: the smallest distance of any
        |R x + t - y| from 3.0 over hypotheses, pairs and corners, and of any gate quantity of the score from its threshold."""
        M = q.shape[0]
        skip_len = M // 50 + 1
        use = M // skip_len
        hp = np.arange(use) * skip_len
        poses = kabsch(d["loc"][q[hp]], d["centre"][q[hp]], self.loc[g[hp]], self.ctr[g[hp]])
        R = poses[:, :9].reshape(-1, 3, 3).transpose(0, 2, 1)
        x = np.einsum("hab,mvb->hmva", R, d["loc"][q]) + poses[:, None, None, 9:]
        dist = norm3(x - self.loc[g][None])                                                       # (use, M, 3)
        fin = np.isfinite(poses).all(axis=1)
        with np.errstate(invalid="ignore"):
            votes = ((dist < VERIFY_DIS).all(axis=2) & fin[:, None]).sum(axis=1)
        margin = float(np.abs(dist[fin] - VERIFY_DIS).min()) if fin.any() else np.inf
        best, max_vote = first_max(votes)
        out = dict(frame=int(frame), votes=M, pairs=M, hypotheses=use, best=best, max_vote=max_vote, useful=0, score=-1.0, pose=poses[best], hyp_votes=votes, hyp_pairs=hp,
                   margin=margin, ties=0)
        if max_vote >= 4:
            s = LR.score(cur_rows, self.clouds[frame], poses[best], prm.normal_threshold, prm.dis_threshold)
            out.update(useful=s["useful"], score=s["score"], margin=min(margin, s["margin"]), ties=s["ties"])
        return out

    def search(self, d, cur_rows, prm=None, perturb=0.0):
        """SearchLoop.  dict(frame, score, pose, candidates, matches (n, 3), visited)."""
        prm = prm or Params()
        cur_rows = np.asarray(cur_rows, dtype=np.float32).reshape(-1, 6)
        res = dict(frame=-1, score=0.0, pose=np.zeros(12), candidates=[], matches=np.zeros((0, 3), np.int32), visited=0)
        if d["triangle"].shape[0] == 0 or self.num_frames == 0:
            return res
        rows, g, visited = self.matches(d, prm, perturb)
        res.update(matches=rows, visited=visited)
        votes = np.bincount(rows[:, 1], minlength=self.num_frames)
        best, chosen = 0.0, None                                                               # SearchLoop: best_score starts at 0, strictly greater wins
        for f, _ in select_candidates(votes, prm.candidate_num):
            sel = rows[:, 1] == f
            c = self.verify(d, rows[sel, 0], g[sel], cur_rows, f, prm)
            res["candidates"].append(c)
            if c["score"] > best:
                best, chosen = c["score"], c
        if chosen is not None and best > prm.icp_threshold:
            res.update(frame=chosen["frame"], score=chosen["score"], pose=chosen["pose"].copy())
        return res
