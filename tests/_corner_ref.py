"""Numpy checker of the corner extraction (include/vxba.h: vxba_corner_*), written against the reference's text: STDescManager::GenerateSTDescs
without generate_std (VoxelSLAM/src/BTC.cpp).  The BTC.cpp lines stand next to each step.  Float64 throughout, every inner product
(a0 b0 + a1 b1) + a2 b2; per-voxel and per-cell sums run in input order (np.add.at adds element by element, in index order).

Where the reference leaves a choice open the checker takes the one include/vxba.h fixes: plane rows ascend by voxel coordinate, the normal's component
of largest magnitude (the first of equals) is positive, sorts are stable, a height bin that reaches cut_num sets no bit.

``extract`` also returns the MARGIN of every decision it takes (``margins``: name -> smallest distance from a threshold, relative to the threshold's
scale), so that a test can show that a last-bit difference in the device arithmetic cannot flip a decision of its input."""
import dataclasses

import numpy as np

REC = 16
SEG = 5


@dataclasses.dataclass
class Params:      # read_parameters, BTC.cpp:7-20, 25 (normal) | :39-52, 57 (high-fly)
    useful_corner_num: int = 100
    plane_merge_normal_thre: float = 0.1
    plane_merge_dis_thre: float = 0.3
    plane_detection_thre: float = 0.01
    voxel_size: float = 1.0
    voxel_init_num: int = 10
    proj_plane_num: int = 2
    proj_image_resolution: float = 0.5
    proj_image_high_inc: float = 0.1
    proj_dis_min: float = 0.0
    proj_dis_max: float = 5.0
    summary_min_thre: float = 10.0
    line_filter_enable: int = 1
    touch_filter_enable: int = 0
    non_max_suppression_radius: float = 2.0


def high_fly():
    return Params(200, 0.3, 0.6, 0.05, 2.0, 10, 1, 0.5, 0.2, 0.0, 10.0, 6.0, 0, 0, 3.0)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm3(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


class Margins(dict):
    def note(self, name, values):
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        if v.size:
            self[name] = min(self.get(name, np.inf), float(np.min(np.abs(v))))


# ---- 1. plane records ------------------------------------------------------------------------------------------------------------------
def voxel_index(xyz, voxel_size):
    """:287-295: divide, subtract 1.0 where negative, truncate"""
    l = np.asarray(xyz, dtype=np.float64) / voxel_size
    l = np.where(l < 0, l - 1.0, l)
    return np.trunc(l).astype(np.int64)


def sym6_to_mat(c):
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


def solve(rec, mg=None):
    """normal, d, radius, lambda_min of a record from its centre and covariance (:110-129, :429-443), with the header's sign rule"""
    lam, vec = np.linalg.eigh(sym6_to_mat(rec[3:9]))
    n = vec[:, 0].copy()
    a = np.abs(n)
    lead = n[0] if (a[0] >= a[1] and a[0] >= a[2]) else (n[1] if a[1] >= a[2] else n[2])
    if lead < 0:
        n = -n
    rec[10:13] = n
    rec[13] = -((n[0] * rec[0] + n[1] * rec[1]) + n[2] * rec[2])
    rec[14] = np.sqrt(lam[2])
    rec[15] = lam[0]
    if mg is not None:
        s = np.sort(a)
        mg.note("sign_rule", [s[2] - s[1]] if lead != 0 else [])      # which component leads
    return lam


def plane_records(xyz, p, mg):
    """:279-321 init_voxel_map, :96-139 init_plane; rows ascend by voxel coordinate, lexicographic in (x, y, z)"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    vi = voxel_index(xyz, p.voxel_size)
    assert np.all(np.abs(vi) < 2 ** 20)
    uniq, inv, cnt = np.unique(vi, axis=0, return_inverse=True, return_counts=True)      # np.unique sorts rows lexicographically
    inv = inv.reshape(-1)
    V = uniq.shape[0]
    sv = np.zeros((V, 3)); sP = np.zeros((V, 6))
    np.add.at(sv, inv, xyz)                                                              # input order within every voxel
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    np.add.at(sP, inv, np.stack([x * x, x * y, x * z, y * y, y * z, z * z], axis=1))
    rows, vox, gaps = [], [], []
    for v in np.nonzero(cnt > p.voxel_init_num)[0]:                                      # :91
        N = float(cnt[v])
        rec = np.zeros(REC)
        c = sv[v] / N                                                                    # :106
        rec[0:3] = c
        rec[3:9] = sP[v] / N - np.array([c[0] * c[0], c[0] * c[1], c[0] * c[2], c[1] * c[1], c[1] * c[2], c[2] * c[2]])      # :107-109
        rec[9] = N
        lam = solve(rec)
        mg.note("lambda_min", [(lam[0] - p.plane_detection_thre) / p.plane_detection_thre])
        if lam[0] < p.plane_detection_thre:                                              # :119
            solve(rec, mg)
            rows.append(rec); vox.append(uniq[v]); gaps.append(lam[1] - lam[0])
    rows = np.array(rows).reshape(-1, REC)
    return rows, np.array(vox).reshape(-1, 3), np.array(gaps)


# ---- 2. / 3. pair test, labelling, groups ----------------------------------------------------------------------------------------------
def pair_matrix(rows, p, mg):
    """:357-370 for every ordered pair (a = outer, b = inner)"""
    n = rows[:, 10:13]; c = rows[:, 0:3]; d = rows[:, 13]
    nd = norm3(n[:, None, :] - n[None, :, :]); ns = norm3(n[:, None, :] + n[None, :, :])
    dis1 = np.abs(dot3(n[:, None, :], c[None, :, :]) + d[:, None])                       # |n_a . c_b + d_a|
    dis2 = dis1.T
    P = rows.shape[0]
    low = np.tril(np.ones((P, P), dtype=bool), -1)
    mg.note("pair_normal", (np.minimum(np.abs(nd - p.plane_merge_normal_thre), np.abs(ns - p.plane_merge_normal_thre)) / p.plane_merge_normal_thre)[low])
    mg.note("pair_dis", (np.abs(dis1 - p.plane_merge_dis_thre) / p.plane_merge_dis_thre)[low | low.T])
    return ((nd < p.plane_merge_normal_thre) | (ns < p.plane_merge_normal_thre)) & (dis1 < p.plane_merge_dis_thre) & (dis2 < p.plane_merge_dis_thre)


def label_rows(pred):
    """:350-382 / :466-497, the two loops as they stand; returns (ids, rows labelled by the "one zero" rule)"""
    P = pred.shape[0]
    ids = [0] * P
    late = []
    cur = 1
    for i in range(P - 1, 0, -1):
        for j in range(0, i):
            if not pred[i, j]:
                continue
            if ids[i] == 0 and ids[j] == 0:
                ids[i] = cur; ids[j] = cur; cur += 1
            elif ids[i] == 0 and ids[j] != 0:
                ids[i] = ids[j]; late.append(i)
            elif ids[i] != 0 and ids[j] == 0:
                ids[j] = ids[i]; late.append(j)
    return np.array(ids, dtype=np.int32), late


def fold(a, b):
    """:405-424 the update of (cov, c, N) of a by b"""
    I = [0, 0, 0, 1, 1, 2]; J = [0, 1, 2, 1, 2, 2]
    Na, Nb = a[9], b[9]
    Ns = Na + Nb
    m = (a[0:3] * Na + b[0:3] * Nb) / Ns
    cov = np.zeros(6)
    for k in range(6):
        p1 = (a[3 + k] + a[I[k]] * a[J[k]]) * Na
        p2 = (b[3 + k] + b[I[k]] * b[J[k]]) * Nb
        cov[k] = (p1 + p2) / Ns - m[I[k]] * m[J[k]]
    a[3:9] = cov; a[0:3] = m; a[9] = Ns


def fold_groups(rows, ids, keep_unlabelled, mg, gaps=None):
    """:386-456 (get_project_plane: unlabelled rows dropped) / :500-568 (merge_plane: kept at their position); the group is solved once at the end --
    the reference re-solves after every fold, but only covariance, centre and N feed the next fold"""
    out, seen, sizes = [], [], []
    for i in range(rows.shape[0]):
        if ids[i] in seen:
            continue
        if ids[i] == 0:
            if keep_unlabelled:
                out.append(rows[i].copy())
            continue
        r = rows[i].copy()
        merged = 0
        for j in range(rows.shape[0]):
            if j != i and ids[j] == ids[i]:
                merged += 1
                fold(r, rows[j])
        if merged:
            lam = solve(r, mg)
            if gaps is not None:
                gaps.append(lam[1] - lam[0])
            seen.append(ids[i]); out.append(r); sizes.append(merged + 1)
    return np.array(out).reshape(-1, REC), sizes


def sort_by_size(rows):
    """:181 / :183 with ties keeping their order"""
    return rows[np.argsort(-rows[:, 9], kind="stable")]


# ---- 4. the gate -----------------------------------------------------------------------------------------------------------------------
def gate(normals, proj_plane_num, mg):
    """:578-598"""
    used, last = [], np.zeros(3)
    for i, n in enumerate(np.asarray(normals).reshape(-1, 3)):
        a, b = norm3(n - last), norm3(n + last)
        mg.note("gate", [(a - 0.3) / 0.3, (b - 0.3) / 0.3])
        if a < 0.3 or b > 0.3:
            last = n.copy()
            used.append(i)
            if len(used) == proj_plane_num:
                break
    return used


# ---- 5. extract_binary -----------------------------------------------------------------------------------------------------------------
def axes(n):
    """:626-654"""
    A, B, Cc = n
    x = np.array([1.0, 1.0, 0.0])
    if Cc != 0:
        x[2] = -(A + B) / Cc
    elif B != 0:
        x[1] = -A / B
    else:
        x[0] = 0.0; x[1] = 1.0
    x = x / norm3(x)
    y = np.array([n[1] * x[2] - n[2] * x[1], n[2] * x[0] - n[0] * x[2], n[0] * x[1] - n[1] * x[0]])
    y = y / norm3(y)
    return x, y


def line_hit(s, s1, s2):
    """:867-889, one direction"""
    thr = s - 3.0
    hit = False
    if s1 >= thr and s2 >= 0.5 * s:
        hit = True
    if s2 >= thr and s1 >= 0.5 * s:
        hit = True
    if s1 >= thr and s2 >= thr:
        hit = True
    return hit


def extract_binary(xyz, centre, normal, plane, p, mg, exact_plane):
    """:613-924; returns the candidates of one plane in (segment x, segment y) order and the image's description"""
    res, hi, dmin, dmax = p.proj_image_resolution, p.proj_image_high_inc, p.proj_dis_min, p.proj_dis_max
    A, B, Cc = normal
    D = -((A * centre[0] + B * centre[1]) + Cc * centre[2])                              # :629
    xa, ya = axes(normal)
    dx = -((xa[0] * centre[0] + xa[1] * centre[1]) + xa[2] * centre[2])                  # :648
    dy = -((ya[0] * centre[0] + ya[1] * centre[1]) + ya[2] * centre[2])                  # :653
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    dis = np.abs(((x * A + y * B) + z * Cc) + D)                                         # :663
    keep = (dis >= dmin) & (dis <= dmax)                                                 # :665
    if not exact_plane:
        mg.note("dis_max", (dis - dmax) / dmax)
        if dmin > 0:
            mg.note("dis_min", (dis - dmin) / dmin)
    den = (A * A + B * B) + Cc * Cc
    c0 = (-A * ((B * y + Cc * z) + D) + x * (B * B + Cc * Cc)) / den                     # :676-681
    c1 = (-B * ((A * x + Cc * z) + D) + y * (A * A + Cc * Cc)) / den
    c2 = (-Cc * ((A * x + B * y) + D) + z * (A * A + B * B)) / den
    px = (((c0 * ya[0] + c1 * ya[1]) + c2 * ya[2]) + dy)[keep]                           # :686 project_x runs along y_axis
    py = (((c0 * xa[0] + c1 * xa[1]) + c2 * xa[2]) + dx)[keep]                           # :688
    dk = dis[keep]
    img = dict(plane=plane, kept=int(keep.sum()), valid=False, x_axis=xa, y_axis=ya)
    if px.shape[0] <= 5:                                                                 # :699
        return [], img
    min_x = min(10.0, float(px.min())); max_x = max(-10.0, float(px.max()))              # :695-715
    min_y = min(10.0, float(py.min())); max_y = max(-10.0, float(py.max()))
    seg_len = SEG * res
    fx, fy = (max_x - min_x) / seg_len + 1, (max_y - min_y) / seg_len + 1                # :719-720
    lx, ly = (max_x - min_x) / res + SEG, (max_y - min_y) / res + SEG                    # :721-722
    mg.note("size_truncation", [v - np.round(v) for v in (fx, fy, lx, ly)])
    x_seg, y_seg, x_len, y_len = int(fx), int(fy), int(lx), int(ly)
    assert x_len < 2 ** 24 and y_len < 2 ** 24
    qx, qy = (px - min_x) / res, (py - min_y) / res                                      # :758-759
    mg.note("cell_edge", np.concatenate([qx - np.round(qx), qy - np.round(qy)])[np.concatenate([qx, qy]) > 0.5])
    cx, cy = qx.astype(np.int64), qy.astype(np.int64)
    cut_num = int((dmax - dmin) / hi)                                                    # :770
    qb = (dk - dmin) / hi                                                                # :780
    if not exact_plane:
        mg.note("height_bin", (qb - np.round(qb))[qb > 0.5])
    bin_ = qb.astype(np.int64)
    cell = cx * y_len + cy
    ucell, inv = np.unique(cell, return_inverse=True)
    inv = inv.reshape(-1)
    K = ucell.shape[0]
    cnt = np.zeros(K, dtype=np.int64); sx = np.zeros(K); sy = np.zeros(K)
    np.add.at(cnt, inv, 1); np.add.at(sx, inv, px); np.add.at(sy, inv, py)               # :760-762, input order
    occ = np.zeros(K, dtype=np.uint64)
    ok = bin_ < cut_num                      # a bin that reaches cut_num (dis == dis_max): counted, no bit -- the reference writes out of bounds
    np.bitwise_or.at(occ, inv[ok], np.uint64(1) << bin_[ok].astype(np.uint64))
    summ = np.array([bin(int(o)).count("1") for o in occ], dtype=np.int64)               # :783-792
    table = {int(c): k for k, c in enumerate(ucell)}

    def S(ix, iy):                                                                       # dis_array; an empty or outside cell reads 0
        if ix < 0 or iy < 0 or ix >= x_len or iy >= y_len:
            return 0
        k = table.get(ix * y_len + iy)
        return 0 if k is None else int(summ[k])

    occupied_segments = sorted({(int(a) // SEG, int(b) // SEG) for a, b in zip(ucell // y_len, ucell % y_len)})
    cands = []
    for sxi, syi in occupied_segments:                                                   # :803-806 (an empty segment yields nothing)
        if sxi >= x_seg or syi >= y_seg:
            continue
        best, bx, by = 0, -10, -10
        for ix in range(sxi * SEG, (sxi + 1) * SEG):                                     # :810-820
            for iy in range(syi * SEG, (syi + 1) * SEG):
                if S(ix, iy) > best:
                    best, bx, by = S(ix, iy), ix, iy
        if best == 0 or not best >= p.summary_min_thre:                                  # :821
            continue
        k = table[bx * y_len + by]
        if p.touch_filter_enable and not (int(occ[k]) & 15):                             # :823-832
            continue
        if bx <= 0 or bx >= x_len - 1 or by <= 0 or by >= y_len - 1:                     # :854-857
            continue
        if p.line_filter_enable:                                                         # :860-890
            hit = False
            for ddx, ddy in ((0, 1), (1, 0), (1, 1), (1, -1)):
                hit |= line_hit(best, S(bx + ddx, by + ddy), S(bx - ddx, by - ddy))
            if hit:
                continue
        mpx, mpy = sx[k] / cnt[k], sy[k] / cnt[k]                                        # :893-898
        loc = (mpy * xa + mpx * ya) + centre                                             # :899
        cands.append(dict(plane=plane, cell_x=bx, cell_y=by, count=int(cnt[k]), summary=best, occupancy=int(occ[k]), location=loc))
    img.update(valid=True, min_x=min_x, min_y=min_y, x_len=x_len, y_len=y_len, x_seg=x_seg, y_seg=y_seg, cells=K,
               cell_table={(int(c) // y_len, int(c) % y_len): (int(cnt[k]), int(occ[k])) for k, c in enumerate(ucell)})
    return cands, img


# ---- 6. / 7. ---------------------------------------------------------------------------------------------------------------------------
def suppress(loc, summary, radius, mg):
    """:926-977; FLANN's radius result set: float32 squared distance strictly below float32(radius^2)"""
    n = loc.shape[0]
    if n == 0:
        return np.zeros(0, dtype=bool)
    f = loc.astype(np.float32)
    d = f[:, None, :] - f[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    r2 = np.float32(radius * radius)
    off = ~np.eye(n, dtype=bool)
    mg.note("suppression", ((d2.astype(np.float64) - float(r2)) / float(r2))[off])
    near = (d2 < r2) & off
    return ~np.any(near & (summary[None, :] >= summary[:, None]), axis=1)                # :960


def cut(kept_idx, summary, useful):
    """:601-609 with a stable sort"""
    kept_idx = np.asarray(kept_idx, dtype=np.int64)
    if useful > kept_idx.shape[0]:
        return kept_idx
    return kept_idx[np.argsort(-summary[kept_idx], kind="stable")][:useful]


# ---- the whole -------------------------------------------------------------------------------------------------------------------------
def extract(xyz, p=None, planes=None):
    """GenerateSTDescs (:156-186) without generate_std.  planes = (centres, normals): stages 4-7 on that list."""
    p = p or Params()
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    mg = Margins()
    out = dict(margins=mg, planes=np.zeros((0, REC)), labels=np.zeros(0, dtype=np.int32), late=[], group_sizes=[], used_gaps=[])
    empty = dict(locations=np.zeros((0, 3)), occupancy=np.zeros(0, dtype=np.uint64), summary=np.zeros(0, dtype=np.int32), candidates=[], kept=np.zeros(0, dtype=bool),
                 proj=np.zeros((0, REC)), used=np.zeros(0, dtype=np.int32), images=[], order=np.zeros(0, dtype=np.int64))
    out.update(empty)
    if xyz.shape[0] == 0:
        return out
    proj_gaps = None
    if planes is None:
        rows, vox, gaps = plane_records(xyz, p, mg)
        out["planes"], out["voxels"], out["voxel_gaps"] = rows, vox, gaps
        ids, late = label_rows(pair_matrix(rows, p, mg)) if rows.shape[0] else (np.zeros(0, dtype=np.int32), [])
        out["labels"], out["late"] = ids, late
        g1 = []
        proj, sizes = fold_groups(rows, ids, False, mg, g1)                              # :172
        out["group_sizes"] = sizes
        out["merged_first"] = proj.shape[0]
        if proj.shape[0] == 0:                                                           # :173-179
            proj = np.zeros((1, REC)); proj[0, 0:3] = xyz[0]; proj[0, 12] = 1.0
            proj_gaps = [np.inf]
        else:
            order = np.argsort(-proj[:, 9], kind="stable")                              # :181
            proj = proj[order]; g1 = [g1[k] for k in order]
            if proj.shape[0] > 1:                                                        # :462
                ids2, _ = label_rows(pair_matrix(proj, p, mg))
                g2 = []
                merged, sizes2 = fold_groups(proj, ids2, True, mg, g2)
                out["group_sizes_second"] = sizes2
                proj = sort_by_size(merged)                                              # :183
                g1 = None                                                                # the gaps of the used planes are taken below
            proj_gaps = g1
    else:
        c, n = np.asarray(planes[0], dtype=np.float64).reshape(-1, 3), np.asarray(planes[1], dtype=np.float64).reshape(-1, 3)
        proj = np.zeros((c.shape[0], REC)); proj[:, 0:3] = c; proj[:, 10:13] = n
    used = gate(proj[:, 10:13], p.proj_plane_num, mg)
    out["proj"] = proj
    u_of = -np.ones(proj.shape[0], dtype=np.int32)
    u_of[used] = np.arange(len(used))
    out["used"] = u_of
    if planes is None:
        for i in used:                      # the eigen-gap of every used plane: what bounds the difference between two solvers' normals
            if proj[i, 9] > 0:
                lam = np.linalg.eigvalsh(sym6_to_mat(proj[i, 3:9]))
                out["used_gaps"].append(float(lam[1] - lam[0]))
    cands, images = [], []
    for u, i in enumerate(used):
        cs, img = extract_binary(xyz, proj[i, 0:3], proj[i, 10:13], u, p, mg, planes is not None)
        cands += cs; images.append(img)
    out["candidates"], out["images"] = cands, images
    loc = np.array([c["location"] for c in cands]).reshape(-1, 3)
    summ = np.array([c["summary"] for c in cands], dtype=np.int64)
    kept = suppress(loc, summ, p.non_max_suppression_radius, mg)
    out["kept"] = kept
    order = cut(np.nonzero(kept)[0], summ, p.useful_corner_num)
    out["order"] = order
    out["locations"] = loc[order]
    out["occupancy"] = np.array([cands[k]["occupancy"] for k in order], dtype=np.uint64)
    out["summary"] = summ[order].astype(np.int32)
    return out
