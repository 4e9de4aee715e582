"""Checkers of the multi-session loop closure (voxel_slam_amd/multisession.py, vxba_loopsearch_search_multi): never the thing run.

1. ``search_multi``: the search over several databases, written over ``tests/_loopsearch_ref.Database.search``.  The reference stamps the query
   with the CURRENT manager's frame number (BTC.cpp:195) and compares it with the SEARCHED manager's entries (BTC.cpp:1184-1186), so an entry j of
   session s is eligible when num_frames(cur) - frame_j > skip[s]; ``Database.search`` tests num_frames(db) - frame_j > skip, hence
   skip_single = skip[s] - (num_frames(cur) - num_frames(db)).  That identity is the whole restatement.
2. Stand-ins for ``vxba.LoopSearch`` (with ``search_multi``), ``vxba.LoopRegistration`` and ``vxba.PoseGraph`` over the numpy checkers
   (_loopsearch_ref, _loopreg_ref, _pgo_ref), and SCRIPTED stand-ins whose answers a test prescribes, so that a stream can be steered into every
   branch of the policy with a stated margin.
3. ``Literal``: thd_loop_closure (voxelslam.cpp:1856-1887, 1909-1929, 1940-2129), PGO_Edges / PGO_Edge (loop_refine.hpp:163-267) and build_graph
   (voxelslam.cpp:1741-1802) restated loop by loop from the reference's text, with the reference's names.
"""
import dataclasses

import numpy as np

from tests import _loopreg_ref as LR
from tests import _loopsearch_ref as S
from tests import _pgo_ref as PG


# ---- 1. the search --------------------------------------------------------------------------------------------------------------------
def single_skip(skip, cur_frames, db_frames):
    return int(skip) - (int(cur_frames) - int(db_frames))


def search_multi(dbs, d, cur_rows, cur_frames, skips, prm=None, perturb=0.0):
    """dbs: ``Database`` objects; d: the checker's descriptors of the current set; cur_frames: frames the CURRENT handle holds.  Returns
    dict(sessions: one ``Database.search`` result per session, matches (n, 3): the lists one after the other with the frame column counting on
    from the frames of the sessions before, offsets (S + 1,))."""
    prm = prm or S.Params()
    out, lists, offs, voff = [], [], [0], 0
    for db, skip in zip(dbs, skips):
        r = db.search(d, cur_rows, dataclasses.replace(prm, skip_near_num=single_skip(skip, cur_frames, db.num_frames)), perturb)
        out.append(r)
        m = r["matches"].copy()
        m[:, 1] += voff
        lists.append(m); offs.append(offs[-1] + m.shape[0]); voff += db.num_frames
    return dict(sessions=out, matches=np.concatenate(lists).reshape(-1, 3) if lists else np.zeros((0, 3), np.int32), offsets=np.array(offs, dtype=np.int64))


# ---- 2. stand-ins ---------------------------------------------------------------------------------------------------------------------
def _ref_params(p):
    return p if isinstance(p, S.Params) else S.Params(**{f.name: getattr(p, f.name) for f in dataclasses.fields(S.Params)}) if p is not None else S.Params()


class RefLoopRegistration:
    """``vxba.LoopRegistration``'s ``add_cloud`` / ``num_clouds`` / ``icp`` over ``_loopreg_ref.icp``."""

    def __init__(self):
        self.clouds = []

    def add_cloud(self, rows):
        self.clouds.append(np.asarray(rows, dtype=np.float32).reshape(-1, 6))
        return len(self.clouds) - 1

    def num_clouds(self):
        return len(self.clouds)

    def icp(self, src_tar, poses, options=None):
        kw = {} if options is None else dict(max_iter=options.max_iter, gates0=tuple(options.gates0), gates1=tuple(options.gates1), step_tol=options.step_tol,
                                             icp_eigval=options.icp_eigval)
        res = [LR.icp(self.clouds[a], self.clouds[b], P, **kw) for (a, b), P in zip(np.asarray(src_tar).reshape(-1, 2), np.asarray(poses).reshape(-1, 12))]
        return dict(poses=np.array([r["pose"] for r in res]).reshape(-1, 12), accept=np.array([r["accept"] for r in res], dtype=bool), detail=res)

    def close(self):
        pass


class RefLoopSearch:
    """``vxba.LoopSearch``'s ``describe`` / ``add`` / ``num_frames`` / ``search_multi`` over ``_loopsearch_ref``."""

    def __init__(self, reg):
        self.reg, self.db, self.d, self.cloud_ids = reg, S.Database(), None, []

    def describe(self, locations, occupancy, params=None):
        self.d = S.describe(locations, occupancy, _ref_params(params))
        return self.d["triangle"].shape[0]

    def add(self, cloud_id):
        self.db.add(self.d, self.reg.clouds[cloud_id])
        self.cloud_ids.append(int(cloud_id))
        return self.db.num_frames - 1

    def num_frames(self):
        return self.db.num_frames

    def search_multi(self, dbs, skip_near_num, cloud_cur, params=None):
        r = search_multi([h.db for h in dbs], self.d, self.reg.clouds[cloud_cur], self.db.num_frames, skip_near_num, _ref_params(params))
        self.last = r
        return [dict(frame=s["frame"], score=s["score"], pose=s["pose"], candidates=s["candidates"]) for s in r["sessions"]]

    def close(self):
        pass


def scripted(plan, reject=()):
    """(search_cls, reg_cls) whose answers are prescribed.  Search handles are numbered in the order they are made -- the session ids, when one is
    made per session --; ``plan[(asking handle, frames it holds, searched handle)]`` = (frame, score, pose (12,)), anything else finds nothing.  The
    registration returns every guess as it is and accepts it unless (source cloud, target cloud) is in ``reject``."""
    made = []

    class Search:
        def __init__(self, reg):
            self.no, self.frames, self.cloud_ids = len(made), 0, []
            made.append(self)

        def describe(self, locations, occupancy, params=None):
            return 0

        def add(self, cloud_id):
            self.frames += 1
            self.cloud_ids.append(int(cloud_id))
            return self.frames - 1

        def num_frames(self):
            return self.frames

        def search_multi(self, dbs, skip_near_num, cloud_cur, params=None):
            out = []
            for h in dbs:
                frame, score, pose = plan.get((self.no, self.frames, h.no), (-1, 0.0, np.zeros(12)))
                out.append(dict(frame=int(frame), score=float(score), pose=np.array(pose, dtype=np.float64).reshape(12), candidates=[]))
            return out

        def close(self):
            pass

    class Registration:
        def __init__(self):
            self.n = 0

        def add_cloud(self, rows):
            self.n += 1
            return self.n - 1

        def num_clouds(self):
            return self.n

        def icp(self, src_tar, poses, options=None):
            st = np.asarray(src_tar).reshape(-1, 2)
            return dict(poses=np.array(poses, dtype=np.float64).reshape(-1, 12), accept=np.array([(int(a), int(b)) not in reject for a, b in st], dtype=bool))

        def close(self):
            pass

    return Search, Registration


# ---- 3. the reference's text ------------------------------------------------------------------------------------------------------------
class PGO_Edge:
    def __init__(self, _m1, _m2, id1, id2, rot, tra, v6):
        self.m1, self.m2 = _m1, _m2
        self.ids1, self.ids2, self.rots, self.tras, self.covs = [], [], [], [], []
        self.push(id1, id2, rot, tra, v6)

    def push(self, id1, id2, rot, tra, v6):
        self.ids1.append(id1); self.ids2.append(id2)
        self.rots.append(np.array(rot)); self.tras.append(np.array(tra))
        self.covs.append(np.array(v6))

    def is_adapt(self, maps, step):
        f1 = f2 = False
        for i in range(len(maps)):
            if self.m1 == maps[i]:
                f1 = True
                step[0] = i
            if self.m2 == maps[i]:
                f2 = True
                step[1] = i
        return f1 and f2


class PGO_Edges:
    def __init__(self):
        self.edges, self.mates = [], []

    def push(self, _m1, _m2, _id1, _id2, rot, tra, v6):
        is_lack = True
        for e in self.edges:
            if e.m1 == _m1 and e.m2 == _m2:
                is_lack = False
                e.push(_id1, _id2, rot, tra, v6)
                break
        if is_lack:
            self.edges.append(PGO_Edge(_m1, _m2, _id1, _id2, rot, tra, v6))
            msize = len(self.mates)
            for i in range(msize, _m2 + 1):
                self.mates.append([])
            self.mates[_m1].append(_m2)
            self.mates[_m2].append(_m1)

    def connect(self, root, ids):
        ids.clear()
        ids.append(root)
        self.tras(root, ids)
        ids.sort()

    def tras(self, ord_, ids):
        if ord_ < len(self.mates):
            for id_ in self.mates[ord_]:
                is_exist = False
                for i in ids:
                    if id_ == i:
                        is_exist = True
                        break
                if not is_exist:
                    ids.append(id_)
                    self.tras(id_, ids)


class ScanPose:
    def __init__(self, x, v6):
        self.x = np.array(x, dtype=np.float64).reshape(12)          # [R column-major | p]
        self.v6 = np.array(v6, dtype=np.float64).reshape(6)

    @property
    def R(self):
        return self.x[:9].reshape(3, 3).T

    @property
    def p(self):
        return self.x[9:]


def add_edge_x(pos1, pos2, x1, x2, graph, noise):
    tt = x1.R.T @ (x2.p - x1.p)
    RR = x1.R.T @ x2.R
    graph.append(("between", pos1, pos2, RR, tt, np.array(noise)))


def add_edge_rt(pos1, pos2, rot, tra, graph, noise):
    graph.append(("between", pos1, pos2, np.array(rot), np.array(tra), np.array(noise)))


class Literal:
    """thd_loop_closure's state and loop.  ``search_cls`` / ``reg_cls``: the stand-ins above; every SearchLoop is one ``search_multi`` over ONE
    manager, every icp_normal one ``icp`` of one pair -- the reference's loop over the sessions, one at a time."""

    def __init__(self, search_cls, reg, params=None, icp_options=None, jud_default=0.45, ratio_drift=0.05, curr_halt=10, prev_halt=30, imported=()):
        self.reg, self.search_cls, self.params, self.icp_options = reg, search_cls, params if params is not None else S.Params(), icp_options
        self.jud_default, self.ratio_drift, self.curr_halt, self.prev_halt = jud_default, ratio_drift, curr_halt, prev_halt
        self.std_managers, self.multimap_scanPoses, self.multimap_keyframes, self.juds, self.skips, self.seqs = [], [], [], [], [], []
        self.lp_edges = PGO_Edges()
        for frames, scan_poses, v6, jud in imported:                # previous_map_read :376-401, the descriptor half
            m = search_cls(reg)
            seq = []
            for corners, cloud, scan_index in frames:
                cid = int(cloud) if np.isscalar(cloud) else reg.add_cloud(cloud)
                m.describe(corners[0], corners[1], self.params)
                m.add(cid)
                seq.append(int(scan_index))
            v6 = np.broadcast_to(np.asarray(v6, dtype=np.float64).reshape(-1, 6), (len(scan_poses), 6))
            self.std_managers.append(m); self.seqs.append(seq)
            self.multimap_scanPoses.append([ScanPose(x, v) for x, v in zip(scan_poses, v6)])
            self.multimap_keyframes.append([dict(id=k, jour=0.0) for k in seq])
            self.juds.append(self.jud_default if jud is None else jud)
            self.skips.append(-(m.num_frames() + 10))
        self.std_manager = search_cls(reg)
        self.std_managers.append(self.std_manager); self.seqs.append([]); self.skips.append(None)
        self.scanPoses, self.keyframes = [], []
        self.multimap_scanPoses.append(self.scanPoses); self.multimap_keyframes.append(self.keyframes)
        self.juds.append(self.jud_default)
        self.jours = [0.0] * len(self.std_managers)
        self.relc_counts = [self.prev_halt] * len(self.std_managers)
        self.v6_init, self.v6_fixd = np.full(6, 1e-4), np.full(6, 1e-6)
        self.initial, self.graph = {}, []
        self.ids, self.stepsizes = [len(self.std_managers) - 1], [0, 0]
        self.buf_base, self.g_update = 0, 0

    def reset(self):                                                # :1856-1887
        self.keyframes = []
        self.multimap_keyframes.append(self.keyframes)
        self.scanPoses = []
        self.multimap_scanPoses.append(self.scanPoses)
        self.buf_base = 0
        self.skips[-1] = -(self.std_manager.num_frames() + 10)
        self.std_manager = self.search_cls(self.reg)
        self.std_managers.append(self.std_manager); self.seqs.append([]); self.skips.append(None)
        self.relc_counts.append(self.prev_halt)
        self.juds.append(self.jud_default)
        self.jours.append(0.0)
        self.initial, self.graph = {}, []
        self.ids = [len(self.std_managers) - 1]
        self.stepsizes = [0, 0]

    def push_scan(self, x, v6):                                     # :1908-1929
        bl_head = ScanPose(x, v6)
        self.scanPoses.append(bl_head)
        xc = bl_head
        g_pos = self.stepsizes[-1]
        self.initial[g_pos] = xc.x.copy()
        if g_pos > 0:
            samv6 = self.scanPoses[self.buf_base - 1].v6
            add_edge_x(g_pos - 1, g_pos, self.scanPoses[self.buf_base - 1], xc, self.graph, samv6)
        else:
            self.graph.append(("prior", 0, xc.x.copy(), self.v6_fixd))
        self.buf_base += 1
        self.stepsizes[-1] += 1

    def build_graph(self, cur_id, lpedge_enable):                   # :1741-1802
        self.initial, self.graph = {}, []
        self.lp_edges.connect(cur_id, self.ids)
        ids, mm = self.ids, self.multimap_scanPoses
        self.stepsizes = [0]
        for i in range(len(ids)):
            self.stepsizes.append(self.stepsizes[-1] + len(mm[ids[i]]))
        stepsizes = self.stepsizes
        for ii in range(len(ids)):
            bsize, id_ = stepsizes[ii], ids[ii]
            for j in range(bsize, stepsizes[ii + 1]):
                self.initial[j] = mm[id_][j - bsize].x.copy()
                if j > bsize:
                    samv6 = mm[ids[ii]][j - 1 - bsize].v6
                    add_edge_x(j - 1, j, mm[id_][j - 1 - bsize], mm[id_][j - bsize], self.graph, samv6)
        if len(mm[ids[0]]) != 0:
            ceil = 1
            for i in range(ceil):
                self.graph.append(("prior", i, mm[ids[0]][i].x.copy(), np.full(6, 1e-9)))
        if lpedge_enable == 1:
            for edge in self.lp_edges.edges:
                step = [0, 0]
                if edge.is_adapt(ids, step):
                    mp = [stepsizes[step[0]], stepsizes[step[1]]]
                    for i in range(len(edge.rots)):
                        id1 = mp[0] + edge.ids1[i]
                        id2 = mp[1] + edge.ids2[i]
                        add_edge_rt(id1, id2, edge.rots[i], edge.tras[i], self.graph, self.v6_init)

    def search_loop(self, id_, cloud):
        skip = self.params.skip_near_num if self.skips[id_] is None else self.skips[id_]
        return self.std_manager.search_multi([self.std_managers[id_]], [skip], cloud, self.params)[0]

    def push_keyframe(self, corners, cloud, jour_step, graph_cls=None):     # :1940-2129
        cur_id = len(self.std_managers) - 1
        xc = self.scanPoses[-1]
        for i in range(len(self.jours)):
            self.jours[i] += jour_step
        smp = dict(id=self.buf_base - 1, jour=self.jours[cur_id])
        self.keyframes.append(smp)
        self.std_manager.describe(corners[0], corners[1], self.params)
        isGraph = isOpt = False
        match_num = 0
        log = []
        for id_ in range(cur_id + 1):
            r = self.search_loop(id_, cloud)
            first, second = r["frame"], r["score"]
            if first >= 0:
                log.append(dict(id=id_, frame=first, score=second, jud=self.juds[id_], tried=bool(second > self.juds[id_])))
            if first >= 0 and second > self.juds[id_]:
                d = log[-1]
                icp = self.reg.icp([[cloud, self.std_managers[id_].cloud_ids[first]]], np.array(r["pose"]).reshape(1, 12), self.icp_options)
                d["accept"] = bool(icp["accept"][0])
                if d["accept"]:
                    P = icp["poses"][0]
                    rot, tra = P[:9].reshape(3, 3).T, P[9:].copy()
                    ord_bl = self.seqs[id_][first]
                    xx = self.multimap_scanPoses[id_][ord_bl]
                    drift_p = float(np.linalg.norm(xx.R @ tra + xx.p - xc.p))
                    d.update(ord_bl=ord_bl, drift_p=drift_p)
                    isPush = False
                    step = -1
                    with np.errstate(divide="ignore", invalid="ignore"):
                        if id_ == cur_id:
                            span = smp["jour"] - self.keyframes[first]["jour"]
                            ratio = float(np.float64(drift_p) / np.float64(span))
                            d.update(kind="current", span=float(span), ratio=ratio, ratio_threshold=self.ratio_drift)
                            if ratio < self.ratio_drift:
                                isPush = True
                                step = len(self.stepsizes) - 2
                                d.update(relc_count=self.relc_counts[id_], halt=self.curr_halt, drift_threshold=0.10)
                                if self.relc_counts[id_] > self.curr_halt and drift_p > 0.10:
                                    isOpt = True
                                    for k in range(len(self.relc_counts)):
                                        self.relc_counts[k] = 0
                        else:
                            for i in range(len(self.ids)):
                                if id_ == self.ids[i]:
                                    step = i
                            if step == -1:
                                d.update(kind="first_contact", jour=self.jours[id_])
                                isGraph = True
                                isOpt = True
                                self.relc_counts[id_] = 0
                                self.g_update = 1
                                isPush = True
                                self.jours[id_] = 0
                            else:
                                ratio = float(np.float64(drift_p) / np.float64(self.jours[id_]))
                                d.update(kind="connected", jour=self.jours[id_], ratio=ratio, ratio_threshold=0.05)
                                if ratio < 0.05:
                                    self.jours[id_] = 1e-6
                                    isPush = True
                                    d.update(relc_count=self.relc_counts[id_], halt=self.prev_halt, drift_threshold=0.25)
                                    if self.relc_counts[id_] > self.prev_halt and drift_p > 0.25:
                                        isOpt = True
                                        for k in range(len(self.relc_counts)):
                                            self.relc_counts[k] = 0
                    d.update(push=isPush, step=step)
                    if isPush:
                        match_num += 1
                        self.lp_edges.push(id_, cur_id, ord_bl, self.buf_base - 1, rot, tra, self.v6_init)
                        if step > -1:
                            id1 = self.stepsizes[step] + ord_bl
                            id2 = self.stepsizes[-1] - 1
                            d.update(node_i=id1, node_j=id2)
                            add_edge_rt(id1, id2, rot, tra, self.graph, self.v6_init)
        for k in range(len(self.relc_counts)):
            self.relc_counts[k] += 1
        self.std_manager.add(cloud)
        self.seqs[cur_id].append(self.buf_base - 1)
        if isGraph:
            self.build_graph(cur_id, 1)
        rec = dict(session=cur_id, keyframe=len(self.keyframes) - 1, scan_index=self.buf_base - 1, sessions=log, isGraph=isGraph, isOpt=isOpt, match_num=match_num,
                   g_update=isGraph, ids=list(self.ids), stepsizes=list(self.stepsizes), optimised=None)
        if isOpt:
            rec["optimised"] = self.optimise(graph_cls or PG.RefPoseGraph)
        return rec

    def flat_graph(self):
        """(between factors (i, j, record (18,)), priors (node, pose (12,), variance)) of the running graph, in the order added."""
        be = [(f[1], f[2], np.concatenate([np.asarray(f[3]).reshape(9), f[4], f[5]])) for f in self.graph if f[0] == "between"]
        pr = [(f[1], f[2], float(f[3][0])) for f in self.graph if f[0] == "prior"]
        return be, pr

    def optimise(self, graph_cls):                                  # :2090-2129, ISAM2 = the pose-graph checker
        n = len(self.initial)
        g = graph_cls()
        g.set_poses(np.array([self.initial[k] for k in range(n)]))
        be, pr = self.flat_graph()
        for node, pose, var in pr:
            g.add_priors([node], pose[None], np.full((1, 6), var))
        if be:
            g.add_edges(np.array([(i, j) for i, j, _ in be], dtype=np.int32), np.array([d for _, _, d in be]))
        results = g.optimize()["poses"]
        g.close()
        x1 = ScanPose(self.scanPoses[self.buf_base - 1].x, np.zeros(6))
        for ii in range(len(self.ids)):
            tip = self.ids[ii]
            for j in range(self.stepsizes[ii], self.stepsizes[ii + 1]):
                ord_ = j - self.stepsizes[ii]
                self.multimap_scanPoses[tip][ord_].x = results[j].copy()
        for ii in range(len(self.ids)):
            tip = self.ids[ii]
            for kf in self.multimap_keyframes[tip]:
                kf["x0"] = self.multimap_scanPoses[tip][kf["id"]].x.copy()
        self.initial = {i: results[i].copy() for i in range(n)}
        x3 = self.scanPoses[self.buf_base - 1]
        dR = x3.R @ x1.R.T
        return dict(dx=(dR, x3.p - dR @ x1.p), poses=np.array([s.x for s in self.scanPoses]))
