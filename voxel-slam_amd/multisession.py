"""Loop closure across sessions (reference: ``thd_loop_closure``, voxelslam.cpp:1806-2129, ``PGO_Edges`` / ``PGO_Edge``, loop_refine.hpp:163-267,
``build_graph``, voxelslam.cpp:1741-1802): every keyframe of the running session is searched against the databases of ALL sessions -- the ones
imported from earlier runs and the ones closed by a reset -- in one ``LoopSearch.search_multi``, registered against every session that answered in
one ``LoopRegistration.icp``, and the reference's policy decides which edges are pushed, when the connected sessions are stitched into one graph and
when that graph is optimised.  Host orchestration only: descriptors, search, ICP and the graph solve run on the GPU behind ``vxba``.

What is kept of the reference as it is written (and what the tests pin against a literal restatement of it, tests/_multisession_ref.py):
the first contact with a session (no edge to it in the running graph: ``step == -1``) is pushed and optimised whatever its drift; ``relc_count`` grows
for every session on every keyframe; a drift over a zero journey is an IEEE division (inf or NaN: not pushed); the running graph keeps every chain
measurement as taken when its scan was pushed, while ``build_graph`` re-derives all of them from the current poses.

``search_cls`` / ``reg_cls`` / ``graph_cls``: stand-ins with the methods of ``vxba.LoopSearch`` / ``LoopRegistration`` / ``PoseGraph`` used here (the
convention of ``hba``); the tests run the whole policy through numpy checkers on the CPU that way."""
from __future__ import annotations

import numpy as np

from . import hba, sessionio, vxba

V6_INIT = 1e-4          # loop edges (voxelslam.cpp:1842)
V6_RUNNING_PRIOR = 1e-6   # the prior on node 0 of a fresh running graph (:1843, :1925)
V6_BUILD_PRIOR = hba.PRIOR_V6   # the prior of build_graph (:1778)
CROSS_RATIO = 0.05      # drift_p / jours[id] of a session already connected (:2044)
CROSS_DRIFT = 0.25      # [m] (:2048)
CURRENT_DRIFT = 0.10    # [m] (:2018)


def _rot(pose12):
    return np.asarray(pose12, dtype=np.float64).reshape(12)[:9].reshape(3, 3).T


class SessionEdges:
    """``PGO_Edges``: loop edges grouped by the ordered session pair (m1, m2), and ``mates``, the adjacency of the sessions that share a group."""

    def __init__(self):
        self.edges = []          # dict(m1, m2, ids1, ids2, rots, tras, covs) in the order the pairs first appeared
        self.mates = []

    def push(self, m1, m2, id1, id2, rot, tra, v6):
        rec = (int(id1), int(id2), np.array(rot, dtype=np.float64).reshape(3, 3), np.array(tra, dtype=np.float64).reshape(3), np.array(v6, dtype=np.float64).reshape(6))
        for e in self.edges:
            if e["m1"] == m1 and e["m2"] == m2:
                break
        else:
            e = dict(m1=int(m1), m2=int(m2), ids1=[], ids2=[], rots=[], tras=[], covs=[])
            self.edges.append(e)
            while len(self.mates) < max(m1, m2) + 1:
                self.mates.append([])
            self.mates[m1].append(int(m2))
            self.mates[m2].append(int(m1))
        for k, v in zip(("ids1", "ids2", "rots", "tras", "covs"), rec):
            e[k].append(v)

    def connect(self, root):
        """The sessions reachable from ``root`` over ``mates``, depth first in insertion order, sorted ascending."""
        ids = [int(root)]

        def walk(o):
            if o < len(self.mates):
                for m in self.mates[o]:
                    if m not in ids:
                        ids.append(m)
                        walk(m)
        walk(int(root))
        return sorted(ids)

    @staticmethod
    def adapt(edge, ids):
        """``PGO_Edge::is_adapt``: the positions of the group's two sessions in ``ids`` (the last one where a session is listed twice), or None."""
        step = [None, None]
        for i, m in enumerate(ids):
            if edge["m1"] == m:
                step[0] = i
            if edge["m2"] == m:
                step[1] = i
        return None if step[0] is None or step[1] is None else (step[0], step[1])

    def to_arrays(self):
        """Data only -- dict(pairs (G, 2), ptr (G + 1,), ids (n, 2) int64; rot (n, 9) row-major, tra (n, 3), v6 (n, 6) float64) -- for a caller that
        keeps the edges between runs; ``from_arrays`` gives the same groups and the same ``mates`` back."""
        G = len(self.edges)
        ptr = np.concatenate([[0], np.cumsum([len(e["ids1"]) for e in self.edges])]).astype(np.int64)
        n = int(ptr[-1])
        cat = lambda k, w: np.array([np.reshape(x, w) for e in self.edges for x in e[k]], dtype=np.float64).reshape(n, w)
        return dict(pairs=np.array([(e["m1"], e["m2"]) for e in self.edges], dtype=np.int64).reshape(G, 2), ptr=ptr,
                    ids=np.array([(a, b) for e in self.edges for a, b in zip(e["ids1"], e["ids2"])], dtype=np.int64).reshape(n, 2),
                    rot=cat("rots", 9), tra=cat("tras", 3), v6=cat("covs", 6))

    @classmethod
    def from_arrays(cls, a):
        out = cls()
        for g, (m1, m2) in enumerate(np.asarray(a["pairs"]).reshape(-1, 2)):
            for k in range(int(a["ptr"][g]), int(a["ptr"][g + 1])):
                out.push(int(m1), int(m2), a["ids"][k][0], a["ids"][k][1], np.asarray(a["rot"][k]).reshape(3, 3), a["tra"][k], a["v6"][k])
        return out


class _Session:
    def __init__(self, search, jud, relc_count):
        self.search = search
        self.cloud_ids, self.scan_index = [], []      # per frame: its plane cloud and the scan it was made at (header.seq)
        self.poses, self.v6, self.vel = np.zeros((0, 12)), np.zeros((0, 6)), np.zeros((0, 3))
        self.keyframes = []                            # (id: scan index, jour)
        self.x0 = np.zeros((0, 12))                    # one pose per keyframe: its scan's pose when it was made, poses[id] after every optimisation
        self.jud, self.jour, self.relc_count = float(jud), 0.0, int(relc_count)
        self.skip = None                               # None: the params' skip_near_num (a session being built)
        self.saved = None                              # the vxba.SavedSession of a session reloaded from disk (import_saved)
        self.hba = None                                # the vxba.HbaSession holding a running session's keyframe clouds (attach_hba)


class MultiSession:
    """The sessions' state and the policy of ``thd_loop_closure``.  Session ids count from 0 in the order of ``import_session`` / ``new_session``; the
    running session is the last."""

    def __init__(self, reg=None, params: "vxba.LoopSearchParams | None" = None, icp_options=None, pgo_options=None, jud_default: float = 0.45,
                 icp_eigval: float = 14.0, ratio_drift: float = 0.05, curr_halt: int = 10, prev_halt: int = 30, device: int = 0, search_cls=None, reg_cls=None,
                 graph_cls=None):
        self.params = params if params is not None else vxba.LoopSearchParams()
        self.jud_default, self.ratio_drift, self.curr_halt, self.prev_halt = float(jud_default), float(ratio_drift), int(curr_halt), int(prev_halt)
        self.icp_options = icp_options if icp_options is not None else vxba.IcpOptions(icp_eigval=icp_eigval)
        self.pgo_options, self.device = pgo_options, device
        self._search_cls = search_cls if search_cls is not None else (lambda reg: vxba.LoopSearch(reg, device=device))
        self._graph_cls = graph_cls if graph_cls is not None else (lambda: vxba.PoseGraph(device=device))
        self._own_reg = reg is None
        self.reg = reg if reg is not None else (reg_cls() if reg_cls is not None else vxba.LoopRegistration(device=device))
        self.edges = SessionEdges()
        self.sessions = [_Session(self._search_cls(self.reg), self.jud_default, self.prev_halt)]
        self.g_update = 0
        self._fresh_graph()

    def close(self):
        for s in self.sessions:
            s.search.close()
            if s.saved is not None:
                s.saved.close()
        if self._own_reg:
            self.reg.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def cur_id(self):
        return len(self.sessions) - 1

    @property
    def current(self):
        return self.sessions[-1]

    # ---- the running graph: nodes in (ids, scan) order; groups of between factors with the node offsets of their two ends; priors ----
    def _fresh_graph(self):
        self.ids, self.stepsizes = [self.cur_id], [0, 0]
        self.initial = np.zeros((0, 12))
        self.priors = []                                # (node, pose (12,), variance)
        self.groups = [dict(ij=[], data=[], off=(0, 0))]   # the last group takes what push_scan / push_keyframe add, under global node numbers

    def graph_factors(self):
        """The running graph flattened: (i, j, record (18,)) per between factor in the order added, and the priors."""
        out = []
        for g in self.groups:
            for (i, j), d in zip(g["ij"], g["data"]):
                out.append((int(i) + g["off"][0], int(j) + g["off"][1], np.asarray(d, dtype=np.float64)))
        return out, list(self.priors)

    @staticmethod
    def _between(a, b, v6):
        """add_edge(pos1, pos2, x1, x2, ...) (loop_refine.hpp:147-153): the record of x1^-1 x2."""
        Ra, Rb = _rot(a), _rot(b)
        return np.concatenate([(Ra.T @ Rb).reshape(9), Ra.T @ (b[9:] - a[9:]), np.asarray(v6, dtype=np.float64).reshape(6)])

    # ---- sessions ----
    def import_session(self, frames, scan_poses, v6, jud=None, keyframes=None):
        """The descriptor half of ``previous_map_read`` (voxelslam.cpp:376-401): an earlier session becomes searchable.  ``frames``: per keyframe
        ((corner locations, occupancy), plane cloud -- (n, 6) rows, or the id of one the registration handle holds --, scan index); ``scan_poses``
        (n, 12) and ``v6`` (n, 6 or 6) of ALL its scans.  Only while the running session is empty; the imported session takes its id and the
        running one moves up.  ``keyframes``: the scan indices of ALL the session's keyframes where there are more of them than frames (a reloaded
        session: one frame per descriptor window) -- what x0 follows after an optimisation; default: one keyframe per frame.  Returns the imported
        session's id."""
        cur = self.current
        if cur.poses.shape[0] or cur.search.num_frames():
            raise vxba.VxbaError("import_session: VXBA_ERR_STATE: the running session has begun")
        s = _Session(cur.search, self.jud_default if jud is None else jud, self.prev_halt)      # the empty handle goes with the id; the running session gets a new one
        cur.search = self._search_cls(self.reg)
        s.poses = np.array(scan_poses, dtype=np.float64).reshape(-1, 12)
        s.v6 = np.array(np.broadcast_to(np.asarray(v6, dtype=np.float64).reshape(-1, 6), (s.poses.shape[0], 6)))
        s.vel = np.zeros((s.poses.shape[0], 3))
        for corners, cloud, scan_index in frames:
            cid = int(cloud) if np.isscalar(cloud) else self.reg.add_cloud(cloud)
            s.search.describe(corners[0], corners[1], self.params)
            s.search.add(cid)
            s.cloud_ids.append(cid); s.scan_index.append(int(scan_index)); s.keyframes.append((int(scan_index), 0.0))
        if keyframes is not None:
            s.keyframes = [(int(k), 0.0) for k in keyframes]
        s.x0 = s.poses[[k for k, _ in s.keyframes]].copy() if s.keyframes else np.zeros((0, 12))
        s.skip = -(s.search.num_frames() + 10)
        self.sessions.insert(len(self.sessions) - 1, s)
        self._fresh_graph()
        return len(self.sessions) - 2

    def import_saved(self, source, jud=None, win_size: int = 10, voxel_size: float = 1.0, acsize: int = 10, mgsize: int = 5, corner_params=None, corners=None,
                     plane_params=None):
        """``previous_map_read`` for one session (voxelslam.cpp:313-404): ``source`` is a session directory or the tuple ``sessionio.read_session``
        returns.  The scans go to the device once (``vxba.SavedSession``); keyframes, descriptor clouds, corners (``corners``: a
        ``vxba.CornerExtractor`` to reuse) and plane clouds are made there, device to device, and the frames are handed to ``import_session``.  The
        ``SavedSession`` stays with the session: ``optimise`` pushes its result into it, ``global_map`` reads it.  A window without a point (n = 0,
        no device address) still makes a frame, as upstream's loop does: no corner, no descriptor, an empty plane cloud -- both consumers take
        (0, NULL).  ``plane_params``: the ``vxba.PlaneCloudParams`` of the plane clouds (default: the library's).  Returns the session's id."""
        scans, _, states, v6 = sessionio.read_session(source) if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__") else source
        poses = np.ascontiguousarray(np.asarray(states, dtype=np.float64).reshape(len(scans), -1)[:, :12])
        saved = vxba.SavedSession(device=self.device)
        ce = corners if corners is not None else vxba.CornerExtractor(device=self.device)
        try:
            saved.load_scans(scans, poses)
            K = saved.build_keyframes(win_size, voxel_size)
            frames = []
            for w in range(vxba.SavedSession.num_windows(K, acsize, mgsize)):
                wc = saved.window_cloud(w, acsize, mgsize)
                ce.extract_device(wc["n"], wc["d_xyz"], corner_params)
                c = ce.read()
                frames.append(((c["locations"], c["occupancy"]), self.reg.add_keyframe_device(wc["n"], wc["d_xyz"], plane_params), wc["frame_id"]))
            sid = self.import_session(frames, poses, v6, jud, keyframes=saved.keyframes()["ids"])
        except Exception:
            saved.close()
            raise
        finally:
            if corners is None:
                ce.close()
        self.sessions[sid].saved = saved
        return sid

    def attach_hba(self, session: "vxba.HbaSession", sid=None):
        """The ``HbaSession`` that holds the keyframe clouds of session ``sid`` (default: the running one), keyframe k of it being keyframe k of the
        session: it takes part in ``global_map`` through them."""
        self.sessions[self.cur_id if sid is None else sid].hba = session

    def global_path(self, ids=None):
        """``pub_global_path``: (n, 4) float32 rows (p, session id) of the sessions ``ids`` (default: all)."""
        ids = list(range(len(self.sessions))) if ids is None else list(ids)
        return sessionio.global_path([s.poses for s in self.sessions], ids)

    def global_map(self, ids=None, interval_size: int = 5000000):
        """``pub_globalmap`` over the sessions ``ids`` (default: every session that holds keyframe clouds on the device -- a reloaded one, or one with
        an ``HbaSession`` attached) under their current x0: ``vxba.global_map``'s dict."""
        chosen = [i for i, s in enumerate(self.sessions) if s.saved is not None or s.hba is not None] if ids is None else list(ids)
        sets = []
        for i in chosen:
            s = self.sessions[i]
            if s.saved is not None:
                sets.append(s.saved.map_set(i))
            elif s.hba is not None:
                d, ptr = s.hba.device_clouds()
                if ptr.size - 1 != len(s.keyframes):
                    raise vxba.VxbaError(f"global_map: VXBA_ERR_STATE: session {i} has {len(s.keyframes)} keyframes, its HbaSession {ptr.size - 1}")
                sets.append(dict(d_xyz=d, cloud_ptr=ptr, poses=s.x0, id=i))
            else:
                raise vxba.VxbaError(f"global_map: VXBA_ERR_STATE: session {i} holds no keyframe clouds on the device")
        return vxba.global_map(sets, interval_size, device=self.device)

    def new_session(self):
        """The reset branch (voxelslam.cpp:1856-1887): the running session is closed -- searchable from now on whatever the distance in frames -- and
        an empty one begins with an empty graph.  Returns the new session's id."""
        closing = self.current
        closing.skip = -(closing.search.num_frames() + 10)
        self.sessions.append(_Session(self._search_cls(self.reg), self.jud_default, self.prev_halt))
        self._fresh_graph()
        return self.cur_id

    # ---- scans and keyframes ----
    def push_scan(self, pose, v6, velocity=None):
        """voxelslam.cpp:1909-1929: the scan joins the running session and the running graph -- chained to the scan before it by the relative pose of
        the two AS THEY ARE NOW under that scan's v6, or, as node 0 of a fresh graph, held by a prior at 1e-6.  Returns the scan's index."""
        s = self.current
        xc = np.array(pose, dtype=np.float64).reshape(12)
        g_pos = self.stepsizes[-1]
        self.initial = np.concatenate([self.initial, xc[None]])
        if g_pos > 0:
            self.groups[-1]["ij"].append((g_pos - 1, g_pos))
            self.groups[-1]["data"].append(self._between(s.poses[-1], xc, s.v6[-1]))
        else:
            self.priors.append((0, xc.copy(), V6_RUNNING_PRIOR))
        s.poses = np.concatenate([s.poses, xc[None]])
        s.v6 = np.concatenate([s.v6, np.asarray(v6, dtype=np.float64).reshape(1, 6)])
        s.vel = np.concatenate([s.vel, np.zeros((1, 3)) if velocity is None else np.asarray(velocity, dtype=np.float64).reshape(1, 3)])
        self.stepsizes[-1] += 1
        return s.poses.shape[0] - 1

    def push_keyframe(self, corners, cloud_id, scan_index=None, jour_step: float = 0.0):
        """voxelslam.cpp:1940-2081 for one keyframe of the running session: ``corners`` = (locations, occupancy), ``cloud_id`` its plane cloud in the
        registration handle, ``scan_index`` the scan it was made at (default: the newest), ``jour_step`` the distance travelled since the last one.
        Returns the record of every decision: per session that was found, the quantity compared and its threshold at every test it reached."""
        cur, cur_id = self.current, self.cur_id
        if cur.poses.shape[0] == 0:
            raise vxba.VxbaError("push_keyframe: VXBA_ERR_STATE: no scan has been pushed")
        scan_index = cur.poses.shape[0] - 1 if scan_index is None else int(scan_index)
        for s in self.sessions:
            s.jour += float(jour_step)
        cur.keyframes.append((scan_index, cur.jour))
        cur.x0 = np.concatenate([cur.x0, cur.poses[scan_index][None]])      # Keyframe(xc): a keyframe has a pose from its creation on, optimised or not
        cur.search.describe(corners[0], corners[1], self.params)
        skips = [self.params.skip_near_num if s.skip is None else s.skip for s in self.sessions]
        found = cur.search.search_multi([s.search for s in self.sessions], skips, int(cloud_id), self.params)
        tried = [i for i, r in enumerate(found) if r["frame"] >= 0 and r["score"] > self.sessions[i].jud]
        icp = None
        if tried:
            pairs = [[int(cloud_id), self.sessions[i].cloud_ids[found[i]["frame"]]] for i in tried]
            icp = self.reg.icp(pairs, np.array([found[i]["pose"] for i in tried]), self.icp_options)
        xc = cur.poses[-1]
        rec = dict(session=cur_id, keyframe=len(cur.keyframes) - 1, scan_index=scan_index, sessions=[], isGraph=False, isOpt=False, match_num=0, g_update=False)
        for i, r in enumerate(found):
            s = self.sessions[i]
            if r["frame"] < 0:
                continue
            d = dict(id=i, frame=int(r["frame"]), score=float(r["score"]), jud=s.jud, tried=i in tried)
            rec["sessions"].append(d)
            if i not in tried:
                continue
            b = tried.index(i)
            d["accept"] = bool(icp["accept"][b])
            if not d["accept"]:
                continue
            P = icp["poses"][b]
            rot, tra = _rot(P), P[9:].copy()
            ord_bl = s.scan_index[r["frame"]]
            xx = s.poses[ord_bl]
            drift_p = float(np.linalg.norm(_rot(xx) @ tra + xx[9:] - xc[9:]))
            d.update(ord_bl=int(ord_bl), drift_p=drift_p)
            push, step = False, -1
            with np.errstate(divide="ignore", invalid="ignore"):
                if i == cur_id:
                    span = cur.keyframes[-1][1] - cur.keyframes[r["frame"]][1]
                    ratio = float(np.float64(drift_p) / np.float64(span))
                    d.update(kind="current", span=float(span), ratio=ratio, ratio_threshold=self.ratio_drift)
                    if ratio < self.ratio_drift:
                        push, step = True, len(self.stepsizes) - 2
                        d.update(relc_count=s.relc_count, halt=self.curr_halt, drift_threshold=CURRENT_DRIFT)
                        if s.relc_count > self.curr_halt and drift_p > CURRENT_DRIFT:
                            rec["isOpt"] = True
                            for t in self.sessions:
                                t.relc_count = 0
                else:
                    for k, m in enumerate(self.ids):
                        if m == i:
                            step = k
                    if step == -1:
                        d.update(kind="first_contact", jour=s.jour)
                        rec["isGraph"] = rec["isOpt"] = rec["g_update"] = True
                        s.relc_count = 0
                        self.g_update = 1
                        push = True
                        s.jour = 0.0
                    else:
                        ratio = float(np.float64(drift_p) / np.float64(s.jour))
                        d.update(kind="connected", jour=s.jour, ratio=ratio, ratio_threshold=CROSS_RATIO)
                        if ratio < CROSS_RATIO:
                            s.jour = 1e-6
                            push = True
                            d.update(relc_count=s.relc_count, halt=self.prev_halt, drift_threshold=CROSS_DRIFT)
                            if s.relc_count > self.prev_halt and drift_p > CROSS_DRIFT:
                                rec["isOpt"] = True
                                for t in self.sessions:
                                    t.relc_count = 0
            d.update(push=push, step=step)
            if push:
                rec["match_num"] += 1
                self.edges.push(i, cur_id, ord_bl, scan_index, rot, tra, np.full(6, V6_INIT))
                if step > -1:
                    id1, id2 = self.stepsizes[step] + ord_bl, self.stepsizes[-1] - 1
                    d.update(node_i=int(id1), node_j=int(id2))
                    self.groups[-1]["ij"].append((id1, id2))
                    self.groups[-1]["data"].append(np.concatenate([rot.reshape(9), tra, np.full(6, V6_INIT)]))
        for s in self.sessions:
            s.relc_count += 1
        cur.search.add(int(cloud_id))
        cur.cloud_ids.append(int(cloud_id)); cur.scan_index.append(scan_index)
        rec["found"] = found
        if rec["isGraph"]:
            self.build_graph(1)
        rec["ids"], rec["stepsizes"] = list(self.ids), list(self.stepsizes)
        rec["optimised"] = self.optimise() if rec["isOpt"] else None
        return rec

    def build_graph(self, lpedge_enable: int = 1):
        """voxelslam.cpp:1741-1802: the graph over every session connected to the running one -- their scans as nodes, session after session in
        ascending id; every chain re-derived from the CURRENT poses under each scan's own v6; one prior at 1e-9 on the first node; with
        ``lpedge_enable`` every loop edge between two connected sessions, under v6_init, at ``stepsizes[step] + id``."""
        self.ids = self.edges.connect(self.cur_id)
        self.stepsizes = [0]
        for m in self.ids:
            self.stepsizes.append(self.stepsizes[-1] + self.sessions[m].poses.shape[0])
        self.initial = np.concatenate([self.sessions[m].poses for m in self.ids]) if self.ids else np.zeros((0, 12))
        self.groups, self.priors = [], []
        for ii, m in enumerate(self.ids):
            s = self.sessions[m]
            if s.poses.shape[0] >= 2:
                ij, data = hba.chain_edges(s.poses, s.v6[:-1])
                self.groups.append(dict(ij=[tuple(r) for r in ij], data=list(data), off=(self.stepsizes[ii], self.stepsizes[ii])))
        first = self.sessions[self.ids[0]]
        if first.poses.shape[0] != 0:
            self.priors.append((0, first.poses[0].copy(), V6_BUILD_PRIOR))
        if lpedge_enable == 1:
            for e in self.edges.edges:
                step = SessionEdges.adapt(e, self.ids)
                if step is None:
                    continue
                data = [np.concatenate([r.reshape(9), t, np.full(6, V6_INIT)]) for r, t in zip(e["rots"], e["tras"])]
                self.groups.append(dict(ij=list(zip(e["ids1"], e["ids2"])), data=data, off=(self.stepsizes[step[0]], self.stepsizes[step[1]])))
        self.groups.append(dict(ij=[], data=[], off=(0, 0)))
        return self.ids, self.stepsizes

    def optimise(self):
        """voxelslam.cpp:2090-2129: the running graph through the pose-graph solver, the result written back per (session, scan): poses, the
        keyframes' x0, the velocities turned with their poses; the solution becomes the graph's initial value.  Returns dict(dx: (R, p), what the
        optimisation did to the newest scan -- x_new = dx x_old --, poses: the running session's, for ``vxba_map_loop_update``, graph: the solver's
        own result)."""
        cur = self.current
        g = self._graph_cls()
        try:
            g.set_poses(self.initial)
            for node, pose, var in self.priors:
                g.add_priors([node], pose[None], np.full((1, 6), var))
            for grp in self.groups:
                if grp["ij"]:
                    g.add_edges(np.array(grp["ij"], dtype=np.int32).reshape(-1, 2), np.array(grp["data"]).reshape(-1, 18), grp["off"][0], grp["off"][1])
            out = g.optimize(self.pgo_options) if self.pgo_options is not None else g.optimize()
        finally:
            g.close()
        res = np.asarray(out["poses"], dtype=np.float64).reshape(-1, 12)
        x1 = cur.poses[-1].copy()
        for ii, m in enumerate(self.ids):
            s = self.sessions[m]
            new = res[self.stepsizes[ii]:self.stepsizes[ii + 1]]
            s.vel = hba.rotate_velocities(s.poses, new, s.vel)
            s.poses = new.copy()
            s.x0 = s.poses[[k for k, _ in s.keyframes]].copy() if s.keyframes else np.zeros((0, 12))
            if s.saved is not None:
                s.saved.set_scan_poses(s.poses)      # kf->x0 = scanPoses[kf->id]->x on the device side too
        self.initial = res.copy()
        x3 = cur.poses[-1]
        dR = _rot(x3) @ _rot(x1).T
        return dict(dx=(dR, x3[9:] - dR @ x1[9:]), poses=cur.poses.copy(), graph=out)
