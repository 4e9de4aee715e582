"""A session on disk, in the reference's own formats (host only, numpy): what ``save_pose`` / ``save_pcd`` / ``pgo_edges_io`` write
(voxelslam.cpp:163-275), what ``read_lidarstate`` (voxelslam.hpp:217-255), ``previous_map_names`` (voxelslam.cpp:278-305) and the loader of
``previous_map_read`` (:323-336) read, and ``pub_global_path`` (:90-106).  No device, no arithmetic beyond the quaternion conversions.

Layout of a session directory: ``alidarState.txt`` (one line per scan) and ``0.pcd``, ``1.pcd``, ... (one body-frame cloud per scan, in the order of
the lines).  ``edge.txt`` lies next to the session directories and holds the loop edges between them.

Quirks, kept as the reference has them:

* ``alidarState.txt``: ``t`` with 6 decimals, then p (3), the quaternion **x y z w** of R, v, bg, ba, g, v6 (6) -- 26 numbers -- in fixed notation with 7
  decimals (``fixed`` persists after ``setprecision(7)``, :186-193).  The quaternion is Eigen's ``Quaterniond(R)``: trace > 0 gives w = sqrt(t + 1) / 2,
  otherwise the largest diagonal element leads.  A session of fewer than 100 scans is NOT written (:178).
* reading accepts lines of 8, 20 or 26 numbers (t p q | + v bg ba g | + v6; :240-253); what a shorter line leaves out is zero (the reference leaves g
  uninitialised there).  R is built from the quaternion WITHOUT normalising it, as ``Quaterniond::matrix()`` does: a non-unit quaternion gives a
  scaled, non-orthonormal R.  The reference splits at single blanks and would throw at a doubled one; any run of white space separates here.
* ``N.pcd``: binary PCD v0.7 of ``PointXYZI`` as ``savePCDFileBinary`` writes it -- fields x y z intensity, four float32, 16 bytes per point -- with
  the points in the BODY frame and the intensity never set (``save_pcd`` leaves it 0).  The header follows PCL's documented format; it has not been
  checked against a file PCL wrote, none being at hand.  ``read_pcd`` parses the header generally (any field order, extra fields, ``DATA binary`` or
  ``ascii``) and refuses ``binary_compressed``.
* ``edge.txt``: ``name1 name2 id1 id2 tx ty tz qx qy qz qw``, numbers with 7 SIGNIFICANT digits (``setprecision(7)`` without ``fixed``, :267).  On
  reading, an edge whose first session comes later in ``names`` than its second is inverted: t <- -R^T t, R <- R^T, ids and sessions swap (:235-242).
  A line naming a session that is not in ``names`` is kept verbatim as ``absent`` -- unless it names the running bag, then it is dropped (:246-247) --
  and the absent lines are written back first (:255-256).  Every edge read gets v6 = 1e-6 (:205).  Blank lines are skipped (upstream: undefined).
* the list of earlier maps ``"a:0.45, #b:0.5, c:0.4"``: ALL white space is removed first, entries starting with ``#`` are skipped, and a malformed
  entry (not exactly two pieces at ``:``) ends the parse, keeping what came before (:282-303).  An empty name (``":0.4"``) is accepted as the
  session ``""``.  The number is read only for an entry that is kept, so ``"#b:x"`` is skipped like any other ``#`` entry, and it is read as
  ``std::stod`` reads it: the longest numeric prefix (``"0.4x"`` is 0.4).  Where a kept entry has no numeric prefix the reference dies of an
  uncaught ``std::invalid_argument``; here that is a ``ValueError``.
* ``pub_global_path`` emits x, y, z, id as float32 (``pcl::PointXYZI``), sessions in the order of ``ids``.
"""
from __future__ import annotations

import os
import re

import numpy as np

V6_EDGE = 1e-6          # v6_init of pgo_edges_io (:205)
STATE_FILE = "alidarState.txt"


# ---- quaternions, Eigen's conventions ----
def quat_from_rot(R):
    """``Eigen::Quaterniond(R)`` as (x, y, z, w)."""
    m = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)      # x y z w
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def rot_from_quat(x, y, z, w):
    """``Eigen::Quaterniond(w, x, y, z).matrix()``: no normalisation."""
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


# ---- alidarState.txt ----
def write_lidarstate(path, t, states, v6, min_scans: int = 100) -> bool:
    """``save_pose``: ``states`` (n, 24) in ``vxba.pack_state`` order [R column-major 9 | p | v | bg | ba | g], ``t`` (n,), ``v6`` (n, 6) or (6,).
    Fewer than ``min_scans`` scans: nothing is written, False."""
    states = np.asarray(states, dtype=np.float64).reshape(-1, 24)
    n = states.shape[0]
    if n < min_scans:
        return False
    t = np.asarray(t, dtype=np.float64).reshape(n)
    v6 = np.broadcast_to(np.asarray(v6, dtype=np.float64).reshape(-1, 6), (n, 6))
    with open(path, "w") as f:
        for k in range(n):
            s = states[k]
            q = quat_from_rot(s[:9].reshape(3, 3).T)
            nums = np.concatenate([s[9:12], q, s[12:24], v6[k]])
            f.write(f"{t[k]:.6f} " + " ".join(f"{v:.7f}" for v in nums) + "\n")
    return True


def read_lidarstate(path):
    """``read_lidarstate``: (t (n,), states (n, 24), v6 (n, 6))."""
    ts, states, v6s = [], [], []
    with open(path) as f:
        for line in f:
            nums = [float(s) for s in line.split()]
            if not nums:
                continue
            if len(nums) < 8:
                raise ValueError(f"{path}: a line of {len(nums)} numbers (8, 20 or 26 expected)")
            R = rot_from_quat(nums[4], nums[5], nums[6], nums[7])
            st = np.zeros(24)
            st[:9] = R.T.reshape(9)
            st[9:12] = nums[1:4]
            if len(nums) >= 20:
                st[12:24] = nums[8:20]
            ts.append(nums[0]); states.append(st)
            v6s.append(np.array(nums[20:26]) if len(nums) >= 26 else np.zeros(6))
    n = len(ts)
    return np.array(ts, dtype=np.float64), np.array(states, dtype=np.float64).reshape(n, 24), np.array(v6s, dtype=np.float64).reshape(n, 6)


# ---- N.pcd ----
def write_pcd(path, xyz):
    """``pcl::io::savePCDFileBinary`` of a ``PointXYZI`` cloud whose intensity was never set."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rows = np.zeros((n, 4), dtype="<f4")
    rows[:, :3] = xyz
    header = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
              f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rows.tobytes())


_PCD_TYPES = {("F", 4): "<f4", ("F", 8): "<f8", ("I", 1): "<i1", ("I", 2): "<i2", ("I", 4): "<i4", ("I", 8): "<i8",
              ("U", 1): "<u1", ("U", 2): "<u2", ("U", 4): "<u4", ("U", 8): "<u8"}


def read_pcd(path, want_fields: bool = False):
    """The x, y, z of a PCD file as (n, 3) float32; with ``want_fields`` also a dict of every field.  Any field order, extra fields, ``DATA binary``
    or ``ascii``; ``binary_compressed`` raises ValueError."""
    with open(path, "rb") as f:
        buf = f.read()
    hdr, pos, data = {}, 0, None
    while data is None:
        end = buf.find(b"\n", pos)
        if end < 0:
            raise ValueError(f"{path}: no DATA line in the PCD header")
        line = buf[pos:end].decode("ascii", errors="replace").strip()
        pos = end + 1
        if not line or line.startswith("#"):
            continue
        key, _, rest = line.partition(" ")
        if key.upper() == "DATA":
            data = rest.strip().lower()
        else:
            hdr[key.upper()] = rest.split()
    if data == "binary_compressed":
        raise ValueError(f"{path}: DATA binary_compressed is not supported (write the file with savePCDFileBinary or savePCDFileASCII)")
    if data not in ("binary", "ascii"):
        raise ValueError(f"{path}: unknown DATA {data!r}")
    try:
        names = hdr["FIELDS"]
        sizes = [int(s) for s in hdr["SIZE"]]
        types = [s.upper() for s in hdr["TYPE"]]
        counts = [int(s) for s in hdr.get("COUNT", ["1"] * len(names))]
        n = int(hdr["POINTS"][0]) if "POINTS" in hdr else int(hdr["WIDTH"][0]) * int(hdr.get("HEIGHT", ["1"])[0])
    except (KeyError, ValueError, IndexError) as e:
        raise ValueError(f"{path}: incomplete PCD header ({e})") from None
    if not (len(names) == len(sizes) == len(types) == len(counts)) or any((t, s) not in _PCD_TYPES for t, s in zip(types, sizes)):
        raise ValueError(f"{path}: inconsistent FIELDS / SIZE / TYPE / COUNT")
    if any(c not in names for c in "xyz"):
        raise ValueError(f"{path}: no x, y, z fields")
    # fields may repeat a name ("_" is PCL's padding): the dtype gets unique labels, the lookup the first of each name
    labels = [f"{nm}#{i}" for i, nm in enumerate(names)]
    dt = np.dtype([(lb, _PCD_TYPES[(t, s)], (c,)) if c != 1 else (lb, _PCD_TYPES[(t, s)]) for lb, t, s, c in zip(labels, types, sizes, counts)])
    if data == "binary":
        if len(buf) - pos < n * dt.itemsize:
            raise ValueError(f"{path}: {n} points of {dt.itemsize} bytes announced, {len(buf) - pos} bytes present")
        rec = np.frombuffer(buf, dtype=dt, count=n, offset=pos)
    else:
        rec = np.zeros(n, dtype=dt)
        rows = [ln.split() for ln in buf[pos:].decode("ascii", errors="replace").splitlines() if ln.strip()]
        if len(rows) < n or any(len(r) != sum(counts) for r in rows[:n]):
            raise ValueError(f"{path}: the ascii body does not hold {n} rows of {sum(counts)} values")
        col = 0
        for lb, c, t in zip(labels, counts, types):
            vals = np.array([[float(x) if t == "F" else int(x) for x in r[col:col + c]] for r in rows[:n]]).reshape(n, c)
            rec[lb] = vals if c != 1 else vals[:, 0]
            col += c
    first = {}
    for lb, nm in zip(labels, names):
        first.setdefault(nm, lb)
    xyz = np.ascontiguousarray(np.stack([rec[first[c]].astype(np.float32) for c in "xyz"], axis=1)).reshape(n, 3)
    if want_fields:
        return xyz, {nm: np.array(rec[lb]) for nm, lb in first.items() if nm != "_"}
    return xyz


# ---- edge.txt ----
def read_edges(path, names, bagname: str = ""):
    """``pgo_edges_io(io = 0)``: (edges, absent).  ``edges``: one dict(m1, m2, id1, id2, rot (3, 3), tra (3,), v6 (6,)) per line whose two sessions are
    in ``names``, with m1 <= m2 -- ``SessionEdges.push(**e)`` takes it; ``absent``: the lines kept verbatim.  A missing file reads as empty."""
    names = list(names)
    edges, absent = [], []
    if not os.path.exists(path):
        return edges, absent
    with open(path) as f:
        for raw in f:
            line = raw.rstrip("\n")
            sts = line.split()
            if not sts:
                continue
            mp = [names.index(s) if s in names else -1 for s in sts[:2]]
            if len(mp) == 2 and mp[0] != -1 and mp[1] != -1:
                id1, id2 = int(sts[2]), int(sts[3])
                v3 = np.array([float(sts[4]), float(sts[5]), float(sts[6])])
                rot = rot_from_quat(float(sts[7]), float(sts[8]), float(sts[9]), float(sts[10]))
                if mp[0] <= mp[1]:
                    edges.append(dict(m1=mp[0], m2=mp[1], id1=id1, id2=id2, rot=rot, tra=v3, v6=np.full(6, V6_EDGE)))
                else:
                    edges.append(dict(m1=mp[1], m2=mp[0], id1=id2, id2=id1, rot=rot.T.copy(), tra=-(rot.T @ v3), v6=np.full(6, V6_EDGE)))
            elif bagname not in sts[:2]:
                absent.append(line)
    return edges, absent


def write_edges(path, names, edges, absent=()):
    """``pgo_edges_io(io = 1)``: the absent lines first, then every edge group by group.  ``edges``: a ``multisession.SessionEdges`` or the list
    ``read_edges`` returns."""
    names = list(names)
    rows = []
    if hasattr(edges, "edges"):
        for e in edges.edges:
            for k in range(len(e["rots"])):
                rows.append((e["m1"], e["m2"], e["ids1"][k], e["ids2"][k], e["rots"][k], e["tras"][k]))
    else:
        rows = [(e["m1"], e["m2"], e["id1"], e["id2"], e["rot"], e["tra"]) for e in edges]
    with open(path, "w") as f:
        for line in absent:
            f.write(line + "\n")
        for m1, m2, id1, id2, rot, tra in rows:
            q = quat_from_rot(rot)
            f.write(f"{names[m1]} {names[m2]} {int(id1)} {int(id2)} " + " ".join(f"{float(v):.7g}" for v in tra) + " " + " ".join(f"{float(v):.7g}" for v in q) + "\n")


# ---- General/previous_map ----
# what strtod converts at the start of a string (no white space is left by then)
_STOD = re.compile(r"[+-]?(?:inf(?:inity)?|nan|0x(?:[0-9a-f]+\.?[0-9a-f]*|\.[0-9a-f]+)(?:p[+-]?\d+)?|(?:\d+\.?\d*|\.\d+)(?:e[+-]?\d+)?)", re.IGNORECASE)


def parse_previous_maps(text: str):
    """``previous_map_names``: (names, juds).  An entry that does not split into exactly two pieces at ``:`` ends the parse; the number is read only
    for an entry that is kept, as ``std::stod`` reads it (the longest numeric prefix); where there is none, ``ValueError``."""
    names, juds = [], []
    text = "".join(str(text).split())
    pieces = text.split(",") if text else []
    if pieces and pieces[-1] == "":
        pieces.pop()                      # getline yields nothing after a trailing comma
    for piece in pieces:
        strs = piece.split(":")
        if strs and strs[-1] == "":
            strs.pop()                    # ... nor after a trailing colon
        if len(strs) != 2:
            break                         # "previous map name wrong": the parse ends here
        if strs[0][:1] != "#":            # an empty name is a name (strs[0][0] is the terminator there, not '#')
            m = _STOD.match(strs[1])
            if m is None:
                raise ValueError(f"previous map {strs[0]!r}: {strs[1]!r} is no number")
            names.append(strs[0]); juds.append(float.fromhex(m.group(0)) if "x" in m.group(0).lower() else float(m.group(0)))
    return names, juds


# ---- a session directory ----
def save_session(path, scans, t, states, v6, min_scans: int = 100) -> bool:
    """``save_pcd`` per scan and ``save_pose``: ``scans`` is one (n_i, 3) body-frame cloud per scan.  The clouds are always written; the state file
    only for ``min_scans`` scans or more (the reference's 100), which is what the return value tells."""
    os.makedirs(path, exist_ok=True)
    for k, s in enumerate(scans):
        write_pcd(os.path.join(path, f"{k}.pcd"), s)
    return write_lidarstate(os.path.join(path, STATE_FILE), t, states, v6, min_scans)


def read_session(path):
    """(scans: list of (n_i, 3) float32, t (n,), states (n, 24), v6 (n, 6)): the state file and one ``i.pcd`` per line of it (:323-336)."""
    t, states, v6 = read_lidarstate(os.path.join(path, STATE_FILE))
    scans = [read_pcd(os.path.join(path, f"{k}.pcd")) for k in range(t.shape[0])]
    return scans, t, states, v6


def global_path(scan_poses_per_session, ids):
    """``pub_global_path``: (n, 4) float32 rows (p, session id), the sessions in the order of ``ids``, each session's scans in order."""
    rows = []
    for i in ids:
        P = np.asarray(scan_poses_per_session[i], dtype=np.float64).reshape(-1, 12)
        rows.append(np.concatenate([P[:, 9:12], np.full((P.shape[0], 1), float(i))], axis=1))
    return np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, 4), np.float32)
