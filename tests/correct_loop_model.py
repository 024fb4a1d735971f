"""A literal Python restatement of LoopClosing::CorrectLoop's Sim3 propagation and first map-point
correction (src/LoopClosing.cc:482-571), of its LoopConnections (cc:595-618), of
MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:386-439) in float64, and of the inputs that the
package's essential_graph_edges takes (Optimizer.cc:913-1089, 1125-1133), on
covisibility_model.Graph: sequential, in the reference's order, with dict and set semantics.  The
keyframe id stands in for KeyFrame* wherever the reference iterates a map or a set of pointers.
Beside each sequential form stands the parallel form that the device runs (the ownership rule, the
interleaved-pose rule, the snapshot form of LoopConnections); tests/test_correct_loop_model.py
shows them equal.  Not a test module.

Arithmetic: float inputs are widened to double, everything after is double, the outputs are
rounded to float where the reference stores a float.  `Variant` switches
single steps to the reference's own float arithmetic or to another composition; the differences
are the scale of legitimate disagreement (tests/correct_loop_spread.py).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np

import covisibility_model as CM
import essential_graph_model as E
from pose_opt_model import quat_from_matrix

REF_NOT_OBSERVER, BAD_INDEX = 1, 2
ASM_CAPACITY, ASM_BAD_KEYFRAME = 1, 2


@dataclass(frozen=True)
class Variant:
    tic: str = "double"      # Tiw * Twc: "double", or "float" (the reference's cv::Mat product)
    centre: str = "double"   # GetCameraCenter(): "double", or "float" (KeyFrame::SetPose)
    norm: str = "double"     # cv::norm and the division: "double", or "float"
    compose: str = "quat"    # Sim3(Ric, tic, 1) * Scw: g2o's quaternion product, or by matrices


BASE = Variant()
VARIANTS = [BASE, Variant(tic="float"), Variant(centre="float"), Variant(norm="float"), Variant(compose="matrix")]
FLOAT_FIELDS = ("corr_S", "poses", "mp_pos", "normal", "max_distance", "min_distance")


# ---- small arithmetic, operation by operation as csrc/orbx_correctloop.hip ------------------------

_CENTRES: dict = {}


def centre(T12, v: Variant = BASE):
    """GetCameraCenter() = -Rcw^T tcw of a pose's rows 0..2 (kept per pose: the walks ask for the
    same few keyframes again and again)."""
    key = (np.asarray(T12, np.float32).tobytes(), v.centre)
    if key not in _CENTRES:
        if len(_CENTRES) > 4096:
            _CENTRES.clear()
        _CENTRES[key] = _centre(T12, v)
    return _CENTRES[key]


def _centre(T12, v: Variant):
    if v.centre == "float":
        T = np.asarray(T12, np.float32).reshape(3, 4)
        return (-(T[:, :3].T @ T[:, 3])).astype(np.float64)
    T = np.asarray(T12, np.float32).astype(np.float64).reshape(3, 4)
    return np.array([-((T[0, c] * T[0, 3] + T[1, c] * T[1, 3]) + T[2, c] * T[2, 3]) for c in range(3)])


def _unit(d, v: Variant):
    if v.norm == "float":
        f = d.astype(np.float32)
        n = np.sqrt(np.float32(np.float32(f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]))
        return (f / n).astype(np.float64), float(n)
    n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return d / n, n


def normal_and_depth(g: CM.Graph, p, P, pose_of, ref, octave, scale, v: Variant = BASE):
    """MapPoint.cc:400-437 of point p at position P (float64); pose_of(kf) gives kf's pose.
    Returns None for a point without observers or with a reference outside the keyframes, else
    (normal, max_distance, min_distance, status) in float64."""
    obs = g.obs[p]
    if not obs:
        return None
    n = np.zeros(3)
    for kf in obs:  # ascending keyframe id
        u, _ = _unit(P - centre(pose_of(kf), v), v)
        n = n + u
    status = 0
    idx = obs.get(ref)
    if idx is None:  # observations[pRefKF] inserts 0
        idx, status = 0, REF_NOT_OBSERVER
    _, dist = _unit(P - centre(pose_of(ref), v), v)
    nl = len(scale)
    level = min(max(int(octave[ref, idx]), 0), nl - 1)
    dmax = dist * float(scale[level])
    return n / float(len(obs)), dmax, dmax / float(scale[nl - 1]), status


def update_normal_and_depth(g: CM.Graph, st, ids=None, v: Variant = BASE):
    """The call over a list of ids (None: every point) on the state st (poses, mp_pos, mp_ref_kf,
    octave, scale, normal, max_distance, min_distance): returns (normal, max_distance,
    min_distance) as float32 copies, and the status."""
    normal, dmax, dmin = st["normal"].copy(), st["max_distance"].copy(), st["min_distance"].copy()
    n_mp, nk = len(g.obs), len(st["poses"])
    status = 0
    for p in (range(n_mp) if ids is None else ids):
        p = int(p)
        if p < 0 or p >= n_mp:
            status |= BAD_INDEX
            continue
        if g._mp_is_bad(p) or not g.obs[p]:
            continue
        ref = int(st["mp_ref_kf"][p])
        if ref < 0 or ref >= nk:
            status |= BAD_INDEX
            continue
        r = normal_and_depth(g, p, st["mp_pos"][p].astype(np.float64), lambda kf: st["poses"][kf], ref, st["octave"],
                             st["scale"], v)
        normal[p], dmax[p], dmin[p] = r[0], r[1], r[2]
        status |= r[3]
    return normal, dmax, dmin, status


def sim3_of(R, t, s=1.0):
    """g2o::Sim3(R, t, s): Quaterniond(R), not normalised."""
    return np.concatenate([quat_from_matrix(np.asarray(R, np.float64)), np.asarray(t, np.float64), [float(s)]])


def compose_scw(R, t, s, Tmw):
    """LoopClosing.cc:359-362 from OptimizeSim3's float R / t / s and the matched keyframe's pose."""
    Scm = sim3_of(np.asarray(R, np.float32).astype(np.float64).reshape(3, 3), np.asarray(t, np.float32).astype(np.float64),
                  float(np.float32(s)))
    return E.s_mul(Scm, E.s_from_tcw(Tmw))


def _sic(Tiw, Tcw, v: Variant):
    """Sim3(Ric, tic, 1) with Tic = Tiw * Twc (cc:508-511)."""
    if v.tic == "float":
        Tc = np.asarray(Tcw, np.float32).reshape(3, 4)
        Twc = np.eye(4, dtype=np.float32)
        Twc[:3, :3] = Tc[:, :3].T
        Twc[:3, 3] = -(Tc[:, :3].T @ Tc[:, 3])
        Ti = np.eye(4, dtype=np.float32)
        Ti[:3] = np.asarray(Tiw, np.float32).reshape(3, 4)
        Tic = (Ti @ Twc).astype(np.float64)
        return sim3_of(Tic[:3, :3], Tic[:3, 3])
    Ti = np.asarray(Tiw, np.float32).astype(np.float64).reshape(3, 4)
    Tc = np.asarray(Tcw, np.float32).astype(np.float64).reshape(3, 4)
    Ow = centre(Tcw)
    Twc = [[Tc[c, r] for c in range(3)] + [Ow[r]] for r in range(3)]
    R = np.array([[(Ti[r, 0] * Twc[0][c] + Ti[r, 1] * Twc[1][c]) + Ti[r, 2] * Twc[2][c] for c in range(3)] for r in range(3)])
    t = np.array([((Ti[r, 0] * Twc[0][3] + Ti[r, 1] * Twc[1][3]) + Ti[r, 2] * Twc[2][3]) + Ti[r, 3] for r in range(3)])
    return sim3_of(R, t)


def _mul(a, b, v: Variant):
    if v.compose == "matrix":
        Ra, Rb = np.array(E.rot_matrix(a)), np.array(E.rot_matrix(b))
        return sim3_of(Ra @ Rb, a[7] * (Ra @ b[4:7]) + a[4:7], a[7] * b[7])
    return E.s_mul(a, b)


def _to_tcw(S):
    return E.s_to_tcw64(np.asarray(S)[:, None])[0].astype(np.float32)


# ---- LoopClosing.cc:482-571 -----------------------------------------------------------------------

def propagate(g: CM.Graph, st, cur, Scw, v: Variant = BASE, parallel=False):
    """Mutates the graph g; returns a new state (poses, mp_pos, mp_corrected_by_kf, mp_corrected_ref,
    normal, max_distance, min_distance changed) plus conn, corr_S (n_conn, 8), kf_corr (K,),
    kf_Tcw_nc (n_conn, 12), status.  parallel: the device's rules instead of the sequential walk."""
    st = {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in st.items()}
    poses, nk = st["poses"], len(st["poses"])
    T_in = poses.copy()
    g.update_connections(cur)  # cc:482
    conn = [k for k in g.ordered[cur] if k != cur and k < nk and not g._kf_is_bad(k)] + [cur]  # cc:488-489
    Scw = np.asarray(Scw, np.float64)
    corr, nc, Tc = {}, {}, {}
    for i in conn:  # cc:501-523
        nc[i] = E.s_from_tcw(T_in[i])
        corr[i] = Scw if i == cur else _mul(_sic(T_in[i], T_in[cur], v), Scw, v)
        Tc[i] = _to_tcw(corr[i])  # cc:558-564
    kf_corr = np.full(g.K, -1, np.int32)
    for j, i in enumerate(conn):
        kf_corr[i] = j
    status = 0
    by_in = st["mp_corrected_by_kf"].copy()

    def correct(i, p, pose_of):
        nonlocal status
        P = st["mp_pos"][p].astype(np.float64)
        Pc = E.s_map(E.s_inv(corr[i]), E.s_map(nc[i], P)).astype(np.float32)  # cc:547-550
        st["mp_pos"][p] = Pc
        st["mp_corrected_by_kf"][p] = cur
        st["mp_corrected_ref"][p] = i
        ref = int(st["mp_ref_kf"][p])
        if ref < 0 or ref >= nk:
            status |= BAD_INDEX
            return
        r = normal_and_depth(g, p, Pc.astype(np.float64), pose_of, ref, st["octave"], st["scale"], v)  # cc:554
        if r is not None:
            st["normal"][p], st["max_distance"][p], st["min_distance"][p] = r[0], r[1], r[2]
            status |= r[3]

    def row(i):
        if g._kf_is_bad(i):  # only cur can be: outside the reference
            return []
        return [int(p) for p in g.clean[i] if p >= 0 and not g._mp_is_bad(int(p))]

    if not parallel:
        for i in sorted(corr):  # cc:526: the map's key order
            for p in row(i):
                if st["mp_corrected_by_kf"][p] == cur:  # cc:541
                    continue
                correct(i, p, lambda kf: poses[kf])
            poses[i] = Tc[i]  # cc:566
            g.update_connections(i)  # cc:570
    else:
        for i in conn:
            for p in row(i):
                if by_in[p] == cur:
                    continue
                owner = next((kf for kf in g.obs[p] if kf_corr[kf] >= 0), -1)
                if owner != i:
                    continue
                correct(i, p, lambda kf, i=i: Tc[kf] if kf_corr[kf] >= 0 and kf < i else T_in[kf])
        for i in conn:
            poses[i] = Tc[i]
        for i in conn:
            g.update_connections(i)
    st.update(conn=np.array(conn, np.int32), corr_S=np.array([corr[i] for i in conn]), kf_corr=kf_corr,
              kf_Tcw_nc=np.array([T_in[i] for i in conn], np.float32), status=status)
    return st


# ---- LoopClosing.cc:595-618 and the tables of OptimizeEssentialGraph ------------------------------

def loop_connections(g: CM.Graph, conn, snapshot=False):
    """Mutates g (UpdateConnections of the members).  Returns the ordered list that
    essential_graph_edges takes: [(member, [(kf, GetWeight), ...]), ...], members and sets in
    ascending id.  snapshot: the device's form -- the members' ordered lists and rows are taken
    before any update; vpPreviousNeighbors of member i is its ordered list, or its whole row when
    the update of a member before it in the list re-ordered it."""
    conn = [int(k) for k in conn]
    members = set(conn)
    lc = {}
    if snapshot:
        prev = {i: list(g.ordered[i]) for i in conn}
        prow = {i: dict(g.row[i]) for i in conn}
        for i in conn:
            g.update_connections(i)
        pos = {i: j for j, i in enumerate(conn)}

        def kmax(j):  # pKFmax of j's fresh row when no entry reaches the threshold, else None
            if not g.row[j] or max(g.row[j].values()) >= CM.TH:
                return None
            best = max(g.row[j].values())
            return min(k for k, w in g.row[j].items() if w == best)

        for i in conn:
            # an earlier member's AddConnection (KeyFrame.cc:139-153) re-ordered i's whole row
            resorted = any(pos[j] < pos[i] and (w >= CM.TH or kmax(j) == i) and prow[i].get(j, 0) != w
                           for j, w in g.row[i].items() if j in members)
            lc[i] = set(g.row[i]) - set(prow[i] if resorted else prev[i]) - members
    else:
        for i in conn:  # cc:598-617
            prev = list(g.ordered[i])
            g.update_connections(i)
            s = set(g.row[i])
            for k in prev:
                s.discard(k)
            for k in conn:
                s.discard(k)
            lc[i] = s
    return [(i, [(k, g.row[i].get(k, 0)) for k in sorted(lc[i])]) for i in sorted(lc)]


def assemble(g: CM.Graph, st, cur, loop, loop_edges, min_feat=100, snapshot=False):
    """The tables of the device assembly from the state that propagate() returned (after the
    caller's fusion and refresh): mutates g.  loop_edges: {kf: [ids ascending]}."""
    from orbslam2commentedbyxcm_amd.optimizer import essential_graph_edges, essential_graph_envelope
    nk = len(st["poses"])
    lc = loop_connections(g, st["conn"], snapshot)
    ids = [k for k in range(nk) if not g._kf_is_bad(k)]
    kf_row = np.full(g.K, -1, np.int32)
    kf_row[ids] = np.arange(len(ids), dtype=np.int32)
    parent = [g.parent[k] for k in ids]
    children = [[c for c in ids if g.parent[c] == k] for k in ids]
    loops = [list(loop_edges.get(k, [])) for k in ids]
    covis = [list(zip(g.ordered[k], g.weights[k])) for k in ids]
    edge_v, edge_kind = essential_graph_edges(ids, parent, children, loops, covis, lc, cur, loop, min_feat)
    n = len(st["mp_pos"])
    pt_ref = np.full(n, -1, np.int32)
    for p in range(n):
        if g._mp_is_bad(p):
            continue
        ref = int(st["mp_corrected_ref"][p] if st["mp_corrected_by_kf"][p] == cur else st["mp_ref_kf"][p])  # cc:1127-1133
        pt_ref[p] = kf_row[ref] if 0 <= ref < nk else -1
    kf_corr_rows = st["kf_corr"][ids]
    rows = np.array([st["kf_Tcw_nc"][st["kf_corr"][k]] if st["kf_corr"][k] >= 0 else st["poses"][k] for k in ids],
                    np.float32).reshape(-1, 12)
    lc_off = np.cumsum([0] + [len(c) for _, c in lc]).astype(np.int32)
    return {"lc": lc, "lc_member": np.array([i for i, _ in lc], np.int32), "lc_off": lc_off,
            "lc_kf": np.array([k for _, c in lc for k, _ in c], np.int32),
            "lc_w": np.array([w for _, c in lc for _, w in c], np.int32),
            "kf_ids": np.array(ids, np.int32), "kf_row": kf_row, "loop_row": int(kf_row[loop]), "kf_corr_rows": kf_corr_rows,
            "kf_Tcw_rows": rows, "edge_v": edge_v, "edge_kind": edge_kind, "pt_ref": pt_ref,
            "env_blocks": essential_graph_envelope(len(ids), int(kf_row[loop]), edge_v),
            "inputs": dict(ids=ids, parent=parent, children=children, loops=loops, covis=covis)}


# ---- scenes -----------------------------------------------------------------------------------------

def _rot(rng, deg):
    a = rng.normal(size=3)
    a = a / np.linalg.norm(a) * np.deg2rad(deg) * rng.uniform(0.3, 1.0)
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def with_geometry(kf_mp, kf_n, kf_bad, mp_bad, seed, poses=None, mp_pos=None, octave=None, nlevels=8):
    """The map state around an integer scene: poses (rotations of a few degrees along a path),
    points in front of them, octaves, mpRefKF = the first observer (a few points get a keyframe
    that does not observe them, one gets the last observer), nothing corrected yet."""
    rng = np.random.default_rng(seed)
    K, cap = np.asarray(kf_mp).shape
    n = len(mp_bad)
    if poses is None:
        poses = np.zeros((K, 12), np.float32)
        for k in range(K):
            R = _rot(rng, 8.0)
            c = np.array([0.8 * k, 0.0, 0.0]) + rng.normal(0, 0.05, 3)
            poses[k] = np.hstack([R, (-R @ c)[:, None]]).reshape(-1)
    if mp_pos is None:
        mp_pos = np.stack([rng.uniform(-3, 0.8 * K + 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], 1).astype(np.float32)
    if octave is None:
        octave = rng.integers(0, nlevels, (K, cap)).astype(np.int32)
    octave = np.array(octave, np.int32)
    octave[0, 0], octave[K - 1, 0] = -3, nlevels + 5  # clamped
    _, obs, _ = CM.observations(kf_mp, kf_n, kf_bad, n)
    ref = np.zeros(n, np.int32)
    for p in range(n):
        ref[p] = next(iter(obs[p])) if obs[p] else int(rng.integers(0, K))
    seen = [p for p in range(n) if len(obs[p]) >= 2]
    for p in seen[::17]:  # a reference keyframe that is not an observer
        ref[p] = next(k for k in range(K) if k not in obs[p])
    for p in seen[3::19]:
        ref[p] = list(obs[p])[-1]
    return {"poses": np.asarray(poses, np.float32).reshape(K, 12).copy(), "mp_pos": np.asarray(mp_pos, np.float32).copy(),
            "octave": octave, "scale": (1.2 ** np.arange(nlevels)).astype(np.float32), "mp_ref_kf": ref,
            "mp_corrected_by_kf": np.full(n, -1, np.int32), "mp_corrected_ref": np.full(n, -1, np.int32),
            "normal": np.zeros((n, 3), np.float32), "max_distance": np.zeros(n, np.float32),
            "min_distance": np.zeros(n, np.float32)}


def drift_scw(st, cur, seed, scale=1.04):
    """mg2oScw: the current keyframe's Sim3 moved by a few degrees, some centimetres and a scale."""
    rng = np.random.default_rng(seed)
    T = st["poses"][cur].astype(np.float64).reshape(3, 4)
    R = _rot(rng, 4.0) @ T[:, :3]
    return sim3_of(R, scale * (T[:, 3] + rng.normal(0, 0.2, 3)), scale)


def fuse(kf_mp, kf_n, takers, donors, counts, seed=0):
    """The caller's fusion as a table edit: taker t gets counts[(t, d)] of donor d's points that it
    does not hold yet, into free slots below kf_n[t]."""
    rng = np.random.default_rng(seed)
    out = np.array(kf_mp, np.int32, copy=True)
    for t in takers:
        for d in donors:
            c = counts[(t, d)] if isinstance(counts, dict) else counts
            have = set(out[t][out[t] >= 0].tolist())
            cand = [int(p) for p in out[d][:kf_n[d]] if p >= 0 and int(p) not in have]
            cand = sorted(set(cand))
            pick = [cand[i] for i in rng.permutation(len(cand))[:c]]
            free = [i for i in range(int(kf_n[t])) if out[t, i] < 0]
            assert len(pick) == c and len(free) >= c, (t, d, len(pick), len(free))
            for i, p in zip(free, pick):
                out[t, i] = p
    return out


def hand_scene():
    """Ten keyframes built from blocks of shared points so that every boundary of the issue is
    reached (tests/test_correct_loop_model.py asserts each): loop side 0-3, keyframe 4 bad, current
    side 5-8 (cur = 8, loop = 1), keyframe 9 alone.  Returns a dict with kf_mp (before the fusion),
    kf_mp_fused, kf_n, kf_bad, mp_bad, cur, loop, loop_edges."""
    K, cap = 10, 512
    rows = [[] for _ in range(K)]
    n = 0

    def block(kfs, count):
        nonlocal n
        ids = list(range(n, n + count))
        n += count
        for k in kfs:
            rows[k].extend(ids)
        return ids

    block((0, 1), 120)
    block((1, 2), 100)   # a covisibility edge at exactly min_feat
    block((2, 3), 120)
    block((0, 3), 99)    # and one just below, not a spanning-tree edge
    block((0, 2), 101)   # a covisible that is a loop edge
    block((3, 5), 30)
    block((3, 4), 25)    # the bad keyframe's row counts for nobody
    block((4, 5), 25)
    block((5, 6), 110)   # 5's parent is 6: a covisible of 6 that is its child
    block((6, 7), 105)   # a covisible that is the parent
    block((7, 8), 130)   # held by two members: the lower id owns them
    block((5, 7), 20)
    block((6, 8), 40)
    block((5, 8), 16)
    solo1 = block((1,), 130)
    solo2 = block((2,), 110)
    block((8,), 12)
    block((9,), 20)      # a keyframe with no edge at all
    kf_mp = np.full((K, cap), -1, np.int32)
    kf_n = np.full(K, cap, np.int32)
    rng = np.random.default_rng(5)
    for k in range(K):
        slots = np.sort(rng.permutation(cap - 8)[:len(rows[k])])  # NULL entries in between
        kf_mp[k, slots] = rows[k]
    kf_bad = np.zeros(K, np.uint8)
    kf_bad[4] = 1
    mp_bad = np.zeros(n, np.uint8)
    mp_bad[[rows[8][3], rows[7][140], rows[1][7]]] = 1
    fused = kf_mp.copy()

    def give(t, pts):
        free = [i for i in range(cap) if fused[t, i] < 0]
        for i, p in zip(free, pts):
            fused[t, i] = p

    give(8, solo1[:60])    # the cur - loop pair below min_feat
    give(8, solo2[:100])   # a LoopConnections pair at exactly min_feat
    give(7, solo1[:120])   # inserted as kind 0: skipped in 7's covisibility walk
    give(7, solo2[:99])    # and one just below
    return {"kf_mp": kf_mp, "kf_mp_fused": fused, "kf_n": kf_n, "kf_bad": kf_bad, "mp_bad": mp_bad, "cur": 8, "loop": 1,
            "loop_edges": {0: [2], 2: [0]}, "max_conn": 16, "min_feat": 100, "already": [rows[8][0], rows[8][150]]}


def band_scene(name):
    """The two random scenes of the GPU tests with a fusion that gives the current side points of
    the loop side."""
    if name == "geo10":
        s = CM.geometric_scene(21)
        base = dict(kf_mp=s["kf_mp"], kf_n=s["kf_n"], kf_bad=s["kf_bad"], mp_bad=s["mp_bad"], cur=8, loop=1, max_conn=16,
                    min_feat=5, loop_edges={3: [0], 0: [3]}, takers=[8, 7], donors=[0, 1], count=5)
        base["geometry"] = dict(poses=s["poses"], mp_pos=s["mp_pos"], octave=s["octave"])
    else:
        kf_mp, kf_n, kf_bad, mp_bad = CM.scene(31)
        base = dict(kf_mp=kf_mp, kf_n=kf_n, kf_bad=kf_bad, mp_bad=mp_bad, cur=19, loop=2, max_conn=32, min_feat=10,
                    loop_edges={10: [1, 3], 1: [10], 3: [10]}, takers=[19, 18, 17], donors=[1, 2, 3], count=10, geometry={})
    km = np.array(base["kf_mp"], copy=True)
    free_rows = base["takers"]
    for t in free_rows:  # room for the fusion
        have = np.flatnonzero(km[t] >= 0)
        free = int(base["kf_n"][t]) - len(have)
        km[t, have[:max(0, len(base["donors"]) * base["count"] - free)]] = -1
    base["kf_mp"] = km
    # the caller's seam: points gained by the fusion, and points lost (Replace) by covisibility_model.mutate
    fused = fuse(km, base["kf_n"], base["takers"], base["donors"], base["count"], seed=3)
    base["kf_mp_fused"] = CM.mutate(fused, base["donors"], np.random.default_rng(4), drop=3)
    base["already"] = [int(p) for p in km[base["cur"]][km[base["cur"]] >= 0][:2]]
    return base


SCENES = ("hand", "geo10", "band24")


def scene(name):
    """(scene dict, initial state) of a named scene; the state's mnCorrectedByKF marks the scene's
    `already` points as corrected by cur."""
    sc = hand_scene() if name == "hand" else band_scene(name)
    st = with_geometry(sc["kf_mp"], sc["kf_n"], sc["kf_bad"], sc["mp_bad"], seed=len(name) * 7,
                       **sc.get("geometry", {}))
    st["mp_corrected_by_kf"][sc["already"]] = sc["cur"]
    st["mp_corrected_ref"][sc["already"]] = sc["loop"]  # a value that no owner writes
    sc["Scw"] = drift_scw(st, sc["cur"], seed=9)
    return sc, st


def graph_of(sc, fused=False):
    """The model graph after UpdateConnections of every keyframe in id order on the scene's table."""
    K = len(sc["kf_n"])
    g = CM.Graph(K, sc["max_conn"])
    g.refresh_observations(sc["kf_mp_fused"] if fused else sc["kf_mp"], sc["kf_n"], sc["kf_bad"], sc["mp_bad"])
    for k in range(K):
        g.update_connections(k)
    return g


def run_propagate(name, v: Variant = BASE, parallel=False):
    """The propagation in the model: (scene, state after it, graph after it)."""
    sc, st = scene(name)
    g = graph_of(sc)
    return sc, propagate(g, st, sc["cur"], sc["Scw"], v, parallel), g


def run(name, v: Variant = BASE, parallel=False, snapshot=False):
    """The whole chain in the model: propagate, fusion + refresh, assemble.  Returns (scene, state
    after the propagation, assembly, graph, the graph as the propagation left it)."""
    sc, out, g = run_propagate(name, v, parallel)
    g_after = copy.deepcopy(g)
    g.refresh_observations(sc["kf_mp_fused"], sc["kf_n"], sc["kf_bad"], sc["mp_bad"])
    asm = assemble(g, out, sc["cur"], sc["loop"], sc["loop_edges"], sc["min_feat"], snapshot)
    return sc, out, asm, g, g_after


def tolerance(spread, value):
    """8 x the measured spread, floor 2 float32 ulps of the entry (the project's rule)."""
    return np.maximum(8.0 * spread, 2.0 * np.spacing(np.abs(np.asarray(value, np.float32))).astype(np.float64))


def spread(name):
    """Per float field, the largest entry difference between the variants on a scene."""
    base = run_propagate(name)[1]
    out = {k: 0.0 for k in FLOAT_FIELDS}
    for v in VARIANTS[1:]:
        r = run_propagate(name, v)[1]
        for k in FLOAT_FIELDS:
            out[k] = max(out[k], float(np.max(np.abs(r[k].astype(np.float64) - base[k].astype(np.float64)), initial=0.0)))
    return out
