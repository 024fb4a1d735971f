"""A literal Python restatement of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:708-775),
KeyFrame::SetBadFlag (src/KeyFrame.cc:492-598) with MapPoint::EraseObservation / SetBadFlag
(src/MapPoint.cc:152-212), LocalMapping::MapPointCulling (src/LocalMapping.cc:185-220) and
MapPoint::Observations() over covisibility_model.Graph, and the scenes of the culling tests.
The keyframe id stands in for KeyFrame* wherever the reference's order is a pointer order.

`maps` is a dict of the map's arrays, changed in place: kf_mp (K, cap) i32, kf_bad (K,) u8 and
mp_bad (n,) u8 -- the very arrays the graph was refreshed with --, octave (K, cap) i32
(mvKeysUn[i].octave), u_right (K, cap) f32 or None, depth (K, cap) f32 and th_depth (K,) f32
(needed unless monocular), to_be_erased (K,) u8 or None.

Deviations from the reference, shared with the device:
  * the graph's *cleaned* table is read, as by every call after a refresh: a MapPoint named at two
    indices of a row counts once in nMPs (the reference's mvpMapPoints would count it twice);
  * a candidate or an id that is bad already is skipped (the reference's lists hold none);
  * a keyframe that is both the parent and a child of the culled one (a cycle, which the
    reference's spanning tree cannot hold) is not among the children;
  * a culled keyframe whose parent is -1 (the reference dereferences NULL): its children that
    find no candidate get parent -1 and the call's status gets NO_PARENT.
g.obs is kept live: after a call the graph's cleaned table and observations equal a fresh
refresh_observations of the mutated table and flags (assert_refreshed).  Not a test module.
"""
from __future__ import annotations

import numpy as np

import covisibility_model as M

NO_PARENT = 1
TH_OBS = 3  # LocalMapping.cc:720


def _check(g: M.Graph, maps):
    assert maps["kf_bad"] is g.kf_bad and maps["mp_bad"] is g.mp_bad, "the graph must read the maps' own flag arrays"


def n_obs(g: M.Graph, p, u_right):
    """MapPoint::Observations(): nObs as AddObservation / EraseObservation keep it (MapPoint.cc:134-180)."""
    return sum(2 if (u_right is not None and u_right[k, i] >= 0) else 1 for k, i in g.obs[p].items())


def observation_counts(g: M.Graph, u_right):
    return np.array([0 if g._mp_is_bad(p) else n_obs(g, p, u_right) for p in range(len(g.obs))], np.int32)


def map_point_set_bad(g: M.Graph, maps, p):
    """MapPoint::SetBadFlag, MapPoint.cc:195-212."""
    maps["mp_bad"][p] = 1
    for k, i in g.obs[p].items():
        maps["kf_mp"][k, i] = -1  # EraseMapPointMatch
        g.clean[k, i] = -1
    g.obs[p] = {}


def erase_observation(g: M.Graph, maps, p, k):
    """MapPoint.cc:152-180.  Returns whether the point went bad."""
    if k not in g.obs[p]:
        return False
    del g.obs[p][k]
    if g._mp_is_bad(p):  # a bad MapPoint holds no observation in the reference: nothing more
        return False
    if n_obs(g, p, maps.get("u_right")) <= 2:
        map_point_set_bad(g, maps, p)
        return True
    return False


def set_bad_flag(g: M.Graph, maps, k, not_erase=None):
    """KeyFrame::SetBadFlag.  Returns (0 nothing | 1 bad now | 2 only marked, status bits, MapPoints that went bad)."""
    _check(g, maps)
    if k <= 0 or k >= len(g.clean) or g._kf_is_bad(k):  # cc:497
        return 0, 0, 0
    if not_erase is not None and not_erase[k]:  # cc:500-503
        if maps.get("to_be_erased") is not None:
            maps["to_be_erased"][k] = 1
        return 2, 0, 0
    for kf in list(g.row[k]):  # cc:506-508
        if kf != k:
            g.erase_connection(kf, k)
    new_bad = 0
    for i in range(max(0, min(int(g.kf_n[k]), g.clean.shape[1]))):  # cc:510-512; the row keeps its entries
        p = int(g.clean[k, i])
        if p >= 0:
            new_bad += erase_observation(g, maps, p, k)
    g.row[k], g.ordered[k], g.weights[k] = {}, [], []  # cc:519-520
    parent = g.parent[k]
    status = NO_PARENT if parent < 0 else 0
    children = [c for c in range(len(g.clean)) if c != k and c != parent and g.parent[c] == k and not g._kf_is_bad(c)]
    candidates = {parent}
    while children:  # cc:527-576
        best, pc, pp = -1, None, None
        for c in children:
            for kf in g.ordered[c]:
                if kf in candidates:
                    w = g.row[c].get(kf, 0)  # GetWeight
                    if w > best:
                        best, pc, pp = w, c, kf
        if pc is None:
            break
        g.parent[pc] = pp
        candidates.add(pc)
        children.remove(pc)
    for c in children:  # cc:578-584
        g.parent[c] = parent
    maps["kf_bad"][k] = 1  # cc:592
    return 1, status, new_bad


def evaluate(g: M.Graph, maps, k, monocular):
    """nMPs and nRedundantObservations of candidate k, LocalMapping.cc:722-760."""
    nmps = nred = 0
    u_right = maps.get("u_right")
    for i in range(max(0, min(int(g.kf_n[k]), g.clean.shape[1]))):
        p = int(g.clean[k, i])
        if p < 0 or g._mp_is_bad(p):
            continue
        if not monocular and (maps["depth"][k, i] > maps["th_depth"][k] or maps["depth"][k, i] < 0):
            continue
        nmps += 1
        if n_obs(g, p, u_right) > TH_OBS:
            level = int(maps["octave"][k, i])
            n = sum(1 for kf, idx in g.obs[p].items() if kf != k and int(maps["octave"][kf, idx]) <= level + 1)
            if n >= TH_OBS:
                nred += 1
    return nmps, nred


def key_frame_culling(g: M.Graph, maps, cur, monocular, not_erase=None):
    """Returns cand, cand_counts (len, 3), culled, n_new_bad_mp, status."""
    _check(g, maps)
    cand = list(g.ordered[cur])  # taken once, cc:714
    counts = np.zeros((len(cand), 3), np.int32)
    culled, new_bad, status = [], 0, 0
    for j, k in enumerate(cand):
        if k <= 0 or k >= len(g.clean) or g._kf_is_bad(k):  # cc:718
            continue
        nmps, nred = evaluate(g, maps, k, monocular)
        counts[j, :2] = nmps, nred
        if float(nred) > 0.9 * float(nmps):  # cc:768
            res, st, nb = set_bad_flag(g, maps, k, not_erase)
            counts[j, 2] = res
            status |= st
            new_bad += nb
            if res == 1:
                culled.append(k)
    return {"cand": np.array(cand, np.int32), "cand_counts": counts, "culled": np.array(culled, np.int32),
            "n_new_bad_mp": new_bad, "status": status}


def map_point_culling(g: M.Graph, maps, recent, cur_id, monocular, found, visible, first_kf, br=None):
    """LocalMapping.cc:185-220.  Returns (the kept list, how many SetBadFlags ran)."""
    _check(g, maps)
    th = 2 if monocular else 3
    kept, n = [], 0
    br = {} if br is None else br

    def hit(name):
        br[name] = br.get(name, 0) + 1

    for p in recent:
        p = int(p)
        if p < 0 or p >= len(g.obs) or g._mp_is_bad(p):
            hit("bad")
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.float32(found[p]) / np.float32(visible[p])
        if ratio < np.float32(0.25):
            map_point_set_bad(g, maps, p)
            n += 1
            hit("ratio")
        elif int(cur_id) - int(first_kf[p]) >= 2 and n_obs(g, p, maps.get("u_right")) <= th:
            map_point_set_bad(g, maps, p)
            n += 1
            hit("few_observations")
        elif int(cur_id) - int(first_kf[p]) >= 3:
            hit("old")
        else:
            kept.append(p)
            hit("kept")
    return kept, n


def assert_refreshed(g: M.Graph, maps):
    """The live state equals a fresh refresh of the mutated table and flags."""
    clean, obs, _ = M.observations(maps["kf_mp"], g.kf_n, maps["kf_bad"], len(maps["mp_bad"]))
    assert np.array_equal(clean, g.clean), np.argwhere(clean != g.clean)[:5]
    for p, (a, b) in enumerate(zip(obs, g.obs)):
        assert list(a.items()) == list(b.items()), (p, a, b)


# ---- scenes --------------------------------------------------------------------------------

class Hand:
    """A map built observation by observation.  `glue` groups of keyframes share 16 points each
    (weight >= 15: they are in each other's ordered lists); glue and link observations have
    depth -1, so that a call that is not monocular leaves them out of nMPs."""

    def __init__(self, K, cap, n_mp):
        self.K, self.cap = K, cap
        self.kf_mp = np.full((K, cap), -1, np.int32)
        self.octave = np.zeros((K, cap), np.int32)
        self.u_right = np.full((K, cap), -1.0, np.float32)
        self.depth = np.ones((K, cap), np.float32)
        self.th_depth = np.full(K, 40.0, np.float32)
        self.next = [0] * K
        self.n_mp, self.used = n_mp, 0

    def see(self, k, p, octave=0, stereo=False, depth=1.0):
        i = self.next[k]
        self.next[k] += 1
        assert i < self.cap, ("row full", k)
        self.kf_mp[k, i], self.octave[k, i], self.depth[k, i] = p, octave, depth
        self.u_right[k, i] = 100.0 if stereo else -1.0
        return i

    def point(self, *observers):
        """A new MapPoint seen by observers (k, octave[, stereo[, depth]])."""
        p = self.used
        self.used += 1
        assert p < self.n_mp
        for o in observers:
            self.see(*((o[0], p) + tuple(o[1:])))
        return p

    def link(self, a, b, n):
        """n points that only a and b see: a connection of weight n."""
        return [self.point((a, 0, False, -1.0), (b, 0, False, -1.0)) for _ in range(n)]

    def glue(self, group, n=16):
        return [self.point(*[(k, 0, False, -1.0) for k in group]) for _ in range(n)]

    def maps(self):
        return {"kf_mp": self.kf_mp, "kf_n": np.full(self.K, self.cap, np.int32), "kf_bad": np.zeros(self.K, np.uint8),
                "mp_bad": np.zeros(self.n_mp, np.uint8), "octave": self.octave, "u_right": self.u_right, "depth": self.depth,
                "th_depth": self.th_depth, "to_be_erased": np.zeros(self.K, np.uint8)}


def bounds_scene():
    """Candidates of keyframe 11 whose counts sit on every boundary of KeyFrameCulling.  Keyframes
    0 .. 11 share the glue; 8, 9, 10 are the witnesses: their observations have octave 0 and the
    candidates' octave 2, so a witness never finds three others that pass the scale test."""
    h = Hand(12, 96, 400)
    h.glue(range(12))
    W = (8, 9, 10)
    names = {}

    def redundant(k, n, lvl=2):
        return [h.point((k, lvl), *[(w, 0) for w in W]) for _ in range(n)]

    # 1: nMPs 10, nRedundant 9 -- kept (9 > 9.0 is false); the tenth has nObs 3
    redundant(1, 9)
    names["nobs3"] = h.point((1, 2), (8, 0), (9, 0))
    # 2: 10 / 10 -- culled
    redundant(2, 10)
    # 3: 20 / 18 -- kept; 4: 20 / 19 -- culled
    redundant(3, 18)
    names["scale_plus2"] = h.point((3, 0), (8, 2), (9, 2), (10, 2))          # scaleLeveli == scaleLevel + 2: fails
    names["two_of_four_pass"] = h.point((3, 0), (8, 1), (9, 1), (10, 2), (7, 3))  # four others, two pass
    redundant(4, 19)
    names["stereo_two_observers"] = h.point((4, 2, True), (8, 0, True))     # nObs 4, one other observer
    # 5: the depth filter: 3 redundant points counted, one beyond mThDepth, one below 0, one exactly at it (counted)
    redundant(5, 3)
    names["depth_far"] = h.point((5, 2, False, 41.0), *[(w, 0) for w in W])
    names["depth_negative"] = h.point((5, 2, False, -0.5), *[(w, 0) for w in W])
    names["depth_at_threshold"] = h.point((5, 2, False, 40.0), *[(w, 0) for w in W])
    names["scale_plus1"] = h.point((5, 0), (8, 1), (9, 1), (10, 1))          # == scaleLevel + 1: passes
    names["nobs4"] = h.point((5, 2), (8, 0), (9, 0), (10, 0))
    # 6: nMPs 0 (only glue, filtered by its depth): 0 > 0.0 is false
    # 7: not_erase and redundant: only marked
    redundant(7, 6)
    m = h.maps()
    m.update(cur=11, monocular=False, not_erase=np.array([0] * 7 + [1] + [0] * 4, np.uint8), names=names)
    return m


def cascade_scene():
    """Keyframe 9's candidates 1 .. 4.  Points seen by exactly {1, 2, 7, 8} make 1 and 2 redundant
    on entry; the list visits 2 first (more shared points with 9), culls it, and 1's points are
    left with two other observers: its verdict at its turn differs from the one on entry.  3 and
    4 see points with witnesses 6, 7, 8: both are culled whatever the order.  `fragile` points
    are seen by 2, 5 and 3 only (nObs 3): culling 2 makes them bad, which takes them out of 3's
    nMPs."""
    h = Hand(10, 96, 300)
    h.glue(range(10))
    h.link(9, 2, 6)
    h.link(9, 1, 4)
    h.link(9, 3, 2)
    for _ in range(12):
        h.point((1, 2), (2, 2), (7, 0), (8, 0))
    for k in (3, 4):
        for _ in range(10):
            h.point((k, 2), (6, 0), (7, 0), (8, 0))
    fragile = [h.point((2, 2), (5, 0), (3, 2)) for _ in range(1)]
    m = h.maps()
    m.update(cur=9, monocular=False, not_erase=None, names={"fragile": fragile})
    return m


TREE = dict(A=1, B=2, C1=3, C2=4, C3=5, C4=6, C5=7, C6=8, C7=9, cur=10)


def tree_scene():
    """Re-parenting.  B's parent is A; C1 .. C7 are B's children (their heaviest connection).
    Round 1 (candidates {A}): C1 wins with 24.  Round 2: C2 through the promoted C1 (30) beats
    everything through A.  Then C5 and C6 tie at 22 through A: the lower id goes first, and C6
    then prefers C5 (28) to A.  C7 holds C5 and C6 at 25 each: the earlier list position (the
    higher id) wins.  C3 goes to A (18); C4 knows only B: it is handed to the grandparent A.
    The redundant points make B a cull candidate of `cur`."""
    t = TREE
    h = Hand(14, 512, 1200)
    A, B = t["A"], t["B"]
    h.link(0, A, 60)
    h.link(A, B, 50)
    for c in ("C1", "C2", "C3", "C4", "C5", "C6", "C7"):
        h.link(t[c], B, 45)
    h.link(t["C1"], A, 24)
    h.link(t["C2"], A, 16)
    h.link(t["C2"], t["C1"], 30)
    h.link(t["C3"], A, 18)
    h.link(t["C5"], A, 22)
    h.link(t["C6"], A, 22)
    h.link(t["C6"], t["C5"], 28)
    h.link(t["C7"], t["C5"], 25)
    h.link(t["C7"], t["C6"], 25)
    h.link(t["cur"], B, 17)
    h.link(t["cur"], 11, 20)
    for _ in range(10):  # B's only counted points: all redundant
        h.point((B, 2), (11, 0), (12, 0), (13, 0))
    m = h.maps()
    m.update(cur=t["cur"], monocular=False, not_erase=None, names={})
    return m


LATE = dict(P=1, B=2, C=3, Cp=4, X=5)


def late_scene():
    """A child whose ordered list gains its entries below 15 from an earlier cull.  Stage 1: C
    shares 40 points with B (its parent), 20 with X, 9 with C' and none with P; C' shares 20 with
    P and 41 with B.  Stage 2 (the table is mutated, C alone is updated): C lost B's points, so
    its row no longer holds B and its list is [X] -- thresholded.  SetBadFlag(B) alone: C finds
    no candidate and is handed to P.  After SetBadFlag(X), whose EraseConnection re-orders C's
    whole row, C's list holds C' (9): C follows the promoted C'."""
    t = LATE
    h = Hand(8, 256, 600)
    h.link(0, t["P"], 60)
    h.link(t["P"], t["B"], 50)
    cb = h.link(t["C"], t["B"], 40)
    h.link(t["C"], t["X"], 20)
    h.link(t["C"], t["Cp"], 9)
    h.link(t["Cp"], t["B"], 41)
    h.link(t["Cp"], t["P"], 20)
    h.link(t["X"], 6, 30)
    h.link(6, 7, 35)
    m = h.maps()
    table0 = m["kf_mp"].copy()
    sel = np.isin(m["kf_mp"][t["C"]], cb)
    m["kf_mp"][t["C"], sel] = -1
    m.update(cur=t["C"], monocular=True, not_erase=None, names={}, kf_mp0=table0, update_ids=[t["C"]])
    return m


def band_scene(seed=11, **kw):
    """covisibility_model.scene with octaves, mvuRight and depths drawn at random, nothing bad on
    entry but the scene's bad MapPoints, and keyframes 8 and 9 at octave 3, so that every other
    observer passes the scale test against them and a call from keyframe 10 culls."""
    kf_mp, kf_n, kf_bad, mp_bad = M.scene(seed, bad_kfs=(), **kw)
    rng = np.random.default_rng(seed + 100)
    K, cap = kf_mp.shape
    m = {"kf_mp": kf_mp, "kf_n": kf_n, "kf_bad": kf_bad, "mp_bad": mp_bad,
         "octave": rng.integers(0, 4, (K, cap)).astype(np.int32),
         "u_right": np.where(rng.random((K, cap)) < 0.5, 50.0, -1.0).astype(np.float32),
         "depth": rng.uniform(-2, 60, (K, cap)).astype(np.float32), "th_depth": np.full(K, 35.0, np.float32),
         "to_be_erased": np.zeros(K, np.uint8)}
    m["octave"][8:10] = 3  # every other observer passes the scale test against them
    m.update(cur=10, monocular=False, not_erase=None, names={})
    return m


def big_scene():
    """cap = 1100, K = 8: a row needs the strided loop, points have observers at indices >= 1024.
    Keyframes 1 .. 7 see the same 1060 points at shifted indices; keyframe 0 a few of them."""
    K, cap, n = 8, 1100, 2600
    rng = np.random.default_rng(5)
    kf_mp = np.full((K, cap), -1, np.int32)
    for k in range(1, K):
        ids = np.arange(1060) if k < 6 else rng.permutation(1300)[:1060]
        kf_mp[k, 30:1090] = np.roll(ids, 37 * k)
    kf_mp[0, :40] = np.arange(40)
    m = {"kf_mp": kf_mp, "kf_n": np.full(K, cap, np.int32), "kf_bad": np.zeros(K, np.uint8), "mp_bad": np.zeros(n, np.uint8),
         "octave": rng.integers(0, 3, (K, cap)).astype(np.int32),
         "u_right": np.where(rng.random((K, cap)) < 0.3, 50.0, -1.0).astype(np.float32),
         "depth": rng.uniform(-1, 50, (K, cap)).astype(np.float32), "th_depth": np.full(K, 45.0, np.float32),
         "to_be_erased": np.zeros(K, np.uint8)}
    m.update(cur=7, monocular=False, not_erase=None, names={})
    return m


SCENES = {"bounds": bounds_scene, "cascade": cascade_scene, "tree": tree_scene, "late": late_scene, "band": band_scene}


def copy_maps(m):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in m.items()}


def build_graph(m, max_conn=64):
    """The model graph of a scene: every keyframe connected in id order on kf_mp0 (or kf_mp), then,
    for a two-stage scene, refreshed on kf_mp with update_ids connected again.  Reads m's own
    flag arrays."""
    K = len(m["kf_mp"])
    g = M.Graph(K, max_conn)
    g.refresh_observations(m.get("kf_mp0", m["kf_mp"]), m["kf_n"], m["kf_bad"], m["mp_bad"])
    for k in range(K):
        g.update_connections(k)
    if "kf_mp0" in m:
        g.refresh_observations(m["kf_mp"], m["kf_n"], m["kf_bad"], m["mp_bad"])
        for k in m["update_ids"]:
            g.update_connections(k)
    return g


def recent_case(m, g, seed, n_recent):
    """mlpRecentAddedMapPoints over a scene's MapPoints with found / visible / first keyframe drawn
    so that every branch of MapPointCulling fires; cur_id = 10."""
    rng = np.random.default_rng(seed)
    n = len(m["mp_bad"])
    recent = rng.permutation(n)[:n_recent].astype(np.int32)
    visible = rng.integers(0, 9, n).astype(np.int32)
    found = np.minimum(rng.integers(0, 9, n), np.maximum(visible, 1)).astype(np.int32)
    first = rng.integers(6, 11, n).astype(np.int32)
    visible[recent[0]], found[recent[0]] = 0, 0           # 0 / 0: NaN does not compare less
    visible[recent[1]], found[recent[1]] = 8, 2           # exactly 0.25: not below
    visible[recent[2]], found[recent[2]] = 0, 3           # inf
    return recent, found, visible, first
