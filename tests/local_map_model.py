"""A literal Python restatement of Tracking::UpdateLocalMap (UpdateLocalKeyFrames and
UpdateLocalPoints, src/Tracking.cc:1342-1500) and of TrackLocalMap's tally (cc:1047-1081) over
covisibility_model.Graph, with the batch layout of orbx_update_local_map_device.  A map or set of
KeyFrame* iterates in keyframe-id order.  Every branch counts how often it fires (`br`).  Not a
test module.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

import covisibility_model as M

CAPACITY, EMPTY = 1, 2


def children_of(g: M.Graph, parent, k):
    """mspChildrens of k: the keyframes that are not bad and have k as their parent, ascending."""
    return [c for c in range(g.K) if int(parent[c]) == k and not g._kf_is_bad(c)]


def update_local_keyframes(g: M.Graph, row, n, parent, old_list, br: Counter, parent_break=True):
    """cc:1391-1500 for one frame.  Returns (mvpMapPoints, mvpLocalKeyFrames, pKFmax or None,
    whether the counter was empty)."""
    n_mp, cap = len(g.obs), len(row)
    fmp = np.array(row, np.int32, copy=True)
    counter, voted = {}, set()
    for i in range(max(0, min(int(n), cap))):  # cc:1393-1408
        p = int(fmp[i])
        if p < 0 or p >= n_mp:
            continue
        if g._mp_is_bad(p):
            fmp[i] = -1
            br["bad_mappoint_nulled"] += 1
            continue
        if p in voted:
            br["duplicate_votes_twice"] += 1
        voted.add(p)
        for kf in g.obs[p]:
            counter[kf] = counter.get(kf, 0) + 1
    if not counter:  # cc:1411
        br["empty_counter"] += 1
        return fmp, list(old_list), None, True
    nmax, kfmax = 0, None
    local, mark = [], set()
    for kf, w in sorted(counter.items()):  # cc:1423-1442
        if g._kf_is_bad(kf):
            br["voted_keyframe_bad"] += 1
            continue
        if w > nmax:
            nmax, kfmax = w, kf
        local.append(kf)
        mark.add(kf)
    if sum(1 for kf in local if counter[kf] == nmax) > 1:
        br["tie_for_maximum"] += 1
    end = len(local)  # itEndKF is taken before the loop
    for e in range(end):  # cc:1445-1493
        if len(local) > 80:
            br["stop_80_before_first" if e == 0 else "stop_80_during_walk"] += 1
            break
        k = local[e]
        neighs = g.best_covisibles(k, 10)
        taken = False
        for nb in neighs:
            if g._kf_is_bad(nb):
                br["bad_neighbour_skipped"] += 1
                continue
            if nb not in mark:
                local.append(nb)
                mark.add(nb)
                taken = True
                break
        if not taken and any(not g._kf_is_bad(nb) and nb not in mark for nb in g.ordered[k][10:]):
            br["neighbour_past_tenth_ignored"] += 1
        for c in children_of(g, parent, k):
            if not g._kf_is_bad(c) and c not in mark:
                if any(int(parent[x]) == k and g._kf_is_bad(x) for x in range(c)):
                    br["child_after_a_bad_child"] += 1
                local.append(c)
                mark.add(c)
                br["child_taken"] += 1
                break
        pk = int(parent[k])
        if 0 <= pk < g.K and pk not in mark:  # not tested for badness
            if g._kf_is_bad(pk):
                br["bad_parent_appended"] += 1
            local.append(pk)
            mark.add(pk)
            br["parent_break"] += 1
            if parent_break:
                break  # leaves the outer loop
    return fmp, local, kfmax, False


def update_local_points(g: M.Graph, local):
    """cc:1354-1380."""
    pts, seen = [], set()
    for kf in local:
        if kf < 0 or kf >= len(g.clean):
            continue
        for p in g.clean[kf]:
            p = int(p)
            if p < 0 or p in seen or g._mp_is_bad(p):
                continue
            seen.add(p)
            pts.append(p)
    return pts


def update_local_map_batch(g: M.Graph, frame_mp, n, local_kf, local_kf_n, ref_kf, max_local_kf, max_local_points,
                           max_total, parent=None, br: Counter | None = None):
    """orbx_update_local_map_device: B frames against the capacities.  local_kf (B, max_local_kf),
    local_kf_n and ref_kf are the in/out arrays on entry.  Returns the arrays after the call;
    local_kf rows are meaningful up to local_kf_n."""
    br = Counter() if br is None else br
    parent = g.parent if parent is None else parent
    frame_mp = np.array(frame_mp, np.int32, copy=True)
    local_kf = np.array(local_kf, np.int32, copy=True).reshape(len(frame_mp), max_local_kf)
    local_kf_n, ref_kf = np.array(local_kf_n, np.int32, copy=True), np.array(ref_kf, np.int32, copy=True)
    B = len(frame_mp)
    off, ids = [0], []
    counts, status = np.zeros((B, 2), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        old = local_kf[b, :max(0, min(int(local_kf_n[b]), max_local_kf))].tolist()
        fmp, local, kfmax, empty = update_local_keyframes(g, frame_mp[b], n[b], parent, old, br)
        if not empty and len(update_local_keyframes(g, frame_mp[b], n[b], parent, old, Counter(), False)[1]) > len(local):
            br["parent_break_cuts_additions"] += 1
        pts = update_local_points(g, local) if len(local) <= max_local_kf else []
        status[b] = EMPTY if empty else 0
        if len(local) > max_local_kf or len(pts) > max_local_points or off[-1] + len(pts) > max_total:
            status[b] |= CAPACITY
            local_kf_n[b] = 0
            off.append(off[-1])
            br["capacity"] += 1
            continue
        frame_mp[b] = fmp
        if not empty:
            local_kf[b, :len(local)] = local
            local_kf_n[b] = len(local)
            if kfmax is not None:
                ref_kf[b] = kfmax
        counts[b] = (len(local), len(pts))
        ids += pts
        off.append(off[-1] + len(pts))
    return {"frame_mp": frame_mp, "local_kf": local_kf, "local_kf_n": local_kf_n, "ref_kf": ref_kf,
            "local_off": np.array(off, np.int32), "local_ids": np.array(ids, np.int32), "counts": counts, "status": status}


def assert_same(got: dict, want: dict, frame_mp=None) -> None:
    """The device's arrays (LocalMapTracker.state()) equal the model's; local_kf up to local_kf_n,
    local_ids up to the total."""
    for name in ("local_kf_n", "ref_kf", "local_off", "counts", "status"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (name, got[name], want[name])
    for b, m in enumerate(want["local_kf_n"]):
        assert got["local_kf"][b, :m].tolist() == want["local_kf"][b, :m].tolist(), ("local_kf", b)
    total = int(want["local_off"][-1])
    assert got["local_ids"][:total].tobytes() == want["local_ids"].tobytes(), "local_ids"
    if frame_mp is not None:
        assert np.array_equal(frame_mp, want["frame_mp"]), "frame_mp"


def tally(frame_mp, n, outlier, observations, only_tracking=False, stereo=False, recently=None, found=None):
    """cc:1047-1081.  Returns (mvpMapPoints, mnMatchesInliers, ok, mnFound)."""
    fmp = np.array(frame_mp, np.int32, copy=True)
    B, cap = fmp.shape
    found = None if found is None else np.array(found, np.int32, copy=True)
    inl, ok = np.zeros(B, np.int32), np.zeros(B, np.uint8)
    for b in range(B):
        m = 0
        for i in range(max(0, min(int(n[b]), cap))):
            p = int(fmp[b, i])
            if p < 0 or p >= len(observations):
                continue
            if not outlier[b, i]:
                if found is not None:
                    found[p] += 1
                if only_tracking or observations[p] > 0:
                    m += 1
            elif stereo:
                fmp[b, i] = -1
        inl[b] = m
        ok[b] = not ((recently is not None and recently[b] and m < 50) or m < 30)
    return fmp, inl, ok, found


# ---- the scenes of the GPU tests (tests/test_gpu_local_map.py); test_local_map_model.py checks
# that together they reach every branch ----

def band_map(name):
    """A covisibility_model.GPU_SCENES map with every keyframe connected while nothing is bad
    (UpdateConnections in id order), after which keyframes 5, 13 and 14 went bad: they stay in
    their neighbours' lists and keep their children, and 13 is the parent of some keyframe."""
    kf_mp, kf_n, kf_bad, mp_bad = M.scene(**M.GPU_SCENES[name])
    kf_bad = np.zeros_like(kf_bad)
    return kf_mp, kf_n, kf_bad, mp_bad, (5, 13, 14)


def build_graph(kf_mp, kf_n, kf_bad, mp_bad, later_bad=(), max_conn=64):
    """The model graph of a map: connected while nothing of later_bad is bad, then refreshed with
    those keyframes bad.  kf_bad is changed in place."""
    g = M.Graph(len(kf_mp), max_conn)
    g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
    for k in range(len(kf_mp)):
        g.update_connections(k)
    for k in later_bad:
        kf_bad[k] = 1
    g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
    return g


def frames(kf_mp, mp_bad, B, seed, width=3):
    """B frames over a map: frame b's mvpMapPoints are drawn from the rows of `width`
    neighbouring keyframes around a centre, at shuffled indices, with NULL entries, a repeated
    MapPoint, ids outside the table and n on both sides of cap.  Frame 1 is all NULL and frame 2
    sees only MapPoints that no keyframe observes (both: an empty counter)."""
    rng = np.random.default_rng(seed)
    K, cap = kf_mp.shape
    n_mp = len(mp_bad)
    fm = np.full((B, cap), -1, np.int32)
    n = np.zeros(B, np.int32)
    seen = set(int(p) for p in kf_mp.reshape(-1) if p >= 0)
    unseen = [p for p in range(n_mp) if p not in seen]
    for b in range(B):
        n[b] = cap + int(rng.integers(-3, 3))
        if b == 1:
            continue
        if b == 2:
            fm[b, :min(len(unseen), 5)] = unseen[:5]
            continue
        c = int(rng.integers(0, K))
        pool = np.unique(kf_mp[max(0, c - width // 2):c + width // 2 + 1])
        pool = pool[pool >= 0]
        ids = rng.permutation(pool)[:int(rng.integers(cap // 3, cap - 6))]
        slots = rng.permutation(cap)[:len(ids)]
        fm[b, slots] = ids
        free = np.flatnonzero(fm[b] < 0)
        if len(ids) and len(free) >= 3:
            fm[b, free[0]] = ids[0]          # the same MapPoint at two indices
            fm[b, free[1]] = n_mp + 5        # outside the table
            fm[b, free[2]] = -9
    return fm, n


RING_HOLES = (30, 31, 60)
RING_LATER_BAD = (40,)


def ring_map(K=100, cap=32):
    """The made scene for the two 80 cases.  Keyframe k sees the 12 band points 20 + 3 k .. (so
    that neighbours share up to 9); the keyframes below 90 also see the 15 common points 0 .. 14,
    which connects each of them to all the others (lists of 89 entries: an 11th neighbour
    exists), and those in 8 .. 87 but RING_HOLES see point 15.  A frame that holds point 0 votes
    for 90 keyframes (the 80 stop before the first entry); one that holds point 15 votes for 77,
    and the walk over them passes 80 at the holes.  Connect it with max_conn = 128."""
    n_mp = 20 + 3 * K + 12
    kf_mp = np.full((K, cap), -1, np.int32)
    for k in range(K):
        row = list(range(20 + 3 * k, 20 + 3 * k + 12))
        if k < 90:
            row += list(range(15))
        if 8 <= k < 88 and k not in RING_HOLES:
            row.append(15)
        kf_mp[k, :len(row)] = row
    return kf_mp, np.full(K, cap, np.int32), np.zeros(K, np.uint8), np.zeros(n_mp, np.uint8)


def ring_frames(cap=32):
    fm = np.full((4, cap), -1, np.int32)
    fm[0, 3] = 0                       # 90 voted keyframes
    fm[1, 5] = 15                      # 77 voted keyframes, then the walk
    fm[2, :12] = np.arange(20 + 3 * 50, 20 + 3 * 50 + 12)   # a small neighbourhood: 47 .. 53
    fm[3, 0] = 15
    fm[3, 1] = 0
    return fm, np.full(4, cap, np.int32)


def ring_parent(K=100):
    """A caller's spanning tree for the ring: above 50 every keyframe's parent is the one below
    it, so that no parent ends the walk over 8 .. 87 before it has passed 80; 40 (bad), 41 and 42
    are further children of 50."""
    p = np.full(K, -1, np.int32)
    p[51:] = np.arange(50, K - 1)
    p[40:43] = 50
    return p


OLD_LIST = (3, 1, 1000, 2)   # mvpLocalKeyFrames of the frame before (one id outside every map)
OLD_REF = 7


def gpu_case(name):
    """A scene of the GPU tests: the map, when its keyframes went bad, the frames, and the spanning
    trees to run it with (None: the graph's own mpParent)."""
    if name == "ring":
        kf_mp, kf_n, kf_bad, mp_bad = ring_map()
        fm, n = ring_frames()
        return dict(map=(kf_mp, kf_n, kf_bad, mp_bad), later_bad=RING_LATER_BAD, max_conn=128, frame_mp=fm, n=n,
                    parents=(None, ring_parent()), max_local_kf=128)
    kf_mp, kf_n, kf_bad, mp_bad, later = band_map(name)
    fm, n = frames(kf_mp, mp_bad, 40, seed=3)
    return dict(map=(kf_mp, kf_n, kf_bad, mp_bad), later_bad=later, max_conn=64, frame_mp=fm, n=n, parents=(None,),
                max_local_kf=48)


GPU_CASES = ("band24", "band40", "ring")


def initial_lists(B, max_local_kf):
    """The in/out arrays before the first call: every frame holds OLD_LIST and OLD_REF."""
    kf = np.full((B, max_local_kf), -1, np.int32)
    kf[:, :len(OLD_LIST)] = OLD_LIST
    return kf, np.full(B, len(OLD_LIST), np.int32), np.full(B, OLD_REF, np.int32)


def capacity_triple(values, first=3):
    """Three frames [a, mid, c] of values[first:] in which mid holds the strict maximum: a
    capacity of values[a] + values[c] + 1 (or values[mid] - 1 per frame) leaves out mid alone."""
    v = np.asarray(values)[first:]
    order = np.argsort(v, kind="stable")
    assert v[order[-1]] > v[order[1]] + 1
    return [first + int(order[0]), first + int(order[-1]), first + int(order[1])]
