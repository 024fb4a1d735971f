"""A literal Python restatement of the reference's covisibility graph, one call at a time.

KeyFrame::AddConnection / UpdateBestCovisibles / GetBestCovisibilityKeyFrames /
GetCovisiblesByWeight / UpdateConnections / SetBadFlag's connection part / EraseConnection
(src/KeyFrame.cc:139-229, 324-415, 506-520, 607-620), MapPoint::GetObservations() rebuilt from
the keyframes' mvpMapPoints, and the graph walk of Optimizer::LocalBundleAdjustment
(src/Optimizer.cc:526-583, 656-760) producing the tables of INTEGRATION.md 4e'.  Dicts are
ordered by keyframe id, which stands in for the reference's KeyFrame* order.  Not a test module.
"""
from __future__ import annotations

import bisect

import numpy as np

TH = 15
CAPACITY, BAD_KEYFRAME, DUPLICATE = 1, 2, 4


def observations(kf_mp, kf_n, kf_bad, n_mp):
    """The cleaned copy of mvpMapPoints, per point its observers {kf: idx} in ascending keyframe
    id (rows of bad keyframes contribute nothing), and the keyframes with a duplicate."""
    kf_mp = np.asarray(kf_mp)
    K, cap = kf_mp.shape
    clean = np.full((K, cap), -1, np.int32)
    obs = [dict() for _ in range(n_mp)]
    dup = np.zeros(K, bool)
    for k in range(K):
        seen = set()
        for i in range(max(0, min(int(kf_n[k]), cap))):
            p = int(kf_mp[k, i])
            if p < 0 or p >= n_mp:
                continue
            if p in seen:
                dup[k] = True  # the lowest index holds the observation
                continue
            seen.add(p)
            clean[k, i] = p
            if kf_bad is None or not kf_bad[k]:
                obs[p][k] = i  # k ascends: the dict is in keyframe-id order
    return clean, obs, dup


class Graph:
    def __init__(self, K, max_conn=8192):
        self.K, self.max_conn = K, max_conn
        self.row = [dict() for _ in range(K)]      # mConnectedKeyFrameWeights
        self.ordered = [[] for _ in range(K)]      # mvpOrderedConnectedKeyFrames
        self.weights = [[] for _ in range(K)]      # mvOrderedWeights
        self.first = [True] * K                    # mbFirstConnection
        self.parent = [-1] * K                     # mpParent
        self.status = [0] * K
        self.clean = self.obs = None
        self.kf_n = self.kf_bad = self.mp_bad = None

    def refresh_observations(self, kf_mp, kf_n, kf_bad=None, mp_bad=None, n_mp=None):
        n_mp = len(mp_bad) if n_mp is None else n_mp
        self.clean, self.obs, dup = observations(kf_mp, kf_n, kf_bad, n_mp)
        self.kf_n, self.kf_bad, self.mp_bad = kf_n, kf_bad, mp_bad
        for k in range(len(dup)):
            self.status[k] = (self.status[k] & ~DUPLICATE) | (DUPLICATE if dup[k] else 0)

    def _kf_is_bad(self, k):
        return self.kf_bad is not None and k < len(self.kf_bad) and bool(self.kf_bad[k])

    def _mp_is_bad(self, p):
        return self.mp_bad is not None and bool(self.mp_bad[p])

    # cc:160-182
    def update_best_covisibles(self, k):
        pairs = sorted((w, kf) for kf, w in self.row[k].items())
        self.ordered[k] = [kf for _, kf in reversed(pairs)]
        self.weights[k] = [w for w, _ in reversed(pairs)]

    # cc:139-153; a row that would exceed max_conn: CAPACITY, state untouched
    def add_connection(self, k, kf, w):
        if kf not in self.row[k]:
            if len(self.row[k]) + 1 > self.max_conn:
                self.status[k] |= CAPACITY
                return
            self.row[k][kf] = w
            self.row[k] = dict(sorted(self.row[k].items()))
        elif self.row[k][kf] != w:
            self.row[k][kf] = w
        else:
            return
        self.update_best_covisibles(k)

    # cc:324-415
    def update_connections(self, k):
        if self._kf_is_bad(k):
            self.status[k] |= BAD_KEYFRAME
            return
        counter = {}
        if k < len(self.clean):
            for p in self.clean[k]:
                p = int(p)
                if p < 0 or self._mp_is_bad(p):
                    continue
                for kf in self.obs[p]:
                    if kf == k:
                        continue
                    counter[kf] = counter.get(kf, 0) + 1
        if not counter:
            return
        counter = dict(sorted(counter.items()))
        if len(counter) > self.max_conn:
            self.status[k] |= CAPACITY
            return
        nmax, kfmax = 0, None
        pairs = []
        for kf, w in counter.items():
            if w > nmax:
                nmax, kfmax = w, kf
            if w >= TH:
                pairs.append((w, kf))
                self.add_connection(kf, k, w)
        if not pairs:
            pairs.append((nmax, kfmax))
            self.add_connection(kfmax, k, nmax)
        pairs.sort()
        self.row[k] = counter
        self.ordered[k] = [kf for _, kf in reversed(pairs)]
        self.weights[k] = [w for w, _ in reversed(pairs)]
        if self.first[k] and k != 0:
            self.parent[k] = self.ordered[k][0]
            self.first[k] = False

    # cc:607-620
    def erase_connection(self, k, kf):
        if kf in self.row[k]:
            del self.row[k][kf]
            self.update_best_covisibles(k)

    # cc:497, 506-508, 519-520
    def erase_keyframe(self, k):
        if k == 0:
            return
        for kf in list(self.row[k]):
            if kf != k:
                self.erase_connection(kf, k)
        self.row[k] = {}
        self.ordered[k] = []
        self.weights[k] = []

    # cc:201-209
    def best_covisibles(self, k, N):
        return self.ordered[k] if len(self.ordered[k]) < N else self.ordered[k][:N]

    # cc:212-229: upper_bound with weightComp(a, b) = a > b on the descending weights
    def covisibles_by_weight(self, k, w):
        if not self.ordered[k]:
            return []
        ws = self.weights[k]
        it = bisect.bisect_right([-x for x in ws], -w)  # first element with w > element
        if it == len(ws) and ws[-1] < w:
            return []
        return self.ordered[k][:it]

    def arrays(self):
        """The state in the device's layout ([K][max_conn] tables are compared up to their counts)."""
        K = self.K
        return {"row": [list(r.items()) for r in self.row], "ordered": [list(zip(o, w)) for o, w in zip(self.ordered, self.weights)],
                "parent": np.array(self.parent, np.int32), "first": np.array(self.first, np.uint8),
                "status": np.array(self.status, np.int32), "K": K}


def device_arrays(st):
    """CovisibilityGraph.state() in the form of Graph.arrays()."""
    K = len(st["row_n"])
    return {"row": [list(zip(st["row_kf"][k, :st["row_n"][k]].tolist(), st["row_w"][k, :st["row_n"][k]].tolist()))
                    for k in range(K)],
            "ordered": [list(zip(st["ordered_kf"][k, :st["ordered_n"][k]].tolist(),
                                 st["ordered_w"][k, :st["ordered_n"][k]].tolist())) for k in range(K)],
            "parent": st["parent"], "first": st["first"], "status": st["status"], "K": K}


def assert_same_state(model: Graph, st) -> None:
    a, b = model.arrays(), device_arrays(st)
    assert a["K"] == b["K"]
    for k in range(a["K"]):
        assert a["row"][k] == b["row"][k], ("row", k, a["row"][k], b["row"][k])
        assert a["ordered"][k] == b["ordered"][k], ("ordered", k, a["ordered"][k], b["ordered"][k])
    for name in ("parent", "first", "status"):
        assert np.array_equal(a[name], b[name]), (name, a[name], b[name])


def observation_csr(obs):
    """obs_off, obs_kf, obs_idx of a list of {kf: idx} dicts."""
    off = np.zeros(len(obs) + 1, np.int32)
    kf, idx = [], []
    for p, d in enumerate(obs):
        for k, i in d.items():
            kf.append(k)
            idx.append(i)
        off[p + 1] = len(kf)
    return off, np.array(kf, np.int32), np.array(idx, np.int32)


def assemble_local_ba(g: Graph, cur, poses, mp_pos):
    """Optimizer.cc:526-583 and the edge walk of cc:656-760 for the current keyframe `cur`: the
    tables of INTEGRATION.md 4e' plus the global ids."""
    local = [cur] + [k for k in g.ordered[cur] if not g._kf_is_bad(k)]  # cc:528-539
    is_local = set([cur] + list(g.ordered[cur]))  # mnBALocalForKF is set on bad neighbours too
    pts, seen = [], set()
    for k in local:  # cc:544-561
        for p in g.clean[k]:
            p = int(p)
            if p < 0 or g._mp_is_bad(p) or p in seen:
                continue
            seen.add(p)
            pts.append(p)
    fixed, marked = [], set()
    for p in pts:  # cc:566-583
        for k in g.obs[p]:
            if k not in is_local and k not in marked:
                marked.add(k)
                if not g._kf_is_bad(k):
                    fixed.append(k)
    kf_id = local + fixed
    row_of = {k: r for r, k in enumerate(kf_id)}
    obs_off, obs_kf, obs_kp = [0], [], []
    for p in pts:  # cc:656-760: every observer that is not bad is a vertex
        for k, i in g.obs[p].items():
            if g._kf_is_bad(k) or k not in row_of:
                continue
            obs_kf.append(row_of[k])
            obs_kp.append(i)
        obs_off.append(len(obs_kf))
    kf_id = np.array(kf_id, np.int32)
    pt_id = np.array(pts, np.int32)
    return {"kf_id": kf_id, "pt_id": pt_id,
            "kf_Tcw": np.asarray(poses, np.float32).reshape(-1, 12)[kf_id],
            "kf_fixed": np.array([1 if (r >= len(local) or k == 0) else 0 for r, k in enumerate(kf_id)], np.uint8),
            "kf_slot": kf_id.copy(), "pt_pos": np.asarray(mp_pos, np.float32).reshape(-1, 3)[pt_id].reshape(-1, 3),
            "obs_off": np.array(obs_off, np.int32), "obs_kf": np.array(obs_kf, np.int32),
            "obs_kp": np.array(obs_kp, np.int32)}


def assemble_batch(g: Graph, cur_kf, poses, mp_pos, max_kf_rows, max_pt_rows, max_obs):
    """B problems into one set of tables: a problem that does not fit the remaining capacity gets
    empty ranges and CAPACITY; the others are laid out as if it were not there."""
    B = len(cur_kf)
    kf_off, pt_off = [0], [0]
    out = {k: [] for k in ("kf_id", "pt_id", "kf_Tcw", "kf_fixed", "kf_slot", "pt_pos", "obs_kf", "obs_kp")}
    obs_off = [0]
    counts = np.zeros((B, 3), np.int32)
    status = np.zeros(B, np.int32)
    for b, cur in enumerate(cur_kf):
        t = assemble_local_ba(g, int(cur), poses, mp_pos)
        nk, npt, no = len(t["kf_id"]), len(t["pt_id"]), len(t["obs_kf"])
        if kf_off[-1] + nk > max_kf_rows or pt_off[-1] + npt > max_pt_rows or obs_off[-1] + no > max_obs:
            status[b] = CAPACITY
            kf_off.append(kf_off[-1])
            pt_off.append(pt_off[-1])
            continue
        counts[b] = (nk, npt, no)
        for k in out:
            out[k].append(t[k])
        obs_off.extend((t["obs_off"][1:] + obs_off[-1]).tolist())
        kf_off.append(kf_off[-1] + nk)
        pt_off.append(pt_off[-1] + npt)

    def cat(name, dtype, tail=()):
        return np.concatenate(out[name]).astype(dtype) if out[name] else np.zeros((0,) + tail, dtype)

    return {"kf_off": np.array(kf_off, np.int32), "pt_off": np.array(pt_off, np.int32), "obs_off": np.array(obs_off, np.int32),
            "kf_id": cat("kf_id", np.int32), "pt_id": cat("pt_id", np.int32), "kf_Tcw": cat("kf_Tcw", np.float32, (12,)),
            "kf_fixed": cat("kf_fixed", np.uint8), "kf_slot": cat("kf_slot", np.int32),
            "pt_pos": cat("pt_pos", np.float32, (3,)), "obs_kf": cat("obs_kf", np.int32), "obs_kp": cat("obs_kp", np.int32),
            "counts": counts, "status": status}


def scene(seed, K=24, cap=96, window=70, step=9, n_null=10, n_bad_mp=6, bad_kfs=(5,), lonely=True):
    """Keyframes along a path, each seeing a window of points: banded covisibility with NULL
    entries, bad points and bad keyframes.  Keyframe k sees a random subset of the points
    [k * step, k * step + window) at shuffled indices; the last keyframe (lonely) sees only
    points nobody else does, so its counter is empty, and the one before it a few points of the
    first window, so that it connects to pKFmax alone.  Returns kf_mp (K, cap) int32, kf_n (K,),
    kf_bad (K,) u8, mp_bad (n,) u8."""
    rng = np.random.default_rng(seed)
    n = (K + 2) * step + window + cap
    kf_mp = np.full((K, cap), -1, np.int32)
    kf_n = np.zeros(K, np.int32)
    for k in range(K):
        if lonely and k == K - 1:
            ids = np.arange(n - cap // 2, n - cap // 2 + 8)
        elif lonely and k == K - 2:  # a few points of the first window: no weight reaches 15
            ids = rng.permutation(np.arange(0, 2 * step))[:step]
        else:
            w = np.arange(k * step, k * step + window)
            ids = rng.permutation(w)[:int(rng.integers(window // 2, min(window, cap - n_null)))]
        row = np.full(cap, -1, np.int32)
        slots = rng.permutation(cap - 4)[:len(ids)]
        row[slots] = ids
        kf_mp[k] = row
        kf_n[k] = cap - int(rng.integers(0, 4))
        kf_mp[k, kf_n[k]:] = -1
    kf_bad = np.zeros(K, np.uint8)
    for k in bad_kfs:
        if k < K:
            kf_bad[k] = 1
    mp_bad = np.zeros(n, np.uint8)
    mp_bad[rng.permutation((K - 1) * step + window)[:n_bad_mp]] = 1
    return kf_mp, kf_n, kf_bad, mp_bad


def mutate(kf_mp, subset, rng, drop=12):
    """A copy of the table in which each keyframe of `subset` lost `drop` of its points."""
    out = np.array(kf_mp, np.int32, copy=True)
    for k in subset:
        have = np.flatnonzero(out[k] >= 0)
        out[k, rng.permutation(have)[:drop]] = -1
    return out


# the scenes of the GPU tests (tests/test_gpu_covisibility.py); test_covisibility_model.py checks
# that each reaches every case
GPU_SCENES = {"band24": dict(seed=11, K=24, cap=96), "band40": dict(seed=12, K=40, cap=65, window=50, step=6, n_null=8)}
GPU_SUBSET = [8, 9, 10]
GPU_CURRENT = [0, 9, 12, 5, 23]


def geometric_scene(seed, K=10, cap=64, n_pts=220, spacing=1.2):
    """A map with geometry for the LocalBA chain: keyframes along x looking down z, each seeing
    the points that project into its 640 x 480 image; keypoints are the noisy projections.
    Returns a dict: kf_mp, kf_n, kf_bad, mp_bad, poses (K, 12), mp_pos (n, 3), xy (K, cap, 2),
    octave (K, cap), u_right (K, cap), cam (fx, fy, cx, cy, bf), inv_sigma2 (8,)."""
    rng = np.random.default_rng(seed)
    fx = fy = 400.0
    cx, cy, bf = 320.0, 240.0, 40.0
    X = np.stack([rng.uniform(-3, spacing * K + 3, n_pts), rng.uniform(-2, 2, n_pts), rng.uniform(4, 8, n_pts)], 1)
    kf_mp = np.full((K, cap), -1, np.int32)
    xy = np.zeros((K, cap, 2), np.float32)
    octave = rng.integers(0, 4, (K, cap)).astype(np.int32)
    u_right = np.full((K, cap), -1.0, np.float32)
    poses = np.zeros((K, 12), np.float32)
    for k in range(K):
        c = np.array([spacing * k, 0.0, 0.0])
        T = np.hstack([np.eye(3), -c[:, None]])
        Xc = X - c
        u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        vis = np.flatnonzero((u > 0) & (u < 640) & (v > 0) & (v < 480))
        ids = rng.permutation(vis)[:cap - 6]
        slots = rng.permutation(cap)[:len(ids)]
        kf_mp[k, slots] = ids
        xy[k, slots, 0] = u[ids] + rng.normal(0, 0.5, len(ids))
        xy[k, slots, 1] = v[ids] + rng.normal(0, 0.5, len(ids))
        stereo = rng.random(len(ids)) < 0.5
        ur = u[ids] - bf / Xc[ids, 2] + rng.normal(0, 0.5, len(ids))
        u_right[k, slots] = np.where(stereo, ur, -1.0)
        T[:, 3] += rng.normal(0, 0.01, 3)
        poses[k] = T.reshape(-1)
    sigma2 = 1.44 ** np.arange(8)
    return {"kf_mp": kf_mp, "kf_n": np.full(K, cap, np.int32), "kf_bad": np.zeros(K, np.uint8),
            "mp_bad": np.zeros(n_pts, np.uint8), "poses": poses,
            "mp_pos": (X + rng.normal(0, 0.02, X.shape)).astype(np.float32), "xy": xy, "octave": octave,
            "u_right": u_right, "cam": (fx, fy, cx, cy, bf), "inv_sigma2": (1.0 / sigma2).astype(np.float32)}
