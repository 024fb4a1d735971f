"""Hand-built matcher scenes: keypoints placed by hand, descriptors random bytes or a
prototype with a chosen number of bits flipped.  The extractor is not involved, so a scene
can hold what a natural frame never does: undistortion bounds with keypoints outside them,
hundreds of keypoints in one grid cell, empty top octaves, 2 to 32 levels, counts at the
13-bit position limit.  numpy only; the oracle and the kernels both take these as they are.

Geometry shared by every scene: the current frame's pose is the identity, a query (u, v) is
the MapPoint at depth Z on the ray through (u, v), so every overload projects it back to
(u, v) up to float rounding -- which the oracle and the kernels round alike.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from orbslam2commentedbyxcm_amd import _lib as L
from orbslam2commentedbyxcm_amd.matcher import FrameView, MapPoints, Track

FX = FY = 500.0
CX, CY = 320.0, 240.0
Z = 5.0
W, H = 640.0, 480.0
COLS, ROWS = 64, 48
BOUNDS = (-23.7, 671.3, -17.2, 498.9)   # (min_x, max_x, min_y, max_y), the shape undistortion gives
LEVELS = (2, 5, 6, 17, 27, 32)
CAPACITY = ((8191, 8191), (8191, 16382), (1000, 9000), (7000, 8192))
CAPACITY_REFUSED = (8192, 100)


def keypoints(x, y, octave, rng):
    k = np.zeros(len(x), L.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = np.asarray(x, np.float32), np.asarray(y, np.float32), octave
    k["angle"] = rng.uniform(0, 360, len(x)).astype(np.float32)
    k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
    return k


def flip_bits(desc, nbits, rng):
    """desc (32,) u8 with nbits distinct bits flipped."""
    d = desc.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def scale_factors(nlevels, sf):
    return (np.float32(sf) ** np.arange(nlevels)).astype(np.float32)


def frame(keys, desc, nlevels, sf=1.2, bounds=(0.0, W, 0.0, H), stereo=False, Tcw=None):
    s = scale_factors(nlevels, sf)
    return FrameView(keys=keys, desc=desc, fx=FX, fy=FY, cx=CX, cy=CY, bf=250.0 if stereo else 0.0,
                     b=0.5 if stereo else 0.0, min_x=bounds[0], max_x=bounds[1], min_y=bounds[2], max_y=bounds[3],
                     scale_factors=s, level_sigma2=(s * s).astype(np.float32),
                     Tcw=np.eye(4, dtype=np.float32) if Tcw is None else Tcw)


def grid_cells(F):
    """(px, py) of Frame::PosInGrid per keypoint (C roundf: half away from zero), unclipped."""
    inv_w = np.float32(COLS) / (np.float32(F.max_x) - np.float32(F.min_x))
    inv_h = np.float32(ROWS) / (np.float32(F.max_y) - np.float32(F.min_y))
    fx = ((F.keys["x"] - np.float32(F.min_x)) * inv_w).astype(np.float32).astype(np.float64)
    fy = ((F.keys["y"] - np.float32(F.min_y)) * inv_h).astype(np.float32).astype(np.float64)
    rnd = lambda v: (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)  # noqa: E731
    return rnd(fx), rnd(fy), fx, fy


def on_grid(F):
    px, py, _, _ = grid_cells(F)
    return (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)


def scene(F, u, v, level, qdesc, rng, obs=None, view_cos=None, order=None, angle=None):
    """A scene: frame F queried by MapPoints at (u, v) with predicted level `level` and
    descriptors qdesc.  MapPoint k lies at depth Z on the ray through (u, v)[k], seen from
    the origin; mfMaxDistance is set so that PredictScale gives level[k] in F; queries is the
    vpMapPoints order (default: ids ascending); trk the hand-made IsInFrustum outputs; angle
    the keypoint angle each MapPoint has in the last frame / keyframe (default: random)."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    level = np.asarray(level, np.int32)
    m = len(u)
    pos = np.stack([(u - np.float32(CX)) / np.float32(FX) * np.float32(Z),
                    (v - np.float32(CY)) / np.float32(FY) * np.float32(Z), np.full(m, Z, np.float32)], 1).astype(np.float32)
    dist = np.linalg.norm(pos.astype(np.float64), axis=1)
    sf = np.asarray(F.scale_factors, np.float64)
    # ratio = sf^level shrunk by a fifth of a level: ceil(log(ratio) / log(sf)) == level
    mx = (dist * sf[level] * (1.0 - 0.2 * (sf[1] - 1.0))).astype(np.float32)
    mps = MapPoints(desc=np.ascontiguousarray(qdesc, np.uint8),
                    observations=np.ones(m, np.int32) if obs is None else np.asarray(obs, np.int32), pos=pos,
                    bad=np.zeros(m, np.uint8), max_distance=mx, min_distance=(mx / np.float32(sf[-1])).astype(np.float32),
                    normal=(pos / dist[:, None]).astype(np.float32))
    trk = Track(in_view=np.ones(m, np.uint8), proj_x=u, proj_y=v,
                proj_xr=(u - np.float32(F.bf) / np.float32(Z)).astype(np.float32), scale_level=level,
                view_cos=np.full(m, 0.9995, np.float32) if view_cos is None else np.asarray(view_cos, np.float32))
    q = np.arange(m, dtype=np.int32) if order is None else np.asarray(order, np.int32)
    return SimpleNamespace(F=F, mps=mps, trk=trk, queries=q, u=u, v=v, level=level,
                           frame_mp0=np.full(len(F.keys), -1, np.int32),
                           angle=rng.uniform(0, 360, m).astype(np.float32) if angle is None else np.asarray(angle, np.float32))


def last_frame(S, tz=0.0):
    """The LastFrame of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (and the
    KeyFrame of the relocalisation overload): keypoint i carries MapPoint i at octave
    level[i].  tz: the z of its pose's translation; with the identity rotation tlc.z = tz, so
    tz > mb makes bForward true and tz < -mb bBackward (ORBmatcher.cc:1643-1651)."""
    T = np.eye(4, dtype=np.float32)
    T[2, 3] = tz
    k = np.zeros(len(S.u), L.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = S.u, S.v, S.level, S.angle
    k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
    F = S.F
    return FrameView(keys=k, desc=S.mps.desc, fx=FX, fy=FY, cx=CX, cy=CY, bf=F.bf, b=F.b, min_x=F.min_x, max_x=F.max_x,
                     min_y=F.min_y, max_y=F.max_y, scale_factors=F.scale_factors, level_sigma2=F.level_sigma2, Tcw=T)


def _own_queries(keys, desc, idx, rng, nlevels, noise=1.5, flips=(0, 12)):
    """Queries on the keypoints idx: 1-2 px of noise, the keypoint's descriptor with a few
    bits flipped (one in five: 40-110 bits, around the acceptance threshold TH_HIGH = 100 and
    the ratio test), predicted level the keypoint's octave or one above (both reach it); the
    angle in the last frame is the keypoint's turned by 24 +- 3 degrees (one in ten: any), so
    the rotation histogram has a dominant bin."""
    u = keys["x"][idx] + rng.uniform(-noise, noise, len(idx)).astype(np.float32)
    v = keys["y"][idx] + rng.uniform(-noise, noise, len(idx)).astype(np.float32)
    lv = np.minimum(keys["octave"][idx] + rng.integers(0, 2, len(idx)), nlevels - 1)
    nb = np.where(rng.random(len(idx)) < 0.2, rng.integers(40, 111, len(idx)), rng.integers(flips[0], flips[1] + 1, len(idx)))
    qd = np.stack([flip_bits(desc[i], int(b), rng) for i, b in zip(idx, nb)])
    ang = (keys["angle"][idx] + 24.0 + rng.normal(0, 3, len(idx))) % 360.0
    ang = np.where(rng.random(len(idx)) < 0.1, rng.uniform(0, 360, len(idx)), ang).astype(np.float32)
    ang[ang >= 360.0] = 0.0
    return u, v, lv, qd, ang


def uniform(seed, n, nq, nlevels, sf=1.2, top=None, bounds=(0.0, W, 0.0, H)):
    """n keypoints uniform over the image, octave i % (top + 1) (every octave 0..top occurs;
    top defaults to the last level); nq queries on keypoints i % n in a seeded order."""
    rng = np.random.default_rng(seed)
    top = nlevels - 1 if top is None else top
    keys = keypoints(rng.uniform(1, W - 1, n), rng.uniform(1, H - 1, n), np.arange(n) % (top + 1), rng)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    F = frame(keys, desc, nlevels, sf, bounds)
    idx = rng.permutation(nq) % n
    u, v, lv, qd, ang = _own_queries(keys, desc, idx, rng, nlevels)
    S = scene(F, u, v, lv, qd, rng, angle=ang)
    S.target = idx
    return S


def knife_edge_x(k, min_x, inv_w):
    """A float x with float((x - min_x) * inv_w) == k + 0.5 exactly (the cell index then
    rounds half away from zero, to k + 1)."""
    t = np.float32(k + 0.5)
    x = np.float32(np.float32(min_x) + t / inv_w)
    for step in range(-64, 65):
        c = x
        for _ in range(abs(step)):
            c = np.nextafter(c, np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
        if np.float32(np.float32(c - np.float32(min_x)) * inv_w) == t:
            return c
    raise AssertionError(f"no float on the half-cell edge {k}")


def bounds(seed=0):
    """Undistortion-shaped bounds; ~1500 keypoints drawn up to 8 px beyond them on every side
    (some off-grid on each), 64 on the half-cell knife edge in x; queries on own keypoints,
    `outside` queries whose window misses the grid on each side, and `wide`: a second scene of
    a few queries whose radius (at th = WIDE_TH) covers the whole grid."""
    rng = np.random.default_rng(seed)
    mnx, mxx, mny, mxy = BOUNDS
    n0 = 1500
    x = rng.uniform(mnx - 8, mxx + 8, n0).astype(np.float32)
    y = rng.uniform(mny - 8, mxy + 8, n0).astype(np.float32)
    # a strip along every side, so each side has its off-grid keypoints whatever the seed
    strip = 40
    x[:strip] = rng.uniform(mnx - 8, mnx - 5.5, strip)
    x[strip:2 * strip] = rng.uniform(mxx + 0.5, mxx + 8, strip)
    y[2 * strip:3 * strip] = rng.uniform(mny - 8, mny - 5.5, strip)
    y[3 * strip:4 * strip] = rng.uniform(mxy + 0.5, mxy + 8, strip)
    inv_w = np.float32(COLS) / (np.float32(mxx) - np.float32(mnx))
    ex = np.array([knife_edge_x(k, mnx, inv_w) for k in range(64)], np.float32)
    ey = rng.uniform(mny + 20, mxy - 20, 64).astype(np.float32)
    x, y = np.concatenate([x, ex]), np.concatenate([y, ey])
    n = len(x)
    keys = keypoints(x, y, rng.integers(0, 8, n), rng)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    F = frame(keys, desc, 8, 1.2, BOUNDS)
    idx = rng.permutation(n)[:1380]
    u, v, lv, qd, ang = _own_queries(keys, desc, idx, rng, 8)
    # windows wholly outside the grid, 30 per side (r <= 4 * 1.2^7 = 14.4 at th = 1)
    no = 30
    ou = np.concatenate([np.full(no, mnx - 60.0), np.full(no, mxx + 60.0), rng.uniform(mnx, mxx, 2 * no)])
    ov = np.concatenate([rng.uniform(mny, mxy, 2 * no), np.full(no, mny - 60.0), np.full(no, mxy + 60.0)])
    od = desc[rng.integers(0, n, 4 * no)]
    S = scene(F, np.concatenate([u, ou]), np.concatenate([v, ov]), np.concatenate([lv, rng.integers(0, 8, 4 * no)]),
              np.concatenate([qd, od]), rng, obs=rng.integers(0, 3, len(u) + 4 * no),
              view_cos=rng.choice(np.array([0.9995, 0.99], np.float32), len(u) + 4 * no),
              order=rng.permutation(len(u) + 4 * no), angle=np.concatenate([ang, rng.uniform(0, 360, 4 * no)]))
    S.outside = np.arange(len(u), len(u) + 4 * no)
    S.knife = np.arange(n0, n)
    S.frame_mp0[rng.random(n) < 0.1] = 3
    wi = rng.permutation(np.nonzero((keys["octave"] >= 6) & on_grid(F) & (S.frame_mp0 < 0))[0])[:6]
    S.wide = scene(F, keys["x"][wi], keys["y"][wi], np.full(6, 7), np.stack([flip_bits(desc[i], 5, rng) for i in wi]), rng)
    return S


WIDE_TH = 100.0  # 2.5 * 100 * 1.2^7 = 896 px: every cell of the grid


CELL_U, CELL_V = 320.0, 240.0   # the centre of grid cell (32, 24) of the 640 x 480 image
GROUPS, PER_GROUP = 30, 20


def one_cell(seed=0, half_zero=False, shuffled=False, per_group=PER_GROUP, off_grid=False):
    """GROUPS prototype groups x per_group keypoints, all inside one 10 x 10 px grid cell;
    keypoint j of a group has the prototype with j bits flipped and octave j & 1.  Each group
    is queried by per_group MapPoints carrying the prototype itself at predicted level 1,
    projected at the cell centre.  With every Observations() > 0 the k-th query of a group
    takes the keypoint of rank k: beyond the 12 entries of its candidate list from k = 12 on.
    half_zero: every other MapPoint has Observations() == 0 (its claims do not block).
    off_grid: the twin -- the same keypoints moved past the right bound (cell column 65), the
    queries beside them at a radius that reaches them: they are in no cell, nothing matches."""
    rng = np.random.default_rng(seed)
    n = GROUPS * per_group
    dx = 327.5 if off_grid else 0.0
    x = CELL_U + dx + rng.uniform(-2.4, 2.4, n)
    y = CELL_V + rng.uniform(-2.4, 2.4, n)
    proto = rng.integers(0, 256, (GROUPS, 32), dtype=np.uint8)
    rank = np.tile(np.arange(per_group), GROUPS)
    group = np.repeat(np.arange(GROUPS), per_group)
    desc = np.stack([flip_bits(proto[g], int(j), rng) for g, j in zip(group, rank)])
    perm = rng.permutation(n)   # the keypoint order carries no information
    keys = keypoints(x[perm], y[perm], rank[perm] & 1, rng)
    F = frame(keys, desc[perm], 8)
    m = GROUPS * per_group
    qgroup = np.repeat(np.arange(GROUPS), per_group)
    obs = np.ones(m, np.int32)
    if half_zero:
        obs[::2] = 0
    u = np.full(m, 639.5 if off_grid else CELL_U, np.float32)
    S = scene(F, u, np.full(m, CELL_V, np.float32), np.ones(m, np.int32), proto[qgroup], rng, obs=obs,
              order=rng.permutation(m) if shuffled else None)
    S.rank, S.group, S.qgroup = rank[perm], group[perm], qgroup
    return S


OFF_GRID_TH = 4.0   # 2.5 * 4 * 1.2 = 12 px: from u = 639.5 past every twin keypoint (x < 650)


def lines(kind, seed=0):
    """All keypoints in grid column 0, in column 63, in row 47; one keypoint; one query."""
    rng = np.random.default_rng(seed)
    n, nq = 400, 400
    if kind == "n1":
        n = 1
    if kind == "nq1":
        nq = 1
    x, y = rng.uniform(1, W - 1, n), rng.uniform(1, H - 1, n)
    if kind == "col0":
        x = rng.uniform(0.0, 4.9, n)
    elif kind == "col63":
        x = rng.uniform(625.1, 634.9, n)
    elif kind == "row47":
        y = rng.uniform(465.1, 474.9, n)
    keys = keypoints(x, y, rng.integers(0, 8, n), rng)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    F = frame(keys, desc, 8)
    idx = rng.permutation(max(n, nq))[:nq] % n
    u, v, lv, qd, ang = _own_queries(keys, desc, idx, rng, 8)
    return scene(F, u, v, lv, qd, rng, obs=rng.integers(0, 3, nq), angle=ang)


LINES = ("col0", "col63", "row47", "n1", "nq1")


def levels(nlevels, seed=0, n=None):
    """nlevels levels at scale factor 1.05, every octave populated, 700-1200 keypoints."""
    n = 700 + 500 * nlevels // 32 if n is None else n
    return uniform(seed + nlevels, n, n, nlevels, sf=1.05)


MISSING_TOP_HIGH = 240


def missing_top(seed=0, stereo=False, n=900):
    """8 levels in the frame view, keypoints only in octaves 0-4 (a third of them in octave
    4).  600 queries on own keypoints of every octave at the octave's level or the one above:
    every level 0-5 occurs, and level 5, whose range [4, 5] straddles the highest populated
    octave, still reaches its octave-4 keypoint.  MISSING_TOP_HIGH more (`high`) at levels 6
    and 7, each exactly on another octave-4 keypoint with that keypoint's descriptor: their
    octave range [5, 6] or [6, 7] lies wholly above the frame's keypoints, so the reference
    matches none of them."""
    rng = np.random.default_rng(seed)
    keys = keypoints(rng.uniform(1, W - 1, n), rng.uniform(1, H - 1, n), np.minimum(np.arange(n) % 6, 4), rng)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    F = frame(keys, desc, 8, stereo=stereo)
    o4 = rng.permutation(np.nonzero(keys["octave"] == 4)[0])
    rest = np.nonzero(keys["octave"] < 4)[0]
    hi = o4[:MISSING_TOP_HIGH // 2]
    own4 = o4[MISSING_TOP_HIGH // 2:][:150]         # the octave-4 keypoints of the ordinary queries
    hi = np.concatenate([hi, hi])                   # each at level 6 and at level 7
    idx = rng.permutation(np.concatenate([own4, rng.permutation(rest)[:600 - len(own4)]]))
    u, v, lv, qd, ang = _own_queries(keys, desc, idx, rng, 8)
    m = len(idx) + len(hi)
    order = rng.permutation(m)
    S = scene(F, np.concatenate([u, keys["x"][hi]]), np.concatenate([v, keys["y"][hi]]),
              np.concatenate([lv, np.repeat([6, 7], MISSING_TOP_HIGH // 2)]), np.concatenate([qd, desc[hi]]), rng,
              order=order, angle=np.concatenate([ang, (keys["angle"][hi] + 24.0) % 360.0]))
    S.high = np.arange(len(idx), m)
    S.high_target = hi
    S.target = idx                                  # the keypoint under each ordinary query
    return S


def capacity(n, nq, seed=0):
    """Uniform keypoints, 8 levels, at the 13-bit position limit."""
    return uniform(seed + 100, n, nq, 8)


# ---- the batched device forms: frames padded to cap, MapPoints of every frame in one table

def device_batch(scenes, cap):
    """Host arrays for search_local_points_device / match_sequence_device from one scene per
    frame (None = an empty frame): kps (B, cap, 7) i32 words, desc (B, cap, 32) u8, n (B,),
    Tcw (B, 12); the MapPoint table is the scenes' MapPoints one after another, local_ids the
    scenes' query lists shifted into it, local_off (B + 1,)."""
    B = len(scenes)
    kps = np.zeros((B, cap, 7), np.int32)
    desc = np.zeros((B, cap, 32), np.uint8)
    n = np.zeros(B, np.int32)
    T = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (B, 1))
    mp = {k: [] for k in ("pos", "desc", "normal", "max_distance", "min_distance", "observations", "bad")}
    ids, off, base = [], [0], []
    tot = 0
    for b, S in enumerate(scenes):
        base.append(tot)
        if S is None:
            off.append(off[-1])
            continue
        k = len(S.F.keys)
        assert k <= cap
        n[b] = k
        kps[b, :k] = np.ascontiguousarray(S.F.keys).view(np.int32).reshape(k, 7)
        desc[b, :k] = S.F.desc
        for name in mp:
            mp[name].append(getattr(S.mps, name))
        ids.append(S.queries + tot)
        tot += len(S.mps.desc)
        off.append(off[-1] + len(S.queries))
    mp = {k: np.concatenate(v) for k, v in mp.items()}
    table = MapPoints(desc=mp["desc"], observations=mp["observations"], pos=mp["pos"], bad=mp["bad"],
                      max_distance=mp["max_distance"], min_distance=mp["min_distance"], normal=mp["normal"])
    return SimpleNamespace(kps=kps, desc=desc, n=n, Tcw=T, mps=mp, table=table,
                           local_ids=np.concatenate(ids).astype(np.int32), local_off=np.array(off, np.int32), base=base)


def sequence_batch(frames, cap):
    """Host arrays for match_sequence_device from FrameViews (None = an empty frame), every
    pose the identity: kps (B, cap, 7) i32 words, desc (B, cap, 32) u8, n (B,), Tcw (B, 12)."""
    B = len(frames)
    kps = np.zeros((B, cap, 7), np.int32)
    desc = np.zeros((B, cap, 32), np.uint8)
    n = np.zeros(B, np.int32)
    for b, F in enumerate(frames):
        if F is None:
            continue
        k = len(F.keys)
        assert k <= cap
        n[b] = k
        kps[b, :k] = np.ascontiguousarray(F.keys).view(np.int32).reshape(k, 7)
        desc[b, :k] = F.desc
    return SimpleNamespace(kps=kps, desc=desc, n=n, Tcw=np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (B, 1)))
