"""Synthetic relocalisation candidates for the PnPsolver tests, the plan each is driven by, and
the guard that says what may be compared (tests/pnp_model.py's two families of variants).

A scene is one candidate: a row of `n` frame keypoints (TUM1 intrinsics, 8 levels at scale 1.2)
whose matched slots are interleaved with -1, negative and out-of-table ids, N of them valid.
"Convention-blind" scenes have keypoints exact up to float rounding and gross outliers; the
others carry 0.5 px of noise."""
from __future__ import annotations

import functools

import numpy as np

import pnp_model as M

K = np.array([517.306408, 516.469215, 318.643040, 255.313989], np.float32)   # TUM1
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float32)
CAP = 512
REF = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991)   # Tracking.cc:1556
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])

# name: seed, N, outlier fraction, pixel noise, convention-blind, parameter overrides, draws, rounds
SCENES = {
    "blind_100": dict(seed=1101, N=100, out=0.2, noise=0.0, blind=True),
    "blind_257": dict(seed=1102, N=257, out=0.2, noise=0.0, blind=True),
    "blind_65": dict(seed=2103, N=65, out=0.2, noise=0.0, blind=True),
    "blind_64": dict(seed=2104, N=64, out=0.2, noise=0.0, blind=True),
    "blind_63": dict(seed=1105, N=63, out=0.2, noise=0.0, blind=True),
    "blind_11": dict(seed=2106, N=11, out=0.1, noise=0.0, blind=True),
    "first_100": dict(seed=1107, N=100, out=0.2, noise=0.0, blind=True, first_clean=True),
    "noisy_100": dict(seed=201, N=100, out=0.2, noise=0.5, blind=False),
    "noisy_63": dict(seed=202, N=63, out=0.2, noise=0.5, blind=False),
    "none_100": dict(seed=301, N=100, out=1.0, noise=0.0, blind=False, params=dict(max_iterations=6)),
    "all_10": dict(seed=302, N=10, out=0.0, noise=0.0, blind=False),          # minInliers == N: one iteration
    "all_4": dict(seed=303, N=4, out=0.0, noise=0.0, blind=False, params=dict(min_inliers=4)),
    "few_9": dict(seed=304, N=9, out=0.0, noise=0.0, blind=False),            # N < minInliers: no iteration
    "few_4": dict(seed=305, N=4, out=0.0, noise=0.0, blind=False),
    "few_3": dict(seed=306, N=3, out=0.0, noise=0.0, blind=False),
    "behind_64": dict(seed=307, N=64, out=0.2, noise=0.0, blind=False, behind=True, params=dict(max_iterations=6)),
    # driven on after a return: the next calls go on from mnIterations, beyond the cap, out of draws
    "cont_100": dict(seed=3401, N=100, out=0.2, noise=0.0, blind=False, plan=(5, 5, 1, 7, 300)),
    # n_draws 10: the third call runs out of draws
    "nodraws_100": dict(seed=403, N=100, out=1.0, noise=0.0, blind=False, params=dict(max_iterations=6), n_draws=10,
                        plan=(5, 3, 5)),
    # iteration 0 and 1 find a decoy pose with exactly minInliers points each (Refine fails once, a tie keeps the
    # earlier iteration and reuses the stored failure), iteration 2 replaces the best state and Refine succeeds
    "staged_100": dict(seed=601, N=100, out=0.0, noise=0.0, blind=False, staged=True,
                       params=dict(epsilon=0.1, min_inliers=10)),
    # degenerate minimal sets at iteration 0 (coplanar points; the same correspondence twice), regular draws after.
    # What such a set's hypothesis is hangs on how a singular matrix is decomposed, so iteration 0 is exempt from the
    # guard's margins; the guard instead requires that it qualifies in no variant, and then nothing that is returned
    # depends on it.
    "coplanar_64": dict(seed=501, N=64, out=0.2, noise=0.0, blind=False, coplanar=True, degenerate=(0,)),
    "repeat_64": dict(seed=502, N=64, out=0.2, noise=0.0, blind=False, repeat=True, degenerate=(0,)),
    # draws out of range cost their iteration only
    "baddraw_64": dict(seed=402, N=64, out=0.2, noise=0.0, blind=False, bad_draws=True),
}
N_DRAWS = 300   # >= max_iterations


def _rodrigues(a):
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


@functools.lru_cache(maxsize=None)
def scene(name: str) -> dict:
    return build(SCENES[name], name)


def _sc(x) -> dict:
    return scene(x) if isinstance(x, str) else x


def build(s: dict, name: str = "") -> dict:
    """The candidate a spec describes (the entries of SCENES are such specs)."""
    rng = np.random.default_rng(s["seed"])
    N = s["N"]
    n = s.get("n", min(CAP, 2 * N + 5))
    R = _rodrigues(rng.normal(size=3) * 0.3)
    t = rng.normal(size=3) * 0.5
    n_mp = N + 40
    # MapPoints in front of the camera (or all behind it), seen inside a 640 x 480 image
    uv = np.stack([rng.uniform(20, 620, n_mp), rng.uniform(20, 460, n_mp)], 1)
    z = rng.uniform(2.0, 9.0, n_mp) * (-1.0 if s.get("behind") else 1.0)
    Xc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], 1)
    pos = ((Xc - t) @ R).astype(np.float32)
    Xc = pos.astype(np.float64) @ R.T + t
    proj = np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1)
    slots = np.sort(rng.choice(n, N, replace=False))
    ids = rng.permutation(n_mp)[:N]
    matches = np.empty(n, np.int32)
    matches[:] = np.array([-1, n_mp + 3, -7, n_mp])[np.arange(n) % 4]
    matches[slots] = ids
    keys = np.zeros(n, KEYPOINT_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    keys["octave"] = rng.integers(0, 8, n)
    keys["octave"][::17] = 9      # clamped into the pyramid
    keys["octave"][5::19] = -1
    keys["size"], keys["angle"], keys["response"], keys["class_id"] = 31.0, rng.uniform(0, 360, n), 50.0, -1
    inl = rng.random(N) >= s["out"]
    if s["out"] == 0.0:
        inl[:] = True
    xy = proj[ids] + rng.normal(size=(N, 2)) * s["noise"]
    keys["x"][slots[inl]], keys["y"][slots[inl]] = xy[inl, 0], xy[inl, 1]
    params = dict(REF, **s.get("params", {}))
    n_draws = s.get("n_draws", N_DRAWS)
    first = min(n_draws, 64)
    draws = np.stack([rng.integers(0, max(1, N - j), first) for j in range(4)], 1).astype(np.int32)
    if n_draws > first:
        more = np.random.default_rng(s["seed"] + 7)
        draws = np.concatenate([draws, np.stack([more.integers(0, max(1, N - j), n_draws - first) for j in range(4)],
                                                1).astype(np.int32)])
    if s.get("first_clean"):   # iteration 0 draws four inliers: the first four in index order, far from each other
        good = np.nonzero(inl)[0][[0, len(np.nonzero(inl)[0]) // 3, 2 * len(np.nonzero(inl)[0]) // 3, -1]]
        avail = list(range(N))
        for j, g in enumerate(good):
            r = avail.index(int(g))
            draws[0, j] = r
            avail[r] = avail[-1]
            avail.pop()
    def force(k, want):   # iteration k draws the correspondences `want`, in this order
        avail = list(range(N))
        for j, g in enumerate(want):
            r = avail.index(int(g))
            draws[k, j] = r
            avail[r] = avail[-1]
            avail.pop()
    if s.get("staged"):    # two decoy poses with 10 correspondences each, the true pose with 50, 30 gross outliers
        groups = (np.arange(0, 10), np.arange(10, 20), np.arange(20, 70))
        poses = ((_rodrigues(rng.normal(size=3) * 0.2) @ R, t + rng.normal(size=3) * 0.3),
                 (_rodrigues(rng.normal(size=3) * 0.2) @ R, t + rng.normal(size=3) * 0.3), (R, t))
        keys["x"][slots], keys["y"][slots] = rng.uniform(0, 640, N), rng.uniform(0, 480, N)
        for grp, (Rg, tg) in zip(groups, poses):
            x = pos[ids[grp]].astype(np.float64) @ Rg.T + tg
            keys["x"][slots[grp]] = K[0] * x[:, 0] / x[:, 2] + K[2]
            keys["y"][slots[grp]] = K[1] * x[:, 1] / x[:, 2] + K[3]
        inl = np.zeros(N, bool)
        inl[groups[2]] = True
        p3, p2 = pos[ids], np.stack([keys["x"][slots], keys["y"][slots]], 1)
        err = (SIGMA2[np.clip(keys["octave"][slots], 0, 7)] * np.float32(params["th2"])).astype(np.float32)
        for k, grp in enumerate(groups):   # iteration k draws four of group k whose hypothesis finds the whole group
            for _ in range(200):
                sel = rng.choice(grp, 4, replace=False)
                Rh, th, _ = M.compute_pose(p3[sel], p2[sel], K)
                if int(M.check_inliers(Rh, th, [np.float64(v) for v in K], p3, p2, err).sum()) == len(grp):
                    break
            else:
                raise AssertionError("no minimal set finds its group")
            force(k, sel)
    if s.get("coplanar"):  # the first four inlier correspondences share a plane in the world; iteration 0 draws them
        e = np.nonzero(inl)[0][:4]
        p = pos[ids[e]].astype(np.float64)
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        nrm /= np.linalg.norm(nrm)
        p[3] -= nrm * ((p[3] - p[0]) @ nrm)
        pos[ids[e[3]]] = p[3].astype(np.float32)
        x = pos[ids[e[3]]].astype(np.float64) @ R.T + t
        keys["x"][slots[e[3]]], keys["y"][slots[e[3]]] = K[0] * x[0] / x[2] + K[2], K[1] * x[1] / x[2] + K[3]
        force(0, e)
    if s.get("repeat"):    # two correspondences with the same MapPoint and keypoint; iteration 0 draws both
        e = np.nonzero(inl)[0][:5]
        matches[slots[e[1]]] = matches[slots[e[0]]]
        keys["x"][slots[e[1]]], keys["y"][slots[e[1]]] = keys["x"][slots[e[0]]], keys["y"][slots[e[0]]]
        force(0, [e[0], e[2], e[1], e[4]])
    if s.get("bad_draws"):
        draws[0, 0] = N
        draws[1, 3] = N - 3
        draws[2, 2] = -1
    return dict(name=name, plan=s.get("plan"), N=N, n=n, keys=keys, matches=matches, pos=pos, n_mp=n_mp, params=params, draws=draws,
                R=R, t=t, inl_slots=slots[inl], blind=s["blind"], degenerate=tuple(s.get("degenerate", ())))


def pack(names, cap=None):
    """The scenes as one batch: rows of `cap` slots, one MapPoint table (`offsets`: each scene's first id)."""
    cap = CAP if cap is None else cap
    B = len(names)
    kps = np.zeros((B, cap), KEYPOINT_DTYPE)
    kps["x"], kps["y"] = 320.0, 240.0
    n = np.zeros(B, np.int32)
    matches = np.zeros((B, cap), np.int32)       # beyond n: id 0, valid, and ignored
    off, pos = 0, []
    scs = [_sc(k) for k in names]
    nd = scs[0]["draws"].shape[0]
    draws = np.zeros((B, nd, 4), np.int32)
    for b, sc in enumerate(scs):
        assert sc["params"] == scs[0]["params"] and sc["draws"].shape[0] == nd
        n[b] = sc["n"]
        kps[b, :sc["n"]] = sc["keys"]
        m = sc["matches"].copy()
        ok = (m >= 0) & (m < sc["n_mp"])
        m[ok] += off                                 # one table for the batch
        m[~ok & (m >= sc["n_mp"])] = 10 ** 6         # stays out of the table
        matches[b, :sc["n"]] = m
        pos.append(sc["pos"])
        off += sc["n_mp"]
        draws[b] = sc["draws"]
    return dict(kps=kps, n=n, matches=matches, pos=np.concatenate(pos), draws=draws, params=scs[0]["params"],
                offsets=np.cumsum([0] + [sc["n_mp"] for sc in scs])[:-1])


def model_for(name, arith="jacobi", conv=None, base=None) -> M.PnPModel:
    sc = _sc(name)
    m = M.PnPModel(np.stack([sc["keys"]["x"], sc["keys"]["y"]], 1), sc["keys"]["octave"], sc["matches"], sc["pos"],
                   SIGMA2, K, arith=arith, conv=conv, base=base)
    m.set_params(sc["draws"], **sc["params"])
    return m


# Two of compute_pose's three solutions usually converge to the same pose, and rep_errors then
# compares two numbers that are equal up to rounding.  Such a comparison (the poses' entries
# closer than pnp_model.SAME_POSE) is not held to the guard's margin; instead family A has the
# variant "flip", which decides every such comparison the other way, so that what the other
# outcome does to every later error2 / mvMaxError is part of the family's spread.
SAME_POSE = M.SAME_POSE
ROUNDS = 8   # at most this many iterate(5) calls per scene


def run_plan(m, step=5, rounds=ROUNDS, plan=None):
    """The outputs of every call of the plan: iterate(k) for each k of `plan`, or iterate(step)
    until a call finds a pose or says no_more."""
    if plan is not None:
        return [m.iterate(k) for k in plan]
    outs = []
    for _ in range(rounds):
        o = m.iterate(step)
        outs.append(o)
        if o["found"] or o["no_more"]:
            break
    return outs


INT_FIELDS = ("found", "no_more", "n_inliers", "refined", "n_corr", "min_inliers_used", "max_its_used", "best_inliers",
              "best_iteration", "iterations", "status")


def _same_ints(a, b, fields):
    return len(a) == len(b) and all(
        all(int(x[f]) == int(y[f]) for f in fields) and np.array_equal(x["inliers"], y["inliers"]) and
        np.array_equal(x["frame_mp"], y["frame_mp"]) for x, y in zip(a, b))


def _margins(traces, skip=()):
    """(the smallest distance of a traced quantity from its threshold, the largest relative
    difference of a traced quantity between the variants); None if the traces differ in shape.
    The entries whose index is in `skip` are left out."""
    base = traces[0]
    if any(len(t) != len(base) for t in traces):
        return None
    margin, spread = np.inf, 0.0
    with np.errstate(all="ignore"):
        for i, e in enumerate(base):
            if i in skip:
                continue
            if e[0] == "err":
                q0 = e[1]
                fin = np.isfinite(q0)
                if fin.any():
                    margin = min(margin, np.abs(q0[fin] - 1.0).min())
                for t in traces[1:]:
                    q = t[i][1]
                    if q.shape != q0.shape or not np.array_equal(np.isfinite(q), fin):
                        return None
                    if fin.any():
                        spread = max(spread, (np.abs(q[fin] - q0[fin]) / np.maximum(np.abs(q0[fin]), 1.0)).max())
            else:
                a0, b0 = e[1], e[2]
                if np.isfinite(a0) and np.isfinite(b0) and not e[3] < SAME_POSE:
                    margin = min(margin, abs(a0 - b0) / max(abs(b0), 1e-300))
                for t in traces[1:]:
                    a, b = t[i][1], t[i][2]
                    if (np.isfinite(a), np.isfinite(b)) != (np.isfinite(a0), np.isfinite(b0)):
                        return None
                    for x, x0 in ((a, a0), (b, b0)):
                        if np.isfinite(x0):
                            spread = max(spread, abs(x - x0) / max(abs(x0), 1e-300))
    return margin, spread


def _tcw_spread(runs, fields=("Tcw", "best_Tcw")):
    d = 0.0
    for r in runs[1:]:
        for x, y in zip(runs[0], r):
            for f in fields:
                a, b = x[f].astype(np.float64), y[f].astype(np.float64)
                fin = np.isfinite(a) & np.isfinite(b)
                if fin.any():
                    d = max(d, np.abs(a[fin] - b[fin]).max())
    return d


def _walk_of(m):
    """How every walked count relates to mRansacMinInliers, and the best-state and Refine events."""
    return [(k, c >= m.min_inliers) for k, c in sorted(m.counts.items())], list(m.events)


@functools.lru_cache(maxsize=None)
def guard_for(name: str) -> dict:
    """Runs the scene's plan under every variant that applies and asserts the guard.  Returns the
    model's outputs (`outs`, the Jacobi variant), `spread_a` (the largest Tcw entry difference
    within family A), and for convention-blind scenes `family_b` (every variant's outputs),
    `spread_b`, and the margin and largest difference of the refined error2 / mvMaxError."""
    sc = scene(name)
    runs, models, basis = [], [], None
    for arith in M.ARITH:
        m = model_for(name, arith=arith, base=basis)
        runs.append(run_plan(m, plan=sc["plan"]))
        models.append(m)
        if basis is None:
            basis = m.basis
    for r in runs[1:]:
        assert _same_ints(runs[0], r, INT_FIELDS), f"{name}: family A disagrees on a count, a flag or a field"
    # every walked count relates to mRansacMinInliers and to the best count alike in all variants
    for m in models[1:]:
        assert _walk_of(m) == _walk_of(models[0]), f"{name}: family A walks the counts differently"
    skip = set()
    for k in sc["degenerate"]:
        for m in models:
            assert m.counts[k] < m.min_inliers, f"{name}: the degenerate iteration {k} qualifies"
        assert len({m.spans[k] for m in models}) == 1, f"{name}: family A walks different comparisons"
        skip.update(range(*models[0].spans[k]))
    ms = _margins([m.trace for m in models], skip)
    assert ms is not None, f"{name}: family A walks different comparisons"
    margin, spread = ms
    assert margin > 1000.0 * spread, f"{name}: a threshold at {margin:.3g}, family A differs by {spread:.3g}"
    out = dict(outs=runs[0], spread_a=_tcw_spread(runs), margin_a=margin, rel_a=spread)
    if sc["blind"]:
        fam, ratios = [], []
        bm = model_for(name)
        base = run_plan(bm, step=300, rounds=1)
        for conv in M.CONVENTIONS:
            m = model_for(name, conv=conv)
            fam.append(run_plan(m, step=300, rounds=1))
            ratios.append(m.refine_ratios)
        for f in fam:
            assert _same_ints([base[-1]], [f[-1]], ("found", "n_inliers")), \
                f"{name}: family B disagrees on found, inliers or n_inliers"
        # every refined error2 / mvMaxError that is reached, in any variant, against the largest difference of
        # the returned Refine's between the variants (relative to the larger of the value and its threshold)
        margin_b, rel_b = np.inf, 0.0
        q0 = bm.refine_ratios[-1] if bm.refine_ratios else None
        with np.errstate(all="ignore"):
            for rs in ratios + [bm.refine_ratios]:
                for q in rs:
                    fin = np.isfinite(q)
                    if fin.any():
                        margin_b = min(margin_b, np.abs(q[fin] - 1.0).min())
                if base[-1]["refined"]:
                    q = rs[-1]
                    fin = np.isfinite(q0)
                    assert np.array_equal(np.isfinite(q), fin), f"{name}: family B differs in what is finite"
                    rel_b = max(rel_b, (np.abs(q[fin] - q0[fin]) / np.maximum(np.abs(q0[fin]), 1.0)).max())
        assert margin_b > 1000.0 * rel_b, f"{name}: a refined threshold at {margin_b:.3g}, family B differs by {rel_b:.3g}"
        out.update(family_b=fam, base_b=base, spread_b=_tcw_spread([base] + fam, ("Tcw",)), margin_b=margin_b,
                   rel_b=rel_b)
    return out
