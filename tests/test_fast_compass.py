"""k_level_tiles' FAST compass pre-test, restated in numpy (no GPU).

The kernel rejects a pixel before the exact 16-arc strength unless two adjacent compass
points (ring 0 (0,+3), 4 (+3,0), 8 (0,-3), 12 (-3,0)) lie beyond t on the same side.  The
adjacent-pair form takes the extrema over the four pairs (0,4), (4,8), (8,12), (12,0) of
the differences a_k = C_k - v.  Every such pair is one vertical point {0, 8} with one
horizontal point {4, 12}, and all four combinations occur, so

    max over pairs of min(a_i, a_j) = min(max(a0, a8), max(a4, a12))
    min over pairs of max(a_i, a_j) = max(min(a0, a8), min(a4, a12))

and the extrema can be taken on the raw pixels with v subtracted once (the opposite-pair
form the kernel evaluates).  Checked here: both forms give the same pass bit, and no
pixel whose exact FAST-9/16 strength M exceeds t fails the test.
"""
import itertools

import numpy as np
import pytest

THRESHOLDS = (0, 1, 7, 20, 254)

# ring k -> (dx, dy), the kernel's order (ring 0 below the centre, then anticlockwise in x)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def pass_adjacent(v, c0, c4, c8, c12, t):
    a0, a4, a8, a12 = c0 - v, c4 - v, c8 - v, c12 - v
    br = np.maximum(np.maximum(np.minimum(a0, a4), np.minimum(a4, a8)),
                    np.maximum(np.minimum(a8, a12), np.minimum(a12, a0)))
    dk = np.minimum(np.minimum(np.maximum(a0, a4), np.maximum(a4, a8)),
                    np.minimum(np.maximum(a8, a12), np.maximum(a12, a0)))
    return np.maximum(br, -dk) - (t + 1) >= 0


def pass_opposite(v, c0, c4, c8, c12, t):
    br = np.minimum(np.maximum(c0, c8), np.maximum(c4, c12))
    dk = np.maximum(np.minimum(c0, c8), np.minimum(c4, c12))
    return np.maximum(br - v, v - dk) - (t + 1) >= 0


def strength(patches):
    """Exact FAST-9/16 strength M of the centre of (N, 7, 7) patches: the maximum over the
    16 contiguous 9-arcs of max(min(ring - v), min(v - ring)), at least 0."""
    p = patches.astype(np.int32)
    v = p[:, 3, 3]
    d = np.stack([p[:, 3 + dy, 3 + dx] for dx, dy in RING], axis=1) - v[:, None]
    best = np.zeros(len(p), np.int32)
    for s in range(16):
        arc = d[:, [(s + i) & 15 for i in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=1), (-arc).min(axis=1)))
    return best


def compass_of(patches):
    p = patches.astype(np.int32)
    return p[:, 3, 3], p[:, 6, 3], p[:, 3, 6], p[:, 0, 3], p[:, 3, 0]


@pytest.mark.parametrize("t", THRESHOLDS)
def test_forms_agree_on_critical_differences(t):
    vals = sorted({-t - 1, -t, -1, 0, 1, t, t + 1})
    a = np.array(list(itertools.product(vals, repeat=4)), np.int32)
    for v in (0, 128, 255):  # the identity is in the differences; any centre gives the same bits
        c = [a[:, k] + v for k in range(4)]
        old, new = pass_adjacent(v, *c, t), pass_opposite(v, *c, t)
        assert np.array_equal(old, new), a[np.nonzero(old != new)[0][:5]]
    assert old.any() and not old.all()


def test_forms_agree_on_random_bytes():
    rng = np.random.default_rng(7)
    v, c0, c4, c8, c12 = rng.integers(0, 256, (5, 1_000_000), dtype=np.int32)
    for t in THRESHOLDS:
        old, new = pass_adjacent(v, c0, c4, c8, c12, t), pass_opposite(v, c0, c4, c8, c12, t)
        assert np.array_equal(old, new), (t, np.nonzero(old != new)[0][:5])


def _arc_patches():
    """Patches whose 9-arc starts on each ring position, bright and dark, the arc exactly
    d beyond the centre and the other ring pixels at, just inside, or opposite to it."""
    out = []
    for s, sign, d, rest in itertools.product(range(16), (1, -1), (1, 2, 8, 21, 100), (0, 1, -1)):
        v = 128
        p = np.full((7, 7), v, np.int32)
        for k, (dx, dy) in enumerate(RING):
            in_arc = ((k - s) & 15) < 9
            p[3 + dy, 3 + dx] = v + sign * d if in_arc else v + sign * (d - 1) * (rest == 1) - sign * d * (rest == -1)
        out.append(p)
    return np.clip(np.array(out), 0, 255).astype(np.uint8)


def test_no_corner_fails_the_compass_test():
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, (100_000, 7, 7), dtype=np.uint8)
    # low-contrast noise as well: byte noise almost never has a strong arc
    soft = (128 + rng.integers(-12, 13, (100_000, 7, 7))).astype(np.uint8)
    for name, patches in (("random", noise), ("soft", soft), ("arcs", _arc_patches())):
        M = strength(patches)
        v, c0, c4, c8, c12 = compass_of(patches)
        for t in (0, 1, 7, 20, 99):
            corner = M > t
            ok = pass_opposite(v, c0, c4, c8, c12, t)
            assert not (corner & ~ok).any(), (name, t, np.nonzero(corner & ~ok)[0][:5])
        if name != "random":
            assert (M > 7).any(), name  # the property is exercised, not vacuous
    M = strength(_arc_patches())
    assert (M > 20).sum() >= 16 * 2  # every start position, both signs
