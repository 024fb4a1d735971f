"""Hand-built stereo pairs for Frame::ComputeStereoMatches (Frame.cc:673-885): keypoints and
descriptors chosen by hand on small images, so that the row-band search, the SAD refinement
and the in-loop outlier pass each meet the edges that extracted ORB keypoints never reach.
numpy only; test_stereo_edge_scenes.py shows with the CPU oracle and an instrumented mirror
of its loop that every scene reaches what its name says, test_gpu_stereo_edges.py runs them
on the GPU.

A *base* is one image pair with its right keypoints and a table of *sites*: a site is one
possible left keypoint (position, octave, descriptor) with a designed outcome, named by its
kind.  A scene is a base plus a sequence of site indices, with repeats: the left keypoint
list.  The outlier pass consumes the sequence of (pushed, SAD) the left keypoints produce,
so any such sequence of any length comes from one small image, and every scene of a base
shares its pyramids.

The right image is the left one 7 px further along one canvas of noise in 40..120, so a
right keypoint at (x - 7, y) under a left keypoint at (x, y) has SAD 0 at shift 0 on level
0; `+v` on one non-centre pixel of that right window makes the SAD exactly v.  Other sites
carry their own patch in both images.

Scene(left, right, keys_l, desc_l, keys_r, desc_r, params, max_disparity, bf) unpacks as
that 9-tuple and also carries .name, .base, .site (site index of every left keypoint) and
.kinds (kind -> left keypoint indices).
"""
import functools
from collections import namedtuple

import numpy as np

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
W0, H0 = 416, 240
SHIFT = 7            # the canvas shift: true disparity of the plain sites
BF = 386.1448
MAX_D = 64.0         # default max_disparity of the hand scenes
TH_ORB = 75          # thOrbDist = (TH_HIGH + TH_LOW) / 2
LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049, 4097, 8191, 8192)
F32 = np.float32

_Scene = namedtuple("Scene", "left right keys_l desc_l keys_r desc_r params max_disparity bf")


class Scene(_Scene):
    """The 9-tuple plus attributes (name, base, site, kinds)."""


def scale_factors(nlevels, factor=1.2):
    """mvScaleFactor (ORBextractor.cc:417-426) as the oracle and the extractor hold it: float products."""
    sf = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        sf[i] = sf[i - 1] * F32(factor)
    return sf


def level_sizes(W, H, sf):
    """(w, h) of every level: cvRound((float)cols * mvInvScaleFactor[l]) (ORBextractor.cc:1637-1640)."""
    inv = F32(1) / sf
    return [(int(np.rint(F32(W) * inv[l])), int(np.rint(F32(H) * inv[l]))) for l in range(len(sf))]


def roundf(v):
    """C roundf of a float32: half away from zero, keeping the sign of zero."""
    v = float(F32(v))
    return float(np.copysign(np.floor(abs(v) + 0.5), v))


def band(y, octave, sf):
    """Rows floor(y - r) .. ceil(y + r), r = 2 mvScaleFactors[octave], in float (cc:697-703)."""
    r = F32(2) * sf[octave]
    return int(np.floor(F32(y) - r)), int(np.ceil(F32(y) + r))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class Base:
    def __init__(self, name, W=W0, H=H0, nlevels=8, seed=0, stripes=False):
        self.name, self.W, self.H, self.nlevels = name, W, H, nlevels
        self.params = (1000, 1.2, nlevels, 20, 7)
        self.sf = scale_factors(nlevels)
        self.inv = F32(1) / self.sf
        self.sizes = level_sizes(W, H, self.sf)
        self.rng = np.random.default_rng(seed)
        if stripes:
            # columns of noise, every other 8 rows 6 brighter: texture along x and y without one
            # FAST corner (a column gives an arc of 7, the step is under minThFAST), so a frame of
            # several megapixels keeps the extractor's octree far from its node capacity
            canvas = np.repeat(self.rng.integers(40, 115, (1, W + SHIFT)), H, axis=0)
            canvas = (canvas + 6 * (np.arange(H)[:, None] % 16 >= 8)).astype(np.uint8)
        else:
            canvas = self.rng.integers(40, 121, (H, W + SHIFT)).astype(np.uint8)
        self.left = canvas[:, :W].copy()
        self.right = canvas[:, SHIFT:].copy()
        self.kr = []          # right keypoints (x, y, octave, desc)
        self.sites = []       # possible left keypoints (x, y, octave, desc)
        self.kind = {}        # kind -> site indices
        self._final = None

    # ---- building blocks
    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    @staticmethod
    def flip(d, bits):
        """d with the given bit positions (0..255) flipped."""
        b = np.unpackbits(d)
        b[list(bits)] ^= 1
        return np.packbits(b)

    def right_kp(self, x, y, octave, d):
        self.kr.append((F32(x), F32(y), int(octave), d))
        return len(self.kr) - 1

    def site(self, kind, x, y, octave, d):
        self.sites.append((F32(x), F32(y), int(octave), d))
        self.kind.setdefault(kind, []).append(len(self.sites) - 1)
        return len(self.sites) - 1

    def bump(self, x, y, v):
        """SAD v for the level-0 right window centred (x, y): +v spread over non-centre pixels."""
        for dx, dy in ((1, 0), (2, 1), (-3, 2), (4, -2)):
            a = min(v, 80)
            self.right[y + dy, x + dx] += a
            v -= a
        assert v == 0 and self.right.max() <= 200

    def patch(self, y, xl, xr, sym=False):
        """One random patch in the left image centred (xl, y) and in the right centred (xr, y):
        11 rows, 11 columns, or 23 mirror-symmetric columns (equal SAD at shifts +k and -k)."""
        if sym:
            half = self.rng.integers(40, 121, (11, 12)).astype(np.uint8)
            p = np.concatenate([half[:, :0:-1], half], axis=1)       # 23 columns, symmetric about the 12th
        else:
            p = self.rng.integers(40, 121, (11, 11)).astype(np.uint8)
        h = p.shape[1] // 2
        self.left[y - 5:y + 6, xl - h:xl + h + 1] = p
        self.right[y - 5:y + 6, xr - h:xr + h + 1] = p

    def pair(self, kind, x, y, octave=0, dx=-SHIFT, bits=()):
        """A site at (x, y) and its right keypoint at (x + dx, y) with the same descriptor, the
        site's with `bits` flipped."""
        d = self.desc()
        self.right_kp(F32(x) + F32(dx), y, octave, d)
        return self.site(kind, x, y, octave, self.flip(d, bits) if len(bits) else d)

    # ---- the arrays
    def keys_r(self):
        return _keys([(x, y, o) for x, y, o, _ in self.kr]), _descs([d for *_, d in self.kr])

    def scene(self, name, seq, max_disparity=MAX_D, n_right=None):
        seq = np.asarray(seq, np.int64).reshape(-1)
        kr, dr = self.keys_r()
        if n_right is not None:
            kr, dr = kr[:n_right], dr[:n_right]
        kl = _keys([self.sites[i][:3] for i in range(len(self.sites))])
        dl = _descs([s[3] for s in self.sites])
        s = Scene(self.left, self.right, kl[seq], dl[seq], kr, dr, self.params, float(max_disparity), BF)
        s.name, s.base, s.site = name, self, seq
        s.kinds = {k: np.nonzero(np.isin(seq, v))[0] for k, v in self.kind.items()}
        check_windows(s)
        return s

    def all_sites(self):
        return np.arange(len(self.sites))


def _keys(rows):
    k = np.zeros(len(rows), KEYPOINT_DTYPE)
    for i, (x, y, o) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
    k["size"] = 31.0
    k["angle"] = 0.0
    k["class_id"] = -1
    return k


def _descs(ds):
    return np.stack(ds).astype(np.uint8) if len(ds) else np.zeros((0, 32), np.uint8)


def check_windows(s):
    """The condition on every scene: the reference reads the 11 x 11 SAD windows unchecked, so
    for every left keypoint and every right keypoint it could take (octave within one, band
    over its row, u in [minU, maxU], Hamming distance under 75) either the iniu / endu test
    fires or the left window and the right windows of all 11 shifts lie inside the level.
    A superset of what the search reaches, over the distinct left keypoints."""
    b = s.base
    if len(s.keys_l) == 0 or len(s.keys_r) == 0:
        return
    kr = s.keys_r
    lo = np.array([band(k["y"], k["octave"], b.sf)[0] for k in kr])
    hi = np.array([band(k["y"], k["octave"], b.sf)[1] for k in kr])
    maxd = F32(s.max_disparity)
    for i in np.unique(s.site):
        x, y, o, d = b.sites[i]
        assert 0 <= int(y) < b.H and 0 <= o < b.nlevels, ("left keypoint outside the pyramid", i)
        row = int(y)
        cand = (np.abs(kr["octave"] - o) <= 1) & (lo <= row) & (hi >= row) & (kr["x"] >= x - maxd) & (kr["x"] <= x)
        for iR in np.nonzero(cand)[0]:
            if hamming(d, s.desc_r[iR]) >= TH_ORB:
                continue
            w, h = b.sizes[o]
            ul, vl, ur = roundf(x * b.inv[o]), roundf(y * b.inv[o]), roundf(kr["x"][iR] * b.inv[o])
            assert 0 <= int(ul) < w and 0 <= int(vl) < h, ("centre pixel", i)      # read before the test
            if ur + 5 - 5 < 0 or ur + 5 + 5 + 1 >= w:
                continue
            ok = int(vl) - 5 >= 0 and int(vl) + 5 < h and int(ul) - 5 >= 0 and int(ul) + 5 < w and \
                int(ur) - 10 >= 0 and int(ur) + 10 < w
            assert ok, ("SAD window leaves the level", s.name, i, int(iR))


# ------------------------------------------------------------------ the level-0 lattice base

def _cells(W, H):
    return [(x, y) for y in range(10, H - 10, 12) for x in range(40, W - 24, 32)]


NDIST = 160   # sites "dist" k = 0..159 have SAD exactly k


@functools.lru_cache(maxsize=None)
def sad_base():
    """416x240, 8 levels, every keypoint at octave 0 on a 32x12 px lattice.  Kinds:
    dist (160 sites, SAD k), nomatch (reaches the outlier pass, pushes nothing), incR-L /
    incR+L (right keypoint 5 px off: the border shift wins, `continue`), h74 / h75 / h99 /
    h100 (best Hamming distance), tie2a / tie2b / tie3 (equal best distances; the lowest iR
    sits in the higher (octave, row) bucket and is the true correspondence in a, 5 px off in
    b), closer_out (an identical descriptor just right of maxU), clamp0 (uR == maxU,
    disparity 0 on a symmetric patch: the 0.01 clamp), umax_out (uR one float above maxU),
    umin_out (uR one float below uL - 7: outside at max_disparity 7 only), negdisp (uR0 == uL,
    best shift +2), xneg (left x < 0), iniu (right x rounds to -1), endu_eq (endu == cols),
    endu_in (endu == cols - 1, windows inside)."""
    b = Base("sad", seed=11)
    cells = _cells(b.W, b.H)
    assert len(cells) >= NDIST + 24
    for k in range(NDIST):
        x, y = cells[k]
        b.pair("dist", x, y)
        b.bump(x - SHIFT, y, k)
    it = iter(cells[NDIST:])
    for _ in range(2):
        x, y = next(it)
        b.right_kp(x - SHIFT, y, 0, b.desc())
        b.site("nomatch", x, y, 0, b.desc())
    x, y = next(it)
    b.pair("incR-L", x, y, dx=-SHIFT + 5)
    x, y = next(it)
    b.pair("incR+L", x, y, dx=-SHIFT - 5)
    for nb in (74, 75, 99, 100):
        x, y = next(it)
        b.pair("h%d" % nb, x, y, bits=range(nb))
        b.bump(x - SHIFT, y, 5)
    # ties: A (lowest iR) in the higher bucket, B (and C) in lower ones, all 10 bits away
    for kind, xa, xb in (("tie2a", -SHIFT, -SHIFT + 5), ("tie2b", -SHIFT + 5, -SHIFT)):
        x, y = next(it)
        d = b.desc()
        b.right_kp(x + xa, y + 1, 0, b.flip(d, range(0, 10)))
        b.right_kp(x + xb, y - 1, 0, b.flip(d, range(10, 20)))
        b.site(kind, x, y, 0, d)
    x, y = next(it)
    d = b.desc()
    b.right_kp(x - SHIFT, y, 1, b.flip(d, range(0, 10)))            # octave 1: the last bucket scanned
    b.right_kp(x - SHIFT + 5, y + 1, 0, b.flip(d, range(10, 20)))
    b.right_kp(x - SHIFT - 5, y - 1, 0, b.flip(d, range(20, 30)))
    b.site("tie3", x, y, 0, d)
    x, y = next(it)
    d = b.desc()
    b.right_kp(x - SHIFT, y, 0, b.flip(d, range(10)))
    b.right_kp(np.nextafter(F32(x), F32(1e9)), y, 0, d)            # distance 0, one float right of maxU
    b.site("closer_out", x, y, 0, d)
    x, y = next(it)
    b.patch(y, x, x, sym=True)
    b.pair("clamp0", x, y, dx=0)
    x, y = next(it)
    b.patch(y, x, x, sym=True)
    d = b.desc()
    b.right_kp(np.nextafter(F32(x), F32(1e9)), y, 0, d)
    b.site("umax_out", x, y, 0, d)
    x, y = next(it)
    d = b.desc()
    b.right_kp(np.nextafter(F32(x - SHIFT), F32(-1e9)), y, 0, d)
    b.site("umin_out", x, y, 0, d)
    x, y = next(it)
    b.patch(y, x, x + 2)
    b.pair("negdisp", x, y, dx=0)
    # off the lattice, on lattice rows
    y0, y1, y2 = cells[0][1], cells[11][1], cells[22][1]
    b.site("xneg", -1.0, y0, 0, b.desc())
    d = b.desc()
    b.right_kp(-0.6, y0, 0, d)
    b.site("iniu", 5.0, y0, 0, d)
    b.patch(y1, 410, 405)
    d = b.desc()
    b.right_kp(405.0, y1, 0, d)
    b.site("endu_eq", 410.0, y1, 0, d)
    b.patch(y2, 410, 404)
    d = b.desc()
    b.right_kp(404.0, y2, 0, d)
    b.site("endu_in", 410.0, y2, 0, d)
    # the random descriptors really are far from each other
    dr = _descs([k[3] for k in b.kr])
    for i in b.kind["nomatch"]:
        assert min(hamming(b.sites[i][3], r) for r in dr) >= TH_ORB
    return b


def _dist(b):
    return np.array(b.kind["dist"])


def sad_scene():
    """Every site of the lattice base once, in table order, max_disparity 64."""
    b = sad_base()
    return b.scene("sad", b.all_sites())


def sad_scene_max_d7():
    """The same at max_disparity 7.0: every plain right keypoint sits exactly on minU, and the
    sub-pixel disparity 7 - deltaR falls on both sides of max_disparity."""
    b = sad_base()
    return b.scene("sad_max_d7", b.all_sites(), max_disparity=7.0)


# ------------------------------------------------------------------ outlier sequences

def equality_median():
    """(m, e): the smallest median m >= 5 whose threshold 1.5f * 1.4f * m is an integer e as float."""
    for m in range(5, 60):
        th = F32(F32(1.5) * F32(1.4)) * F32(m)
        if float(th) == int(th):
            return m, int(th)
    raise AssertionError("no exact threshold")


def _mix(n, seed):
    """n left keypoints: mostly SAD 8..40, one in six 60..159, one in ten non-pushing (reaching
    or not), in random order."""
    b = sad_base()
    rng = np.random.default_rng(seed)
    D = _dist(b)
    small = D[rng.integers(8, 41, n)]
    large = D[rng.integers(60, NDIST, n)]
    other = np.array(b.kind["nomatch"] + b.kind["incR-L"] + b.kind["xneg"])[rng.integers(0, 4, n)]
    u = rng.random(n)
    return np.where(u < 0.1, other, np.where(u < 0.1 + 1 / 6, large, small))


def _holes(seq, period):
    """seq with non-pushing left keypoints on every multiple of `period` and the index before:
    the last iteration of one chunk (segment) and the first of the next."""
    b = sad_base()
    nm, sk = b.kind["nomatch"][0], b.kind["incR-L"][0]
    seq = np.array(seq)
    i = np.arange(len(seq))
    seq[(i % period == 0)] = nm
    seq[(i % period == period - 1)] = sk
    return seq


def outlier_names():
    names = ["const", "ascending", "descending", "alternating", "zero_prefix", "equality", "none", "one", "two",
             "empty_start", "chunk_holes_100", "chunk_holes_1025", "segment_holes_2049", "segment_holes_4097"]
    return names + ["len_%d" % n for n in LENGTHS]


def outlier_scene(name):
    b = sad_base()
    D = _dist(b)
    nm, sk = b.kind["nomatch"][0], b.kind["incR-L"][0]
    if name == "const":
        seq = [D[20]] * 40
    elif name == "ascending":
        seq = list(D[1:31]) + list(D[100:])       # the jump marks itself until the median climbs
    elif name == "descending":
        seq = list(D[:129:-1]) + list(D[60:0:-1])  # the large ones fall once the small outnumber them
    elif name == "alternating":
        seq = [D[5], D[150]] * 15 + [D[5]] * 2 + [D[150], D[5]] * 15   # marked by the next push, then by their own
    elif name == "zero_prefix":
        seq = [D[0]] * 5 + [D[10 + i] for i in range(100)]
    elif name == "equality":
        m, e = equality_median()
        seq = [D[m]] * 6 + [D[e - 1], D[e], D[e + 1]] + [D[m]] * 2
    elif name == "none":
        seq = [nm, sk, nm, b.kind["xneg"][0]]
    elif name == "one":
        seq = [nm, D[5], sk]
    elif name == "two":
        seq = [D[50], nm, D[5]]
    elif name == "empty_start":
        seq = [nm] * 5 + [sk] * 3 + [nm] + list(_mix(60, 3))
    elif name == "chunk_holes_100":
        seq = _holes(_mix(100, 4), 7)            # ceil(100 / 16)
    elif name == "chunk_holes_1025":
        seq = _holes(_mix(1025, 5), 65)          # ceil(1025 / 16)
    elif name == "segment_holes_2049":
        seq = _holes(_mix(2049, 6), 3)           # ceil(2049 / 1024)
    elif name == "segment_holes_4097":
        seq = _holes(_mix(4097, 7), 5)           # ceil(4097 / 1024)
    elif name.startswith("len_"):
        n = int(name[4:])
        seq = _mix(n, 100 + n)
        if n <= 2:
            seq = [D[50], D[5]][:n]
    else:
        raise KeyError(name)
    return b.scene("outlier_" + name, seq)


# ------------------------------------------------------------------ band scenes

@functools.lru_cache(maxsize=None)
def band_base():
    """416x240, 8 levels.  Per octave o one right keypoint near row 120 (octave 0: integer y,
    r = 2 exactly; octaves 1-7: y = level row x scale in float) and left keypoints with its
    descriptor on the rows floor(y - r) and ceil(y + r) (kind edge<o>), one row beyond each
    (beyond<o>), at octaves o +- 1 (near<o>) and o +- 2 (far<o>) on its own row; right keypoints
    above and below the image whose band reaches rows 0 / 1 and 238 / 239 (top_in, bot_in:
    the row index clamps them; their x rounds below 0 on the level, so iniu fires) or does
    not (top_out, bot_out); empty (a row no band covers)."""
    b = Base("band", seed=12)
    for o in range(8):
        s = b.sf[o]
        xl = int(round((60 + 40 * o) / float(s)))
        x = F32(xl) * s
        yR = F32(int(round(120 / float(s)))) * s
        d = b.desc()
        b.right_kp(x - F32(SHIFT), yR, o, d)
        lo, hi = band(yR, o, b.sf)
        frac = 0.0 if o == 0 else 0.3
        for kind, row in (("edge", lo), ("edge", hi), ("beyond", lo - 1), ("beyond", hi + 1)):
            b.site("%s%d" % (kind, o), x, row + frac, o, d)
        for kind, ol in (("near", o - 1), ("near", o + 1), ("far", o - 2), ("far", o + 2)):
            if 0 <= ol < 8:
                b.site("%s%d" % (kind, o), x, int(yR) + frac, ol, d)
    # above / below the image: x = -scale rounds to -1 on the keypoint's level
    for kind, y, o, rows in (("top_in", -1.0, 0, (0, 1)), ("top_out", -3.0, 0, (0,)),
                             ("top_in", -F32(2) * b.sf[5], 5, (0,)), ("top_in", -4.0, 7, (0, 3, 4)),
                             ("top_out", -9.0, 7, (0,)),
                             ("bot_in", 240.0, 0, (238, 239)), ("bot_out", 243.0, 0, (239,)),
                             ("bot_in", 243.5, 6, (237,)), ("bot_out", 248.0, 6, (239,))):
        d = b.desc()
        b.right_kp(-b.sf[o], y, o, d)
        for row in rows:
            b.site(kind, 5.0, row + 0.25, o, d)
    b.site("empty", 200.0, 40.0, 0, b.desc())
    b.site("empty", 200.0, 200.25, 3, b.desc())
    return b


def band_scene():
    """Every site once, the top octave first (an octave-0 SAD of 0 pushed first would be the
    median and mark everything)."""
    b = band_base()
    return b.scene("band", b.all_sites()[::-1])


# ------------------------------------------------------------------ geometry scenes

@functools.lru_cache(maxsize=None)
def levels_base(W, H, nlevels):
    """Sites at every octave on a 32x12 lattice of the level (up to 12 per octave), the right
    keypoint 7 px to the left at the same octave: the outcome above level 0 is whatever the
    resized noise gives, checked by the mirror, not designed."""
    b = Base("levels_%dx%d_%d" % (W, H, nlevels), W, H, nlevels, seed=13 + nlevels, stripes=W * H > 2_000_000)
    for o in range(nlevels):
        w, h = b.sizes[o]
        cells = [(xl, yl) for yl in range(8, h - 6, 12) for xl in range(20, w - 12, 32)]
        step = max(1, len(cells) // 12)
        for xl, yl in cells[::step][:12]:
            b.pair("oct%d" % o, F32(xl) * b.sf[o], F32(yl) * b.sf[o], o)
            if o == 0:
                b.bump(xl - SHIFT, yl, 300)       # beside the SAD of the resized levels, not 0
    return b


# 12 levels at 1280 rows: 66,568 bytes of row index in k_stereo_index (over 64 KB); at 2953 rows the
# 153,564 bytes that are the most it takes.  The widths are what the extractor needs to build the
# pyramids: it refuses a level whose octree would have round(width / height) = 0 root nodes.
LEVELS = ((W0, H0, 2), (W0, H0, 8), (832, 1280, 12), (1664, 2953, 12))


def levels_scene(W, H, nlevels):
    """Top octave first, so that the first medians come from the resized levels."""
    b = levels_base(W, H, nlevels)
    return b.scene(b.name, b.all_sites()[::-1])


def no_right_scene():
    b = sad_base()
    return b.scene("n_right_0", _dist(b)[:30], n_right=0)


def no_left_scene():
    b = sad_base()
    return b.scene("n_left_0", [])


def all_scenes():
    """(name, builder) of every hand scene."""
    out = [("sad", sad_scene), ("sad_max_d7", sad_scene_max_d7), ("band", band_scene),
           ("n_right_0", no_right_scene), ("n_left_0", no_left_scene)]
    out += [("levels_%dx%d_%d" % g, functools.partial(levels_scene, *g)) for g in LEVELS]
    out += [("outlier_" + n, functools.partial(outlier_scene, n)) for n in outlier_names()]
    return out
