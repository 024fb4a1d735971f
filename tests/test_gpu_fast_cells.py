"""k_fast_cells (dword staging of each FAST window) against the oracle, keypoints byte for
byte and descriptors exactly, at the smallest shapes where its staging can go wrong:
window origins of every residue mod 4, windows wider than 32 px, the widest window the
cell grid produces, last columns / rows of cells clipped to windows 1 to 3 px wide / tall
(and to no rows at all), both workgroup placements, and a row stride.  The frames are
noise (every cell holds far more than 256 candidates: the full list), flat (every load
step skipped) or a faint texture (cells that are empty at iniThFAST and not at minThFAST).
A lost, extra or misordered candidate changes the octree's output.

Each shape's claim is asserted from the reference's cell grid (ORBextractor.cc:1025-1085),
recomputed here, so a shape that stops covering its case fails instead of passing.

Threshold pairs whose minimum is 0 (the map keeps M = 1, which is no candidate) are
accepted by init_params and are covered below.
"""
import ctypes as C
import math

import numpy as np
import pytest

from orbslam2commentedbyxcm_amd import ORBextractor
from orbslam2commentedbyxcm_amd import _lib as L

pytestmark = pytest.mark.gpu

BUDGET = 5000  # far above what the small frames yield: the octree discards little


def _axis(size, skip):
    """Detection windows (origin, length) of one axis of a level `size` px long: the cell
    loop of cc:1025-1085 (skip = 6 for columns, 3 for rows), window = cell minus 3 px a side."""
    min_b, max_b = 16, size - 19 + 3
    span = max_b - min_b
    n = span // 30
    if n <= 0:
        return 0, []
    cell = math.ceil(span / n)
    out = []
    for j in range(n):
        ini = min_b + j * cell
        end = ini + cell + 6
        if ini >= max_b - skip:
            continue
        end = min(end, max_b)
        out.append((ini + 3, end - ini - 6))
    return cell, out


def _cols(w):
    return _axis(w, 6)


def _rows(h):
    return _axis(h, 3)


def _noise(B, W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W), dtype=np.uint8)


def _texture(W, H, seed, amp):
    """Smooth background with sparse faint dots: corners of contrast around `amp`."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 120, np.int32)
    n = W * H // 600
    ys, xs = rng.integers(3, H - 3, n), rng.integers(3, W - 3, n)
    img[ys, xs] += rng.integers(amp // 2, 2 * amp, n)
    return img.astype(np.uint8)


def _cmp(kp_gpu, desc_gpu, kp_ref, desc_ref, what):
    assert len(kp_gpu) == len(kp_ref), (what, len(kp_gpu), len(kp_ref))
    assert kp_gpu.tobytes() == kp_ref.tobytes(), what
    assert (desc_gpu == desc_ref).all(), what


_REF = {}


def _ref(oracle, key, img, prm):
    """The oracle's extraction of a frame, computed once per (frame, parameters)."""
    k = (key, prm)
    if k not in _REF:
        _REF[k] = oracle.extract(img, oracle.params(*prm))[:2]
    return _REF[k]


def _check(oracle, key, frames, prm):
    ex = ORBextractor(*prm)
    kps, desc, n = ex.extract_batch(frames)
    total = 0
    for b in range(frames.shape[0]):
        kr, dr = _ref(oracle, (key, b), frames[b], prm)
        _cmp(kps[b][: n[b]], desc[b][: n[b]], kr, dr, f"{key} frame {b}")
        total += len(kr)
    return total


def test_origin_residues_and_wide_windows(oracle, orbx_built):
    """156 x 156, 4 levels: level 0 has 31-px cells whose window origins 19, 50, 81, 112 take
    every residue mod 4; level 1 (130 px) a window wider than 32; level 3 (90 px) a single
    58-px cell (window 52 px: the level's border clips it)."""
    prm = (BUDGET, 1.2, 4, 20, 7)
    sizes = oracle.level_sizes(oracle.params(*prm), 156, 156)
    assert [s[0] for s in sizes] == [156, 130, 108, 90]
    cell, wins = _cols(156)
    assert cell == 31 and [o for o, _ in wins] == [19, 50, 81, 112]
    assert sorted(o % 4 for o, _ in wins) == [0, 1, 2, 3]
    cell, wins = _cols(130)
    assert cell == 33 and max(w for _, w in wins) > 32
    cell, wins = _cols(90)
    assert cell == 58 and wins == [(19, 52)]
    assert _check(oracle, "156", _noise(2, 156, 156, 1), prm) > 100


def test_widest_window(oracle, orbx_built):
    """91 x 91: one cell 59 px wide, the widest the grid produces (a level 92 px wide has two
    columns).  Its window is 53 px from column 19: 56 of the 64 staged bytes."""
    prm = (BUDGET, 1.2, 2, 20, 7)
    widest = max((w for size in range(62, 2000) for _, w in _cols(size)[1]), default=0)
    cell, wins = _cols(91)
    assert cell == 59 and wins == [(19, 53)] and widest == 53
    assert 19 % 4 + 53 + 1 <= 64
    assert _check(oracle, "91", _noise(2, 91, 91, 2), prm) > 20


@pytest.mark.parametrize("W,last", [(783, 1), (723, 3)])
def test_last_column_clipped(oracle, orbx_built, W, last):
    """The smallest widths whose last column of cells is clipped to a window 1 / 3 px wide."""
    _, wins = _cols(W)
    assert wins[-1][1] == last
    assert _check(oracle, f"w{W}", _noise(1, W, 100, W), (BUDGET, 1.2, 2, 20, 7)) > 100


@pytest.mark.parametrize("H,last", [(783, 1), (723, 3), (813, 0)])
def test_last_row_clipped(oracle, orbx_built, H, last):
    """The same for the last row of cells: windows 1 and 3 px tall, and a last row of cells
    6 px tall whose window has no row at all (the reference still visits it)."""
    _, wins = _rows(H)
    assert wins[-1][1] == last
    assert _check(oracle, f"h{H}", _noise(1, 440, H, H), (BUDGET, 1.2, 2, 20, 7)) > 100


@pytest.mark.parametrize("B", [8, 3])
def test_placements(oracle, orbx_built, B):
    """640 x 480 x 8 levels: a batch of 8 takes the XCD-aware placement, 3 the plain one."""
    frames = _noise(8, 640, 480, 11)[:B]
    assert _check(oracle, "vga", frames, (1000, 1.2, 8, 20, 7)) > 900 * B


def test_flat_frame(oracle, orbx_built):
    """No candidate anywhere: every load step is skipped."""
    assert _check(oracle, "flat", np.full((1, 156, 156), 128, np.uint8), (BUDGET, 1.2, 4, 20, 7)) == 0


@pytest.mark.parametrize("ini,mn", [(40, 15), (12, 3), (20, 0), (0, 20)])
def test_threshold_pairs(oracle, orbx_built, ini, mn):
    """Noise at other threshold pairs; with a minimum of 0 the map keeps M = 1, which
    cv::FAST(t = 0) scores 0 and non-max suppression never keeps."""
    assert _check(oracle, "333", _noise(1, 333, 257, 5), (BUDGET, 1.2, 3, ini, mn)) > 100


@pytest.mark.parametrize("ini,mn", [(40, 15), (12, 3), (20, 0)])
def test_cells_falling_back_to_min_threshold(oracle, orbx_built, ini, mn):
    """A faint texture on which some level-0 cells are empty at iniThFAST and not at
    minThFAST, others not empty at iniThFAST, and some empty at both."""
    img = _texture(333, 257, 9, ini)
    _, both = oracle.level_candidates_cells(img, oracle.params(BUDGET, 1.2, 1, ini, mn))
    _, at_ini = oracle.level_candidates_cells(img, oracle.params(BUDGET, 1.2, 1, ini, ini))
    assert len(both) == len(at_ini)
    assert ((at_ini == 0) & (both > 0)).any() and (at_ini > 0).any()
    assert _check(oracle, f"tex{ini}", img[None], (BUDGET, 1.2, 3, ini, mn)) > 20


def test_row_stride(oracle, orbx_built):
    """A 157 x 131 noise frame inside a 192-byte-pitch buffer (orbx_extract's `stride`)."""
    img = _noise(1, 157, 131, 13)[0]
    buf = np.zeros((131, 192), np.uint8)
    buf[:, :157] = img
    prm = (BUDGET, 1.2, 3, 20, 7)
    ex = ORBextractor(*prm)
    cap = ex.max_keypoints(157, 131)
    kps = np.zeros(cap, dtype=L.KEYPOINT_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = C.c_int()
    L.check(L.lib().orbx_extract(ex._h, L.u8ptr(buf), 157, 131, 192, kps.ctypes.data, L.u8ptr(desc), cap,
                                 C.byref(n)))
    kr, dr = _ref(oracle, "stride", img, prm)
    _cmp(kps[: n.value], desc[: n.value], kr, dr, "stride")
    assert len(kr) > 50
