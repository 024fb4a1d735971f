"""What make_plan precomputes for k_fast_cells' dword staging (CellGeom, orbx_geometry.h):
the aligned source offset and the byte masks of a window's first and last dword, each
checked against the per-byte test the kernel evaluated before (byte lies in the window iff
0 <= column < wc), the condition that a window and its right frame column fit the 16 dwords
a row's lanes cover, the bound on what the unclamped loads reach, the workgroup's LDS,
and the multiplier that replaces the division of the workgroup id.  Run with -s to see
the LDS bytes per shape."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "orbslam2commentedbyxcm_amd" / "csrc"

# configs[1], configs[4], KITTI, EuRoC, and the GPU test's small shapes
SHAPES = [(640, 480, 1000, 8), (640, 480, 5000, 12), (1241, 376, 2000, 8), (752, 480, 1200, 8),
          (156, 156, 5000, 4), (91, 91, 5000, 2), (783, 100, 5000, 2), (723, 100, 5000, 2),
          (440, 783, 5000, 2), (440, 723, 5000, 2), (440, 813, 5000, 2), (333, 257, 5000, 3),
          (157, 131, 5000, 3), (1023, 767, 1000, 8)]

FC_STRIDE, FC_SPAN, FC_ROWS = 68, 64, 4


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fcp") / "fast_cells_plan"
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "fast_cells_plan.cpp"), str(CSRC / "orbx_geometry.cpp"),
                    str(CSRC / "orbx_runtime.cpp"), "-o", str(exe)], check=True)
    return exe


def _plan(exe, W, H, nf, L):
    out = subprocess.run([str(exe), str(W), str(H), str(nf), str(L)], capture_output=True, text=True, check=True)
    lines = out.stdout.strip().split("\n")
    assert not lines[0].startswith("FAIL"), lines[0]
    ints = lambda s: [int(v) for v in s.split()]
    L_, ncells, fc_wr, fc_wc, fb = ints(lines[0])
    levels = [ints(lines[1 + l]) for l in range(L_)]
    cells = [ints(lines[1 + L_ + i]) for i in range(ncells)]
    divs = [ints(s) for s in lines[1 + L_ + ncells:]]
    return levels, cells, fc_wr, fc_wc, fb, divs


def _lane_mask(q, first_mask, last_q, last_mask):
    """The kernel's per-lane byte mask of dword q."""
    mk = 0 if q > last_q else 0xffffffff
    if q == 0:
        mk &= first_mask
    if q == last_q:
        mk &= last_mask
    return mk


@pytest.mark.parametrize("W,H,nf,L", SHAPES)
def test_fast_cells_plan(plan_exe, W, H, nf, L):
    levels, cells, fc_wr, fc_wc, fb, divs = _plan(plan_exe, W, H, nf, L)
    assert cells
    windows = 0
    for (lv, x0, y0, cols, rows, src_off, pitch, src_al, first_mask, last_q, last_mask) in cells:
        w, h, lpitch, off = levels[lv]
        assert pitch == lpitch and pitch % 64 == 0 and off % 256 == 0
        assert src_off == off + (y0 + 3) * pitch + x0 + 3
        wc, wr = cols - 6, rows - 6
        assert wc <= fc_wc and wr <= fc_wr
        if wc <= 0 or wr <= 0:
            continue  # no detection window: the kernel loads nothing
        windows += 1
        a = src_off & 3
        assert src_al == src_off - a and src_al % 4 == 0
        # the window and its right frame column inside the 64 bytes a row's 16 lanes cover
        assert a + wc + 1 <= FC_SPAN
        for q in range(16):
            mk = _lane_mask(q, first_mask, last_q, last_mask)
            for b in range(4):
                col = 4 * q + b - a  # what the byte-per-lane kernel tested: col in [0, wc)
                assert bool((mk >> (8 * b)) & 0xff) == (0 <= col < wc), (q, b)
                assert (mk >> (8 * b)) & 0xff in (0, 0xff)
        # the unclamped loads: ceil(wr / 4) loads of 4 rows x 64 bytes from src_al, all
        # inside the level's block of the frame (never before it, never past its last row)
        nl = -(-wr // FC_ROWS)
        assert src_al >= off
        assert src_al + (FC_ROWS * nl - 1) * pitch + FC_SPAN <= off + pitch * h <= fb
        # and no further than the byte-per-lane kernel was allowed: 15 rows, 63 columns
        assert FC_ROWS * nl - wr <= 3
    assert windows
    assert fc_wc + 1 + 3 <= FC_SPAN
    lds = 4 * ((((fc_wr + 2) * FC_STRIDE + 2 * fc_wr * fc_wc) + 15) & ~15)
    print(f"{W}x{H} L={L}: fc_wr {fc_wr} fc_wc {fc_wc}, dynamic LDS per workgroup {lds} B")
    assert lds <= 64 * 1024
    if (W, H, nf, L) == (640, 480, 1000, 8):
        assert lds <= 19904  # what the byte layout held
    # the workgroup id's division by d as (id * mul) >> 31, exact while id * d < 2^31
    for d, mul, exact in divs:
        assert exact == 1 and mul == (1 << 31) // d + 1 and mul < 1 << 32
        top = (1 << 31) // d  # ids below top satisfy id * d < 2^31
        ids = np.unique(np.concatenate([np.arange(0, min(top, 400000)), np.arange(max(top - 400000, 0), top)]))
        ids = ids.astype(np.uint64)
        assert (((ids * np.uint64(mul)) >> np.uint64(31)) == ids // np.uint64(d)).all()
