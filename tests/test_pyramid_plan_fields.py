"""What make_plan precomputes for k_pyramid beyond the tile rectangles (orbx_geometry.h):
the per-(tile, level) constants the kernel's threads used to derive themselves, and the
column-quad tap records of its dword-window form.  Each field is checked against the
formula the kernel evaluated before, and every quad's source window against the staged
rectangle it is read from.  Run with -s to see the LDS bytes per shape."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "orbslam2commentedbyxcm_amd" / "csrc"

SHAPES = [(640, 480, 1000, 8, None), (1241, 376, 2000, 8, None), (752, 480, 1200, 8, None),
          (640, 480, 5000, 12, None), (640, 480, 5000, 12, {"ORBX_PZ_SEG": "0"}),
          (640, 480, 5000, 12, {"ORBX_PZ_SEG": "4"}), (1241, 376, 2000, 10, {"ORBX_PZ_SEG": "3"}),
          (320, 240, 500, 4, None), (1023, 767, 1000, 8, None),
          # the GPU test's small shapes: second tiles 1 to 3 px wide
          (129, 97, 500, 4, None), (131, 99, 500, 4, None), (257, 193, 500, 8, None)]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pzf") / "pyramid_plan_fields"
    subprocess.run(["g++", "-O1", "-std=c++17", "-DORBX_DEBUG=1", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "pyramid_plan_fields.cpp"), str(CSRC / "orbx_geometry.cpp"),
                    str(CSRC / "orbx_runtime.cpp"), "-o", str(exe)], check=True)
    return exe


def _plan(exe, W, H, nf, L, env):
    out = subprocess.run([str(exe), str(W), str(H), str(nf), str(L)], capture_output=True, text=True,
                         check=True, env=dict(os.environ, **(env or {})))
    lines = out.stdout.split("\n")
    ints = lambda s: [int(v) for v in s.split()]
    L_, nseg = ints(lines[0])
    segs = [ints(lines[1 + s]) for s in range(nseg)]
    i, levels = 1 + nseg, []
    for l in range(L_):
        w, h = ints(lines[i])
        i += 1
        xt = yt = None
        if l > 0:
            xt = np.array(ints(lines[i])).reshape(-1, 2)
            yt = np.array(ints(lines[i + 1])).reshape(-1, 2)
            i += 2
        levels.append((w, h, xt, yt))
    rects = []
    for (l0, nl, nx, ny, _a, _b) in segs:
        n = nx * ny * nl
        rects.append(np.array([ints(lines[i + k]) for k in range(n)]).reshape(nx * ny, nl, 8))
        i += n
    pz_win = int(lines[i])
    i += 1
    fields = []
    for (l0, nl, nx, ny, _a, _b) in segs:
        n = nx * ny * nl
        fields.append(np.array([ints(lines[i + k]) for k in range(n)]).reshape(nx * ny, nl, 8 + 17))
        i += n
    quads = [None]
    for l in range(1, L_):
        nqd = int(lines[i])
        quads.append(np.array([ints(lines[i + 1 + k]) for k in range(nqd)]).reshape(nqd, 17))
        i += 1 + nqd
    return levels, segs, rects, pz_win, fields, quads


def _check_quad(rec, cols, xt):
    """A tap record against the resize table: column k of the quad reads source bytes
    c00 + selector (low / high u16 half of the pair)."""
    c00 = rec[16]
    for k, x in enumerate(cols):
        assert rec[2 * k] >> 8 == 0x0c and rec[2 * k + 1] >> 8 == 0x0c  # the u16 halves' zero bytes
        assert c00 + (rec[2 * k] & 0xff) == xt[x, 0] and c00 + (rec[2 * k + 1] & 0xff) == xt[x, 1]
        assert 0 <= (rec[2 * k] & 0xff) <= 7 and 0 <= (rec[2 * k + 1] & 0xff) <= 7


@pytest.mark.parametrize("W,H,nf,L,env", SHAPES)
def test_pyramid_plan_fields(plan_exe, W, H, nf, L, env):
    levels, segs, rects, pz_win, fields, quads = _plan(plan_exe, W, H, nf, L, env)
    assert pz_win == 1  # scale factor 1.2: the dword-window form
    tid = np.arange(256)
    for l in range(1, L):  # the row walk: a row's first source row is at or past the row before's second
        yt = levels[l][3]
        assert (yt[1:, 0] >= yt[:-1, 1]).all()
        # level-wide records: columns past the width borrow the last column's taps
        w, xt = levels[l][0], levels[l][2]
        assert len(quads[l]) == (w + 3) // 4
        for q, rec in enumerate(quads[l]):
            _check_quad(rec, [min(4 * q + k, w - 1) for k in range(4)], xt)
    for (l0, nl, nx, ny, lds_a, lds_b), R, F in zip(segs, rects, fields):
        print(f"{W}x{H} L={L} {env or ''} segment at level {l0}: lds_a + lds_b = {lds_a} + {lds_b} = {lds_a + lds_b}")
        for t in range(R.shape[0]):
            for k in range(nl):
                x0, y0, x1, y1 = R[t, k, :4]
                nq, G, rc, sstride, sxa, sy0, mlo, mhi = F[t, k, :8]
                if x1 <= x0 or y1 <= y0:
                    assert nq == 0 and G == 0 and rc == 0
                    continue
                hn = y1 - y0
                # the formulas k_pyramid evaluated per thread before
                assert nq == (x1 - (x0 & ~3) + 3) >> 2
                nqp = min(nq, 256)
                assert G == 256 // nqp
                assert rc == (hn + G - 1) // G and 1 <= rc <= hn
                assert (((tid * (mlo | (mhi << 16))) >> 16) == tid // nqp).all()
                assert 4 * nq * hn + 16 <= (lds_b if k & 1 else lds_a)
                if k == 0:
                    continue
                px0, py0, px1, py1 = R[t, k - 1, :4]
                assert sxa == px0 & ~3 and sy0 == py0 and sstride == 4 * ((px1 - sxa + 3) >> 2)
                xt = levels[l0 + k][2]
                xa = x0 & ~3
                for q in range(nq):
                    if q == 0:  # the tile's own record: columns clamped into the rectangle
                        rec, cols = F[t, k, 8:], [min(max(xa + c, x0), x1 - 1) for c in range(4)]
                        _check_quad(rec, cols, xt)
                    else:  # the level's record; its columns inside the rectangle are the real ones
                        rec = quads[l0 + k][(xa >> 2) + q]
                        assert xa + 4 * q >= x0
                    # the three-dword window: inside the staged row plus the 8 bytes of slack
                    # behind it (the next row, or the buffer's 16 spare bytes)
                    wb = (rec[16] & ~3) - sxa
                    assert 0 <= wb and wb + 12 <= sstride + 8
                    # and the bytes a needed column reads are staged source columns
                    for c in range(4):
                        x = xa + 4 * q + c
                        if x0 <= x < x1:
                            assert px0 <= xt[x, 0] and xt[x, 1] < px1
