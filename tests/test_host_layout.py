"""orbx_layout.h against the offset chains it replaced (CPU only).

tests/cpp/host_layout.cpp includes nothing but csrc/orbx_layout.h and prints the offsets
and the total of a list of regions.  Each case below gives it the regions one converted
site declares, in the order it declares them, and compares with that site's earlier chain
`o_a = 0, o_b = o_a + pad(...), ...` written out here with

    up256(b) = (b + 255) & ~255         orbx_sim3 / orbx_initializer / orbx_kfdb / orbx_vocab
    pad(b)   = up256(b) + 256           orbx_matcher

so a moved offset or a changed allocation size fails here, without a GPU.
"""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "orbslam2commentedbyxcm_amd" / "csrc"
KP = 28            # sizeof(orbx_keypoint)
GEOM_KF = 112      # sizeof(TriGeomKF): five pointers, Tcw [12] float, Ow [3] double
NS = (0, 1, 63, 64, 65, 257)
NMP = (0, 1)
ITS = (1, 300)


def up256(b):
    return (b + 255) & ~255


def pad(b):
    return up256(b) + 256


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("layout") / "host_layout"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", f"-I{CSRC}",
                    str(ROOT / "tests" / "cpp" / "host_layout.cpp"), "-o", str(out)], check=True)
    return out


def layout(exe, rounding, regions):
    """Offsets of `regions` (ints; "@" aligns the cursor to 256 and has no offset) and the total."""
    r = subprocess.run([str(exe), rounding, *map(str, regions)], capture_output=True, text=True, check=True)
    v = [int(x) for x in r.stdout.split()]
    return v[:-1], v[-1]


def test_a_zero_byte_region(exe):
    # the chains give it zero bytes plus the rounding: pad(0) = 256, up256(0) = 0
    assert layout(exe, "pad", [0, 0, 5]) == ([0, 256, 512], 1024)
    assert layout(exe, "up256", [0, 0, 5]) == ([0, 0, 0], 256)
    assert layout(exe, "packed", [0, 0, 5]) == ([0, 0, 0], 5)
    assert layout(exe, "packed", [5, "@", 0, 1, "@"]) == ([0, 256, 256], 512)


@pytest.mark.parametrize("n_mp", NMP)
@pytest.mark.parametrize("n", NS)
def test_pose_optimization_host_form(exe, n, n_mp):
    cap, nt = max(n, 1), max(n_mp, 1)
    o_keys = 0
    o_ur = o_keys + pad(KP * cap)
    o_mp = o_ur + pad(4 * cap)
    o_pos = o_mp + pad(4 * cap)
    o_in = o_pos + pad(12 * nt)
    o_out = o_in + pad(64)
    out_bytes = 12 * 4 + 2 * 4 + 8 * 4 + cap
    total = o_out + pad(out_bytes)
    # Tcw_opt, ninliers, ninit, trace, outlier
    res = layout(exe, "packed", [48, 4, 4, 32, cap])
    assert res == ([0, 48, 52, 56, 88], out_bytes)
    assert layout(exe, "pad", [KP * cap, 4 * cap, 4 * cap, 12 * nt, 64, res[1]]) == (
        [o_keys, o_ur, o_mp, o_pos, o_in, o_out], total)


@pytest.mark.parametrize("n_mp", NMP)
@pytest.mark.parametrize("n2", (0, 65))
@pytest.mark.parametrize("n1", NS)
def test_optimize_sim3_host_form(exe, n1, n2, n_mp):
    c1, c2, nt = max(n1, 1), max(n2, 1), max(n_mp, 1)
    o_k1 = 0
    o_mp1 = o_k1 + pad(KP * c1)
    o_i2 = o_mp1 + pad(4 * c1)
    o_k2 = o_i2 + pad(4 * c1)
    o_pos = o_k2 + pad(KP * c2)
    o_in = o_pos + pad(12 * nt)
    o_out = o_in + pad(40 * 4)
    out_bytes = 20 * 4 + 4 * c1
    total = o_out + pad(out_bytes)
    # R12_opt, t12_opt, s12_opt, ninliers, ncorr, nbad, trace, matches12
    res = layout(exe, "packed", [36, 12, 4, 4, 4, 4, 16, 4 * c1])
    assert res == ([0, 36, 48, 52, 56, 60, 64, 80], out_bytes)
    assert layout(exe, "pad", [KP * c1, 4 * c1, 4 * c1, KP * c2, 12 * nt, 160, res[1]]) == (
        [o_k1, o_mp1, o_i2, o_k2, o_pos, o_in, o_out], total)


@pytest.mark.parametrize("nmatched", NS)
@pytest.mark.parametrize("nk", NS)
def test_triangulate_pairs_host_form(exe, nk, nmatched):
    kcap, C = max(1, nk), max(nmatched, 1)
    kb, fb = pad(KP * kcap), pad(4 * kcap)
    per_kf = 2 * kb + 2 * fb
    o_pairs = 2 * per_kf
    o_cnt = o_pairs + pad(8 * C)
    o_out = o_cnt + pad(16)
    q_new, q_idx = 0, 16
    q_max = q_idx + 4 * C
    q_min = q_max + 4 * C
    q_pos = q_min + 4 * C
    q_nrm = q_pos + 12 * C
    q_rsn = q_nrm + 12 * C
    q_mth = q_rsn + C
    out_bytes = q_mth + C
    total = o_out + pad(out_bytes)
    res = layout(exe, "packed", [16, 4 * C, 4 * C, 4 * C, 12 * C, 12 * C, C, C])
    assert res == ([q_new, q_idx, q_max, q_min, q_pos, q_nrm, q_rsn, q_mth], out_bytes)
    kf = [KP * kcap, KP * kcap, 4 * kcap, 4 * kcap]
    want = [b + o for b in (0, per_kf) for o in (0, kb, 2 * kb, 2 * kb + fb)] + [o_pairs, o_cnt, o_out]
    assert layout(exe, "pad", kf + kf + [8 * C, 16, res[1]]) == (want, total)


@pytest.mark.parametrize("npairs", (1, 65))
@pytest.mark.parametrize("nkf", (0, 2, 257))
def test_triangulate_tables(exe, nkf, npairs):
    # nkf = 0 is a zero-byte region: pad(0) = 256 bytes
    o_kf = 0
    o_pk = o_kf + pad(GEOM_KF * nkf)
    o_sc = o_pk + pad(8 * npairs)
    o_sg = o_sc + pad(4 * 32)
    tab = pad(GEOM_KF * nkf) + pad(8 * npairs) + 2 * pad(4 * 32)
    assert layout(exe, "pad", [GEOM_KF * nkf, 8 * npairs, 128, 128]) == ([o_kf, o_pk, o_sc, o_sg], tab)


@pytest.mark.parametrize("its", ITS)
@pytest.mark.parametrize("n_mp", NMP)
@pytest.mark.parametrize("cap", (1, 63, 64, 65, 257))
def test_sim3_host_form(exe, cap, n_mp, its):
    c4, npos, ndraw = up256(cap * 4), up256(max(n_mp, 1) * 12), up256(its * 12)
    o_n1, o_mp1 = 0, 256
    o_mp2 = o_mp1 + c4
    o_oct1 = o_mp2 + c4
    o_oct2 = o_oct1 + c4
    o_T = o_oct2 + c4
    o_pos = o_T + 256
    o_draws = o_pos + npos
    o_out = o_draws + ndraw
    ints, floats = 8, 16 + 9 + 3 + 1
    total = o_out + up256(ints * 4 + floats * 4 + cap)
    # eight ints; T12, best_R, best_t, best_s; inliers
    res = layout(exe, "packed", [4] * 8 + [64, 36, 12, 4, cap])
    assert res == ([4 * i for i in range(8)] + [32, 32 + 64, 32 + 100, 32 + 112, 32 + 116], 32 + 116 + cap)
    assert layout(exe, "up256", [4, 4 * cap, 4 * cap, 4 * cap, 4 * cap, 96, max(n_mp, 1) * 12, its * 12, res[1]]) == (
        [o_n1, o_mp1, o_mp2, o_oct1, o_oct2, o_T, o_pos, o_draws, o_out], total)


@pytest.mark.parametrize("its", ITS)
@pytest.mark.parametrize("kcap", (1, 63, 64, 65, 257))
def test_initializer_host_form(exe, kcap, its):
    nkeys, c1, c4 = up256(kcap * KP), up256(kcap), up256(kcap * 4)
    o_n, o_k1 = 0, 256
    o_k2 = o_k1 + nkeys
    o_m = o_k2 + nkeys
    o_sets = o_m + c4
    o_out = o_sets + up256(its * 32)
    ints, floats = 12, 36
    r_fl = ints * 4
    r_ih = up256(r_fl + floats * 4)
    r_if = r_ih + c1
    r_tr = r_if + c1
    r_p3d = r_tr + c1
    r_total = r_p3d + up256(kcap * 12)
    total = o_out + r_total
    # eleven ints, status with the spare; SH SF RH parallax H21 F21 R21 t21; align; the arrays
    res = layout(exe, "packed", [4] * 10 + [8] + [4] * 4 + [36, 36, 36, 12, "@", c1, c1, c1, up256(kcap * 12)])
    fl = [r_fl + 4 * k for k in (0, 1, 2, 3, 4, 13, 22, 31)]
    assert res == ([4 * i for i in range(11)] + fl + [r_ih, r_if, r_tr, r_p3d], r_total)
    assert layout(exe, "up256", [8, kcap * KP, kcap * KP, kcap * 4, its * 32, res[1]]) == (
        [o_n, o_k1, o_k2, o_m, o_sets, o_out], total)


@pytest.mark.parametrize("its", ITS)
@pytest.mark.parametrize("cap", (1, 65, 257))
@pytest.mark.parametrize("B", (1, 3))
def test_sim3_work(exe, B, cap, its):
    slots, planes, state = B * cap, 10, 8
    o_pts = 0
    o_thr = o_pts + up256(slots * planes * 8)
    o_idx = o_thr + up256(slots * 2 * 4)
    o_state = o_idx + up256(slots * 4)
    o_counts = o_state + up256(B * state * 4)
    total = o_counts + up256(B * its * 4)
    assert layout(exe, "up256", [slots * planes * 8, slots * 8, slots * 4, B * state * 4, B * its * 4]) == (
        [o_pts, o_thr, o_idx, o_state, o_counts], total)


@pytest.mark.parametrize("its", ITS)
@pytest.mark.parametrize("kcap", (1, 65, 257))
@pytest.mark.parametrize("B", (1, 3))
def test_initializer_work(exe, B, kcap, its):
    slots, n, state, mats, hyps = B * kcap, B * its, 8, 27, 8
    o_pts = 0
    o_idx1 = o_pts + up256(slots * 4 * 8)
    o_norm = o_idx1 + up256(slots * 4)
    o_state = o_norm + up256(B * 8 * 8)
    o_mats = o_state + up256(B * state * 4)
    o_bad = o_mats + up256(n * mats * 8)
    o_scores = o_bad + up256(n * 4)
    o_inl = o_scores + up256(n * 2 * 8)
    o_hyp = o_inl + up256(slots)
    o_cosw = o_hyp + up256(B * hyps * 12 * 8)
    o_good = o_cosw + up256(slots * hyps * 8)
    o_par = o_good + up256(B * hyps * 4)
    total = o_par + up256(B * hyps * 8)
    regions = [slots * 32, slots * 4, B * 64, B * state * 4, n * mats * 8, n * 4, n * 16, slots, B * hyps * 96,
               slots * hyps * 8, B * hyps * 4, B * hyps * 8]
    assert layout(exe, "up256", regions) == (
        [o_pts, o_idx1, o_norm, o_state, o_mats, o_bad, o_scores, o_inl, o_hyp, o_cosw, o_good, o_par], total)
