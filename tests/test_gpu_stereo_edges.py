"""GPU parity of ComputeStereoMatches (k_stereo_index, k_stereo, k_stereo_outlier) on the
hand-built pairs of stereo_edge_scenes.py, bit for bit against the CPU oracle in u_right and
depth, in the host form and the batched device form.  test_stereo_edge_scenes.py shows on the
CPU that every scene reaches what its name says.

The images are extracted only to put their pyramids on the device (each level is compared
with the oracle's first, so a failure points at the right stage); the keypoints and
descriptors the matcher sees are the scene's own.  Every scene of one base shares one
extraction.  Frames are packed, or in the pitched layout of extractor.device_frames with
level 0 read in place from the caller's frames (416-byte rows at a 448-byte pitch).

The row index of a pair lives in LDS, (nlevels + 1) * rows + 2 words: 1280 rows at 12 levels
need 66,568 bytes (the hipFuncSetAttribute path), 2953 rows the 153,564 bytes that are the most
it takes, and 2960 rows are refused with ORBX_ERR_UNSUPPORTED before any upload or launch.
Those frames are 832 and 1664 px wide: the extractor, which builds the pyramids, refuses a
256-px-wide frame of that height (its octree would have round(width / height) = 0 roots).
"""
import ctypes as C

import numpy as np
import pytest

import stereo_edge_scenes as E
from orbslam2commentedbyxcm_amd import ORBextractor
from orbslam2commentedbyxcm_amd import _lib as L
from orbslam2commentedbyxcm_amd.extractor import device_frames
from orbslam2commentedbyxcm_amd.matcher import FrameView, ORBmatcher

pytestmark = pytest.mark.gpu

SCENES = dict(E.all_scenes())
PITCHED = ("sad", "sad_max_d7", "band", "outlier_len_1025", "levels_416x240_2")
_staged, _ref, _scene = {}, {}, {}


def scene(name):
    if name not in _scene:
        _scene[name] = SCENES[name]() if name in SCENES else E.outlier_scene(name[len("outlier_"):])
    return _scene[name]


def extract_device(ex, imgs, pitched):
    """Pyramids of imgs (B, H, W) on the device through extract_batch_device; returns what must stay alive."""
    import torch

    dev = torch.device("cuda", 0)
    B, H, W = imgs.shape
    if pitched:
        ex.set_level0_in_place(True)
        frames = device_frames(imgs, dev)
        assert frames.stride(1) % 64 == 0 and frames.stride(1) != W
    else:
        frames = torch.from_numpy(imgs).to(dev)
    cap = ex.max_keypoints(W, H)
    kps = torch.empty((B, cap, 7), dtype=torch.int32, device=dev)
    desc = torch.empty((B, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ex.extract_batch_device(frames, kps, desc, n)
    torch.cuda.synchronize()
    return frames, kps, desc, n


def staged(oracle, base, pitched=False):
    """(extractor holding base.left, base.right as frames 0, 1; the oracle's two pyramids)."""
    key = (base.name, pitched)
    if key not in _staged:
        ex = ORBextractor(*base.params)
        imgs = np.stack([base.left, base.right])
        keep = extract_device(ex, imgs, True) if pitched else ex.extract_batch(imgs)
        p = oracle.params(*base.params)
        pl, pr = oracle.pyramid(base.left, p), oracle.pyramid(base.right, p)
        for f, pyr in ((0, pl), (1, pr)):
            for lv in range(base.nlevels):
                assert np.array_equal(ex.pyramid_level(lv, f), pyr[lv]), ("pyramid", base.name, f, lv)
        assert np.array_equal(ex.GetScaleFactors(), base.sf)
        _staged[key] = (ex, pl, pr, keep)
    return _staged[key][:3]


def view_of(s):
    return FrameView(keys=s.keys_l, desc=s.desc_l, bf=s.bf, scale_factors=s.base.sf)


def reference(oracle, s, pl, pr):
    if s.name not in _ref:
        _ref[s.name] = oracle.compute_stereo_matches(view_of(s), s.keys_r, s.desc_r, pl, pr, s.max_disparity)
    return _ref[s.name]


def check_host(oracle, name, pitched=False):
    s = scene(name)
    ex, pl, pr = staged(oracle, s.base, pitched)
    ur_r, dp_r = reference(oracle, s, pl, pr)
    ur_g, dp_g = ORBmatcher(0.6, True).ComputeStereoMatches(ex, 0, ex, 1, view_of(s), s.keys_r, s.desc_r,
                                                            s.max_disparity)
    assert np.array_equal(ur_g, ur_r), (name, np.nonzero(ur_g != ur_r)[0][:10])
    assert np.array_equal(dp_g, dp_r), (name, np.nonzero(dp_g != dp_r)[0][:10])
    return ur_r


@pytest.mark.parametrize("name", list(SCENES))
def test_host(oracle, orbx_built, name):
    ur = check_host(oracle, name)
    if name in ("sad", "band", "sad_max_d7") or name.startswith("levels"):
        assert (ur >= 0).sum() >= 10 and (ur < 0).sum() >= 4


@pytest.mark.parametrize("name", PITCHED)
def test_host_pitched(oracle, orbx_built, name):
    check_host(oracle, name, pitched=True)


@pytest.mark.parametrize("cap,pitched", [(1500, True), (8192, False)])
def test_batch_device(oracle, orbx_built, cap, pitched):
    """One launch of eight pairs: N = 0, 1, 17, 1025, cap and 700 of the lattice base, one pair
    without right keypoints, and the band scene; outputs prefilled with a sentinel, slots past
    each pair's count exactly -1, and a second call writes the same bytes."""
    import torch

    names = ["n_left_0", "outlier_len_1", "outlier_len_17", "outlier_len_1025", "outlier_len_%d" % cap,
             "outlier_len_700", "n_right_0", "band"]
    S = [scene(n) for n in names]
    B = len(S)
    refs = []
    for s in S:
        p = oracle.params(*s.base.params)
        refs.append(reference(oracle, s, oracle.pyramid(s.left, p), oracle.pyramid(s.right, p)))
    ex = ORBextractor(*S[0].params)
    imgs = np.stack([s.left for s in S] + [s.right for s in S])
    keep = extract_device(ex, imgs, pitched)
    hk = np.zeros((2 * B, cap), L.KEYPOINT_DTYPE)
    hd = np.full((2 * B, cap, 32), 0xA5, np.uint8)
    hn = np.zeros(2 * B, np.int32)
    for b, s in enumerate(S):
        for row, k, d in ((b, s.keys_l, s.desc_l), (B + b, s.keys_r, s.desc_r)):
            hk[row, :len(k)], hd[row, :len(k)], hn[row] = k, d, len(k)
    assert sorted(hn[:B])[:4] == [0, 1, 17, 30] and hn[:B].max() == cap and hn[B + names.index("n_right_0")] == 0
    dev = torch.device("cuda", 0)
    kps = torch.from_numpy(hk.view(np.int32).reshape(2 * B, cap, 7)).to(dev)
    desc = torch.from_numpy(hd).to(dev)
    n = torch.from_numpy(hn).to(dev)
    m = ORBmatcher(0.6, True)
    outs = []
    for _ in range(2):
        ur = torch.full((B, cap), 7.0, dtype=torch.float32, device=dev)
        dp = torch.full((B, cap), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        m.ComputeStereoMatchesBatchDevice(ex, ex, kps[:B], desc[:B], n[:B], kps[B:], desc[B:], n[B:], E.BF, E.MAX_D,
                                          ur, dp, left_frame0=0, right_frame0=B)
        torch.cuda.synchronize()
        outs.append((ur.cpu().numpy(), dp.cpu().numpy()))
    (hur, hdp), (hur2, hdp2) = outs
    assert hur.tobytes() == hur2.tobytes() and hdp.tobytes() == hdp2.tobytes()
    for b, (s, (ur_r, dp_r)) in enumerate(zip(S, refs)):
        nl = len(s.keys_l)
        assert s.max_disparity == E.MAX_D
        assert np.array_equal(hur[b, :nl], ur_r), (names[b], np.nonzero(hur[b, :nl] != ur_r)[0][:10])
        assert np.array_equal(hdp[b, :nl], dp_r), names[b]
        assert (hur[b, nl:] == -1).all() and (hdp[b, nl:] == -1).all(), names[b]
    del keep


# ---- refusals of the host form: the outputs are all -1

def host_rc(m, ex, s, kl=None, kr=None, n_out=None):
    """orbx_compute_stereo_matches on scene s with its left / right keypoints replaced;
    returns (rc, u_right, depth) with the outputs prefilled with 7."""
    kl = s.keys_l if kl is None else kl
    kr = np.ascontiguousarray(s.keys_r if kr is None else kr)
    dl = np.zeros((len(kl), 32), np.uint8)
    dl[:min(len(kl), len(s.desc_l))] = s.desc_l[:len(kl)]
    lv = FrameView(keys=kl, desc=dl, bf=s.bf, scale_factors=s.base.sf)
    c = lv.c()
    dr = np.ascontiguousarray(s.desc_r)
    ur = np.full(max(len(kl), 1), 7.0, np.float32)
    dp = np.full(max(len(kl), 1), 7.0, np.float32)
    F32P = C.POINTER(C.c_float)
    rc = L.lib().orbx_compute_stereo_matches(m._h, ex._h, 0, ex._h, 1, C.addressof(c), kr.ctypes.data, L.u8ptr(dr),
                                             len(kr), C.c_float(s.max_disparity), ur.ctypes.data_as(F32P),
                                             dp.ctypes.data_as(F32P))
    return rc, ur, dp


@pytest.mark.parametrize("field,value,side", [("y", -0.5, "l"), ("y", 240.0, "l"), ("octave", 8, "l"),
                                              ("octave", -1, "l"), ("octave", 8, "r"), ("octave", -1, "r")])
def test_host_refuses_keypoints_outside_the_pyramid(oracle, orbx_built, field, value, side):
    s = scene("sad")
    ex, _, _ = staged(oracle, s.base)
    k = (s.keys_l if side == "l" else s.keys_r).copy()
    k[field][len(k) // 2] = value
    rc, ur, dp = host_rc(ORBmatcher(0.6, True), ex, s, **{"kl" if side == "l" else "kr": k})
    assert rc == L.ORBX_ERR_ARG
    assert (ur == -1).all() and (dp == -1).all()


def test_host_refuses_more_than_8192_keypoints(oracle, orbx_built):
    s = scene("sad")
    ex, _, _ = staged(oracle, s.base)
    kl = np.resize(s.keys_l, 8193)
    rc, ur, dp = host_rc(ORBmatcher(0.6, True), ex, s, kl=kl)
    assert rc == L.ORBX_ERR_UNSUPPORTED and len(ur) == 8193
    assert (ur == -1).all() and (dp == -1).all()


def test_row_index_over_150_kb_is_refused(oracle, orbx_built):
    """12 levels x 2960 rows: 153,928 bytes of row index.  Both forms refuse before any upload or
    launch; the host form's outputs are all -1, the device form's are untouched."""
    import torch

    W, H = 1664, 2960
    assert (13 * H + 2) * 4 > 150 * 1024 >= (13 * 2953 + 2) * 4
    ex = ORBextractor(1000, 1.2, 12, 20, 7)
    ex.extract_batch(np.full((2, H, W), 100, np.uint8))
    s = scene("levels_832x1280_12")
    m = ORBmatcher(0.6, True)
    rc, ur, dp = host_rc(m, ex, s)
    assert rc == L.ORBX_ERR_UNSUPPORTED and "150 KB" in L.lib().orbx_last_error().decode()
    assert (ur == -1).all() and (dp == -1).all()
    dev = torch.device("cuda", 0)
    cap = 64
    kps = torch.zeros((2, cap, 7), dtype=torch.int32, device=dev)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros((2,), dtype=torch.int32, device=dev)
    out = torch.full((2, cap), 7.0, dtype=torch.float32, device=dev)
    with pytest.raises(L.OrbxError) as e:
        m.ComputeStereoMatchesBatchDevice(ex, ex, kps[:1], desc[:1], n[:1], kps[1:], desc[1:], n[1:], E.BF, E.MAX_D,
                                          out[:1], out[1:], left_frame0=0, right_frame0=1)
    assert e.value.code == L.ORBX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
