"""GPU parity of k_level_tiles (blur + FAST strength map, 64 x 48 level tiles) on the
smallest inputs where its dense passes can go wrong: single frames, 500 features, scale
1.2, 4 levels, every keypoint field, the keypoint order, all descriptor bits (which read
the blurred image) and the pyramid compared bit for bit with the oracle.

* 333 x 251: the width is no multiple of 4 and the last tile column is 13 px wide; the
  last tile row holds 11 rows, so two of its three compass row groups lie wholly outside
  the image and are masked, not skipped; the detection border x = 19 / w - 19 falls
  inside a column quad.
* uniform random bytes at that size: nearly every pixel passes the compass test, so the
  tiles' survivor lists run at their capacity.
* a constant image (no survivors, no keypoints), and one with an 8 x 8 bright square
  centred at (19, 19), whose corners lie on the detection border.
* one 640 x 480 synthetic frame through the device call with level 0 read in place and
  copied: the level-0 source pointer and pitch differ between the two.
"""
import numpy as np
import pytest

from orbslam2commentedbyxcm_amd import ORBextractor, synth
from orbslam2commentedbyxcm_amd import _lib as L

pytestmark = pytest.mark.gpu

PRM = (500, 1.2, 4, 20, 7)
W, H = 333, 251


def _square():
    img = np.full((H, W), 60, np.uint8)
    img[15:23, 15:23] = 220  # 8 x 8, centred at (19, 19)
    return img


IMAGES = {
    "synth": lambda: synth.frame(5, W, H),
    "noise": lambda: np.random.default_rng(3).integers(0, 256, (H, W), dtype=np.uint8),
    "flat": lambda: np.full((H, W), 128, np.uint8),
    "square": _square,
}


def _cmp(kp_gpu, desc_gpu, kp_ref, desc_ref):
    assert len(kp_gpu) == len(kp_ref), (len(kp_gpu), len(kp_ref))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        a, b = kp_gpu[f], kp_ref[f]
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"field {f}: {bad.size} mismatches, first {bad[:5]} gpu={a[bad[:5]]} ref={b[bad[:5]]}"
    bad = np.nonzero((desc_gpu != desc_ref).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} descriptor mismatches, first {bad[:5]}"


@pytest.mark.parametrize("name", list(IMAGES))
def test_333x251_matches_oracle(oracle, orbx_built, name):
    img = IMAGES[name]()
    p = oracle.params(*PRM)
    ex = ORBextractor(*PRM)
    kps, desc = ex(img)
    kr, dr, _ = oracle.extract(img, p)
    if kps is None:
        kps, desc = np.zeros(0, dtype=L.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
    _cmp(kps, desc, kr, dr)
    if name == "flat":
        assert len(kr) == 0
    if name in ("synth", "noise"):
        assert len(kr) > 300, len(kr)
    for lv, (a, b) in enumerate(zip(ex.mvImagePyramid, oracle.pyramid(img, p))):
        assert a.shape == b.shape
        assert np.array_equal(a, b), f"level {lv}: {(a != b).sum()} pixels differ"


@pytest.fixture(scope="module")
def vga_reference(oracle):
    img = synth.frame(5)
    p = oracle.params(*PRM)
    kr, dr, _ = oracle.extract(img, p)
    return img, kr, dr, oracle.pyramid(img, p)


@pytest.mark.parametrize("in_place", [True, False])
def test_640x480_level0_in_place_and_copied(orbx_built, vga_reference, in_place):
    import torch

    img, kr, dr, pyr = vga_reference
    ex = ORBextractor(*PRM)
    ex.set_level0_in_place(in_place)
    cap = ex.max_keypoints(640, 480)
    dev = torch.device("cuda", 0)
    d_frames = torch.from_numpy(img[None]).to(dev)
    kps = torch.empty((1, cap, 7), dtype=torch.int32, device=dev)
    desc = torch.empty((1, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.empty((1,), dtype=torch.int32, device=dev)
    ex.extract_batch_device(d_frames, kps, desc, n)
    torch.cuda.synchronize()
    assert not ex.status().any()
    m = int(n.cpu()[0])
    k = kps.cpu().numpy().view(np.uint8).reshape(cap, 28).view(L.KEYPOINT_DTYPE).reshape(cap)
    _cmp(k[:m], desc.cpu().numpy()[0, :m], kr, dr)
    assert len(kr) > 300
    for lv in range(PRM[2]):
        a = ex.pyramid_level(lv, frame=0)
        assert a.shape == pyr[lv].shape and np.array_equal(a, pyr[lv]), lv
