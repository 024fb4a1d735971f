"""k_pyramid against the oracle's pyramid, byte for byte, at the smallest shapes where its
tiling, ownership or tap records can go wrong: 2 x 2 tiles whose second tile is 1 to 3 px
wide (widths of every residue mod 4), more tiles than levels, both workgroup placements
(a batch of 8 takes the XCD-aware one), two segments, unaligned rows, the byte-read form,
and level 0 read in place or copied.  The frames are noise, so a wrong tap, or a pixel two
tiles write differently, shows."""
import numpy as np
import pytest

from orbslam2commentedbyxcm_amd import ORBextractor

pytestmark = pytest.mark.gpu


@pytest.fixture
def switch():
    """orbx_debug_set for one test: every switch back to its default afterwards."""
    from orbslam2commentedbyxcm_amd import _lib as L
    yield L.debug_set
    L.debug_set(None)


def _noise(B, W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W), dtype=np.uint8)


def _check(oracle, frames, prm, in_place=False):
    import torch

    B, H, W = frames.shape
    ex = ORBextractor(*prm)
    if in_place:
        ex.set_level0_in_place(True)
    dev = torch.device("cuda", 0)
    d_frames = torch.from_numpy(frames).to(dev)  # rows W bytes apart
    cap = ex.max_keypoints(W, H)
    kps = torch.empty((B, cap, 7), dtype=torch.int32, device=dev)
    desc = torch.empty((B, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    ex.extract_batch_device(d_frames, kps, desc, n)
    torch.cuda.synchronize()
    p = oracle.params(*prm)
    for b in range(B):
        ref = oracle.pyramid(frames[b], p)
        assert len(ref) == prm[2]
        for lv, want in enumerate(ref):
            got = ex.pyramid_level(lv, b)
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"frame {b} level {lv}: {len(bad)} pixels differ, first (y, x) {bad[:4].tolist()}"
    del d_frames


@pytest.mark.parametrize("W,H,nl,B", [(129, 97, 4, 2), (131, 99, 4, 2), (130, 98, 4, 1), (132, 100, 4, 1),
                                      (257, 193, 8, 2), (640, 480, 8, 3), (640, 480, 8, 8), (640, 480, 12, 2),
                                      (1241, 376, 8, 2)])
def test_pyramid_tiles_match_oracle(oracle, orbx_built, W, H, nl, B):
    """1241-byte rows are the unaligned-row path of the level-0 staging; 12 levels are two
    segments (the second reads its input level back from the pyramid)."""
    _check(oracle, _noise(B, W, H, 1000 + W + nl + B), (1000, 1.2, nl, 20, 7))


@pytest.mark.parametrize("W,H,sf,nl", [(640, 480, 1.2, 8), (131, 99, 1.2, 4), (640, 480, 2.5, 3)])
def test_pyramid_tiles_byte_form(oracle, orbx_built, switch, W, H, sf, nl):
    """The byte-read form: forced by the switch pz_byte at scale factor 1.2, chosen by the
    plan at 2.5 (four columns' taps span more than 8 source bytes)."""
    if sf < 2.0:
        switch("pz_byte", 1)
    _check(oracle, _noise(2, W, H, 7 + W), (1000, sf, nl, 20, 7))


@pytest.mark.parametrize("sf,nl", [(1.5, 6), (2.0, 3), (1.05, 4)])
def test_pyramid_tiles_other_scales(oracle, orbx_built, sf, nl):
    """Other scale factors in the dword-window form: wider source spans per quad, and a
    factor near 1 where most output rows reuse the row before's second source row."""
    _check(oracle, _noise(2, 333, 251, 31), (1000, sf, nl, 20, 7))


@pytest.mark.parametrize("in_place", [True, False])
def test_pyramid_tiles_level0(oracle, orbx_built, in_place):
    """Level 0 read in place from the caller's frames (not stored by k_pyramid) or copied."""
    _check(oracle, _noise(3, 640, 480, 5), (1000, 1.2, 8, 20, 7), in_place=in_place)
