"""The hand-built matcher scenes (match_edge_scenes.py) are what their names say -- checked
with the CPU oracle alone, no GPU.  The thresholds are conditions on the reference: a scene
that stops reaching its mechanism (one_cell with 10 keypoints per group, missing_top with a
keypoint in octave 5) fails here, before the GPU parity tests can pass vacuously.
"""
import numpy as np
import pytest

import match_edge_scenes as E


def local(oracle, S, th=1.0, nnratio=0.8):
    fmp = S.frame_mp0.copy()
    n = oracle.sbp_local(S.F, fmp, S.queries, S.mps, S.trk, th, nnratio)
    return n, fmp


def matched_ids(fmp, fmp0):
    """MapPoint ids the search assigned (entries that changed)."""
    return set(int(x) for x in fmp[fmp != fmp0])


def test_bounds(oracle):
    S = E.bounds()
    px, py, fx, _ = E.grid_cells(S.F)
    assert (px < 0).sum() >= 10 and (px >= E.COLS).sum() >= 10
    assert (py < 0).sum() >= 10 and (py >= E.ROWS).sum() >= 10
    knife = fx - np.floor(fx) == 0.5
    assert knife.sum() == 64 and np.array_equal(np.nonzero(knife)[0], S.knife)
    assert np.array_equal(px[S.knife], np.arange(1, 65))   # half away from zero; the last one off-grid
    n, fmp = local(oracle, S)
    assert n >= 500
    assert not (matched_ids(fmp, S.frame_mp0) & set(S.outside.tolist()))
    # the outside queries really are in the list, in view, and miss the grid on all four sides
    assert set(S.outside.tolist()) <= set(S.queries.tolist())
    assert (S.u[S.outside] < E.BOUNDS[0] - 15).sum() == 30 and (S.u[S.outside] > E.BOUNDS[1] + 15).sum() == 30
    assert (S.v[S.outside] < E.BOUNDS[2] - 15).sum() == 30 and (S.v[S.outside] > E.BOUNDS[3] + 15).sum() == 30
    nw, _ = local(oracle, S.wide, th=E.WIDE_TH)
    assert nw >= 3


@pytest.mark.parametrize("shuffled", [False, True])
def test_one_cell(oracle, shuffled):
    S = E.one_cell(shuffled=shuffled)
    px, py, _, _ = E.grid_cells(S.F)
    assert len(S.F.keys) == 600 and (px == 32).all() and (py == 24).all()
    n, fmp = local(oracle, S)
    assert n == 600 and (fmp >= 0).all()
    # keypoint i was taken by MapPoint fmp[i] of its own group; its rank in the group is the
    # place it has in that query's distance-ordered candidates
    assert np.array_equal(S.qgroup[fmp], S.group)
    assert (S.rank >= 12).sum() >= 200
    Sh = E.one_cell(shuffled=shuffled, half_zero=True)
    nh, fh = local(oracle, Sh)
    assert nh == 600 and not np.array_equal(fh, fmp)


def test_one_cell_ten_per_group_misses_the_mechanism(oracle):
    """The condition above is a real one: with 10 keypoints per group no query looks past
    its own 12-entry list."""
    S = E.one_cell(per_group=10)
    n, _ = local(oracle, S)
    assert n == 300 and (S.rank >= 12).sum() == 0


def test_one_cell_off_grid(oracle):
    S = E.one_cell(off_grid=True)
    assert not E.on_grid(S.F).any()
    r = 2.5 * E.OFF_GRID_TH * 1.2
    assert (np.abs(S.F.keys["x"] - 639.5) < r).all() and (np.abs(S.F.keys["y"] - E.CELL_V) < r).all()
    n, fmp = local(oracle, S, th=E.OFF_GRID_TH)
    assert n == 0 and np.array_equal(fmp, S.frame_mp0)


@pytest.mark.parametrize("kind", E.LINES)
def test_lines(oracle, kind):
    S = E.lines(kind)
    px, py, _, _ = E.grid_cells(S.F)
    if kind == "col0":
        assert (px == 0).all()
    if kind == "col63":
        assert (px == 63).all()
    if kind == "row47":
        assert (py == 47).all()
    n, _ = local(oracle, S)
    assert n >= (1 if kind in ("n1", "nq1") else 100)


@pytest.mark.parametrize("nlevels", E.LEVELS)
def test_levels(oracle, nlevels):
    S = E.levels(nlevels)
    assert 700 <= len(S.F.keys) <= 1200 and len(S.F.scale_factors) == nlevels
    assert np.array_equal(np.unique(S.F.keys["octave"]), np.arange(nlevels))
    n, _ = local(oracle, S)
    assert 2 * n >= len(S.queries)


def test_missing_top(oracle):
    S = E.missing_top()
    assert len(S.F.scale_factors) == 8 and S.F.keys["octave"].max() == 4
    assert len(S.high) >= 200 and (S.level[S.high] >= 6).all()
    assert np.array_equal(np.unique(S.level), np.arange(8))       # queries at every predicted level
    # each high query sits exactly on an octave-4 keypoint with an identical descriptor
    t = S.high_target
    assert (S.F.keys["octave"][t] == 4).all() and np.array_equal(S.mps.desc[S.high], S.F.desc[t])
    assert np.array_equal(S.u[S.high], S.F.keys["x"][t]) and np.array_equal(S.v[S.high], S.F.keys["y"][t])
    n, fmp = local(oracle, S)
    got = matched_ids(fmp, S.frame_mp0)
    assert not (got & set(S.high.tolist()))
    assert len(got) >= 200
    # level 5 straddles the highest populated octave: range [4, 5], bucket 5 empty beside
    # bucket 4.  Those queries still take the octave-4 keypoint under them.
    l5 = np.nonzero(S.level[:len(S.target)] == 5)[0]
    assert len(l5) >= 40 and (S.F.keys["octave"][S.target[l5]] == 4).all()
    took = [q for q in l5 if fmp[S.target[q]] == q]
    assert len(took) >= 20, len(took)
    # the frame overload moving forward (octaves [nLastOctave, inf)): the same queries find
    # nothing; moving backward (octaves [0, nLastOctave]) they do -- the 240 sit on 120 distinct
    # keypoints, two each, and a keypoint goes to one of them
    St = E.missing_top(stereo=True)
    for tz, want_high in ((1.0, 0), (-1.0, 100)):
        last = E.last_frame(St, tz)
        cur = St.frame_mp0.copy()
        assert np.array_equal(np.unique(last.keys["octave"]), np.arange(8))   # octaves 5-7 included
        oracle.sbp_frame(St.F, cur, last, np.arange(len(St.u), dtype=np.int32), St.mps, 15.0, False, False)
        nhigh = len(matched_ids(cur, St.frame_mp0) & set(St.high.tolist()))
        assert nhigh == 0 if want_high == 0 else nhigh >= want_high, (tz, nhigh)


def test_capacity(oracle):
    for n, nq in E.CAPACITY:
        assert n < 8192
    S = E.capacity(8191, 8191)
    assert len(S.F.keys) == 8191
    n, _ = local(oracle, S)
    assert n >= 5000
