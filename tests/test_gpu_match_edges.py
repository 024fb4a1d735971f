"""GPU parity of the projection matcher on hand-built frames (match_edge_scenes.py), bit for
bit against the CPU oracle: undistortion bounds with off-grid and half-cell keypoints, 600
keypoints in one grid cell (candidate lists truncated at 12 entries and re-scored), grid
columns 0 / 63 and row 47, 2 to 32 pyramid levels, frames whose top octaves are empty, and
sizes at the 13-bit position limit.  test_match_edge_scenes.py shows with the oracle alone
that each scene reaches its mechanism.

Oracle counts (CPU, SearchByProjection(F, vpMapPoints, th = 1, nnratio 0.8)):
  bounds 1045 of 1500 queries on 1564 keypoints (the frame overload 1025, 899 after the
  rotation check); one_cell 600 of 600, 240 of them past their own 12-entry list, in group
  order or shuffled, blocking or half non-blocking; lines 389 / 389 / 387 of 400;
  levels(2, 5, 6, 17, 27, 32) 693 / 738 / 748 / 920 / 1066 / 1136 of 731 / 778 / 793 / 965 /
  1121 / 1200; missing_top (queries at every level 0-7: 64 / 99 / 115 / 115 / 131 / 76 / 120 /
  120) 576 of 840, none of the 240 queries at levels 6 and 7 (frame overload forward 284,
  backward 694); capacity (n, nq) (8191, 8191) 7845, (8191, 16382)
  8079, (1000, 9000) 989, (7000, 8192) 6737.

missing_top is the scene a single call got wrong before its bucket tables were sized by the
frame's nlevels: sized by the highest octave present, the scoring clamped the range [5, 6]
onto bucket 4 and matched the octave-4 keypoints under the queries.  The batched device
forms always sized them by nlevels and are the control.

The single host calls take any nq for n < 8192 (the grid holds n keypoints, the scoring
launch is sized by nq); n >= 8192 is ORBX_ERR_UNSUPPORTED before any device work.

k_proj_search forms at footprint 0 (1024 threads), 8 levels, as the launcher reports them
on the MI355X (<QLDS, DLDS>; FORMS below): nq = n -- <1,1> to n = 1213, <0,1> to 2741,
<0,0> from 2742; max_nq = 500 -- <0,1> at cap 2741, <1,0> 2742 to 4464, <0,0> from 4465.
Refused (ORBX_ERR_UNSUPPORTED, nothing launched): 32 levels at cap >= 2661 in every
footprint but 2 (the split launches keep the bucket tables in global memory); cap 2660 runs
in all six.
"""
import re

import numpy as np
import pytest

import match_edge_scenes as E
from orbslam2commentedbyxcm_amd import _lib as L
from orbslam2commentedbyxcm_amd.matcher import MapPoints, ORBmatcher

pytestmark = pytest.mark.gpu


@pytest.fixture
def switch():
    """orbx_debug_set for one test: every switch back to its default afterwards."""
    yield L.debug_set
    L.debug_set(None)


def _diff(a, b):
    return np.nonzero(a != b)[0][:10]


# ---- the single host calls

def check_local(oracle, S, th=1.0, nnratio=0.8, m=None):
    m = m or ORBmatcher(nnratio, False)
    fg, fr = S.frame_mp0.copy(), S.frame_mp0.copy()
    ng = m.SearchByProjectionLocal(S.F, fg, S.queries, S.mps, S.trk, th)
    nr = oracle.sbp_local(S.F, fr, S.queries, S.mps, S.trk, th, nnratio)
    assert ng == nr, (ng, nr)
    assert np.array_equal(fg, fr), _diff(fg, fr)
    return nr


def check_frame(oracle, S, check_ori, tz=0.0, mono=True, th=15.0):
    last = E.last_frame(S, tz)
    last_mp = np.arange(len(S.u), dtype=np.int32)
    cg, cr = S.frame_mp0.copy(), S.frame_mp0.copy()
    ng = ORBmatcher(0.9, check_ori).SearchByProjectionFrame(S.F, cg, last, last_mp, S.mps, th, mono)
    nr = oracle.sbp_frame(S.F, cr, last, last_mp, S.mps, th, mono, check_ori)
    assert ng == nr, (ng, nr)
    assert np.array_equal(cg, cr), _diff(cg, cr)
    return nr


def check_keyframe(oracle, S, check_ori=True, th=10.0, orb_dist=100):
    kf = E.last_frame(S)
    kf_mp = np.arange(len(S.u), dtype=np.int32)
    cg, cr = S.frame_mp0.copy(), S.frame_mp0.copy()
    ng = ORBmatcher(0.9, check_ori).SearchByProjectionKeyFrame(S.F, cg, kf, kf_mp, S.mps, th, orb_dist)
    nr = oracle.sbp_keyframe(S.F, cr, kf, kf_mp, S.mps, th, orb_dist, check_ori)
    assert ng == nr, (ng, nr)
    assert np.array_equal(cg, cr), _diff(cg, cr)
    return nr


def check_sim3(oracle, S, th=10):
    Scw = np.eye(4, dtype=np.float32)[:3]
    g = np.full(len(S.F.keys), -1, np.int32)
    r = g.copy()
    ng = ORBmatcher(0.75, False).SearchByProjectionSim3(S.F, Scw, S.queries, g, S.mps, th)
    nr = oracle.sbp_sim3(S.F, Scw, S.queries, r, S.mps, th)
    assert ng == nr, (ng, nr)
    assert np.array_equal(g, r), _diff(g, r)
    return nr


@pytest.fixture(scope="module")
def bounds_scene():
    return E.bounds()


@pytest.fixture(scope="module")
def missing_top_scene():
    return E.missing_top()


def test_bounds_local(oracle, orbx_built, bounds_scene):
    assert check_local(oracle, bounds_scene) >= 500
    assert check_local(oracle, bounds_scene, th=3.0, nnratio=0.6) >= 100
    assert check_local(oracle, bounds_scene.wide, th=E.WIDE_TH) >= 3   # every cell in the window


@pytest.mark.parametrize("check_ori", [True, False])
def test_bounds_frame(oracle, orbx_built, bounds_scene, check_ori):
    assert check_frame(oracle, bounds_scene, check_ori) >= 100


def test_bounds_keyframe_sim3(oracle, orbx_built, bounds_scene):
    assert check_keyframe(oracle, bounds_scene) >= 100
    assert check_sim3(oracle, bounds_scene) >= 100


@pytest.mark.parametrize("half_zero,shuffled", [(False, False), (False, True), (True, False), (True, True)])
def test_one_cell_local(oracle, orbx_built, half_zero, shuffled):
    assert check_local(oracle, E.one_cell(half_zero=half_zero, shuffled=shuffled)) == 600


def test_one_cell_off_grid(oracle, orbx_built):
    S = E.one_cell(off_grid=True)
    fg = S.frame_mp0.copy()
    assert ORBmatcher(0.8, False).SearchByProjectionLocal(S.F, fg, S.queries, S.mps, S.trk, E.OFF_GRID_TH) == 0
    assert np.array_equal(fg, S.frame_mp0)
    assert check_local(oracle, S, th=E.OFF_GRID_TH) == 0


@pytest.mark.parametrize("check_ori", [True, False])
def test_one_cell_frame(oracle, orbx_built, check_ori):
    """(The angles are random: the rotation check keeps three bins of thirty, 82 of 600.)"""
    floor = 50 if check_ori else 600
    assert check_frame(oracle, E.one_cell(), check_ori) >= floor
    assert check_frame(oracle, E.one_cell(half_zero=True, shuffled=True), check_ori, th=7.0) >= floor


@pytest.mark.parametrize("kind", E.LINES)
def test_lines_local(oracle, orbx_built, kind):
    assert check_local(oracle, E.lines(kind)) >= (1 if kind in ("n1", "nq1") else 100)


@pytest.mark.parametrize("nlevels", E.LEVELS)
def test_levels_local_frame(oracle, orbx_built, nlevels):
    S = E.levels(nlevels)
    assert 2 * check_local(oracle, S) >= len(S.queries)
    for check_ori in (True, False):
        assert check_frame(oracle, S, check_ori) >= 100


def test_missing_top_local(oracle, orbx_built, missing_top_scene):
    """Queries whose octave range lies wholly above the frame's highest populated octave
    match nothing (Frame.cc:515-521), though they sit on a keypoint with their descriptor."""
    S = missing_top_scene
    assert check_local(oracle, S) >= 200
    fg = S.frame_mp0.copy()
    ORBmatcher(0.8, False).SearchByProjectionLocal(S.F, fg, S.queries, S.mps, S.trk, 1.0)
    assert not np.isin(fg, S.high).any()
    # level 5 straddles the highest populated octave (range [4, 5], an empty bucket beside a
    # populated one): those queries still take the octave-4 keypoint under them
    l5 = np.nonzero(S.level[:len(S.target)] == 5)[0]
    assert sum(fg[S.target[q]] == q for q in l5) >= 20


@pytest.mark.parametrize("check_ori", [True, False])
def test_missing_top_frame(oracle, orbx_built, check_ori):
    """The frame overload, non-monocular: forward (octaves [nLastOctave, inf): the high
    queries find nothing), backward ([0, nLastOctave]) and neither."""
    S = E.missing_top(stereo=True)
    assert check_frame(oracle, S, check_ori, tz=1.0, mono=False) >= 100
    cg = S.frame_mp0.copy()
    ORBmatcher(0.9, check_ori).SearchByProjectionFrame(S.F, cg, E.last_frame(S, 1.0), np.arange(len(S.u), dtype=np.int32),
                                                       S.mps, 15.0, False)
    assert not np.isin(cg, S.high).any()
    assert check_frame(oracle, S, check_ori, tz=-1.0, mono=False) >= 100
    assert check_frame(oracle, S, check_ori, tz=0.0, mono=False) >= 100


def test_missing_top_keyframe_sim3(oracle, orbx_built, missing_top_scene):
    assert check_keyframe(oracle, missing_top_scene) >= 100
    assert check_sim3(oracle, missing_top_scene) >= 100


# ---- Fuse, FuseSim3, SearchBySim3, SearchForInitialization: their own window code

def _window_scenes():
    return [E.bounds()] + [E.lines(k) for k in E.LINES]


@pytest.fixture(scope="module", params=range(1 + len(E.LINES)), ids=("bounds",) + E.LINES)
def window_scene(request):
    return _window_scenes()[request.param]


def test_fuse(oracle, orbx_built, window_scene):
    S = window_scene
    rng = np.random.default_rng(1)
    skip = (rng.random(len(S.u)) < 0.1).astype(np.uint8)
    m = ORBmatcher(0.6, True)
    for th in (3.0, 8.0):
        got, ref = m.Fuse(S.F, S.queries, skip, S.mps, th), oracle.fuse(S.F, S.queries, skip, S.mps, th)
        assert np.array_equal(got, ref), _diff(got, ref)
    Scw = np.eye(4, dtype=np.float32)[:3]
    got, ref = m.FuseSim3(S.F, Scw, S.queries, skip, S.mps, 4.0), oracle.fuse_sim3(S.F, Scw, S.queries, skip, S.mps, 4.0)
    assert np.array_equal(got, ref), _diff(got, ref)
    assert (ref >= 0).sum() >= (1 if len(S.u) == 1 or len(S.F.keys) == 1 else 50)


def test_search_by_sim3(oracle, orbx_built, window_scene):
    """KF1 = the queries' keyframe (MapPoints 0..m-1), KF2 = the scene's frame, whose keypoints
    carry MapPoints m..m+n-1 at depth Z on their rays; both poses the identity."""
    S = window_scene
    F = S.F
    m1, n2 = len(S.u), len(F.keys)
    rng = np.random.default_rng(2)
    S2 = E.scene(F, F.keys["x"], F.keys["y"], F.keys["octave"], F.desc, rng)
    a, b = S.mps, S2.mps
    cat = lambda x, y: np.concatenate([x, y])  # noqa: E731
    mps = MapPoints(desc=cat(a.desc, b.desc), observations=cat(a.observations, b.observations), pos=cat(a.pos, b.pos),
                    bad=cat(a.bad, b.bad), max_distance=cat(a.max_distance, b.max_distance),
                    min_distance=cat(a.min_distance, b.min_distance), normal=cat(a.normal, b.normal))
    kf1 = E.last_frame(S)
    mp1 = np.arange(m1, dtype=np.int32)
    mp2 = np.arange(m1, m1 + n2, dtype=np.int32)
    mp2[rng.random(n2) < 0.1] = -1
    got = np.full(m1, -1, np.int32)
    ref = got.copy()
    R12, t12 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    ng = ORBmatcher(0.75, True).SearchBySim3(kf1, mp1, F, mp2, got, mps, 1.0, R12, t12, 7.5)
    nr = oracle.search_by_sim3(kf1, mp1, None, F, mp2, None, mps, 1.0, R12, t12, 7.5, ref)
    assert ng == nr and np.array_equal(got, ref), (ng, nr, _diff(got, ref))
    assert nr >= (0 if m1 == 1 or n2 == 1 else 30)


def test_search_for_initialization(oracle, orbx_built, window_scene):
    """F1 = the queries as level-0 keypoints, F2 = the scene's frame with every octave 0
    (the initialiser matches level 0 only), windowSize 10."""
    S = window_scene
    f1 = E.last_frame(S)
    f1.keys["octave"] = 0
    k2 = S.F.keys.copy()
    k2["octave"] = 0
    f2 = E.frame(k2, S.F.desc, 8, bounds=(S.F.min_x, S.F.max_x, S.F.min_y, S.F.max_y))
    for check_ori in (True, False):
        pg = np.ascontiguousarray(np.stack([S.u, S.v], 1).astype(np.float32))
        pr = pg.copy()
        ng, mg = ORBmatcher(0.9, check_ori).SearchForInitialization(f1, f2, pg, 10)
        nr, mr, pr = oracle.search_for_initialization(f1, f2, pr, 10, 0.9, check_ori)
        assert ng == nr and np.array_equal(mg, mr), (ng, nr, _diff(mg, mr))
        assert np.array_equal(pg.view(np.uint32), pr.view(np.uint32))
        assert nr >= (1 if len(S.u) == 1 or len(S.F.keys) == 1 else 200)


# ---- replay widths on the truncation -> re-scoring path

@pytest.fixture(scope="module")
def one_cell_refs(oracle):
    out = []
    for kw in (dict(), dict(half_zero=True, shuffled=True)):
        S = E.one_cell(**kw)
        fr = S.frame_mp0.copy()
        out.append((S, fr, oracle.sbp_local(S.F, fr, S.queries, S.mps, S.trk, 1.0, 0.8)))
    return out


@pytest.mark.parametrize("width", [64, 128, 256, 512, 1024])
def test_one_cell_replay_widths(orbx_built, one_cell_refs, switch, capfd, width):
    """Every replay width on lists that run out.  The diagnostic line's re-scored count is
    required on the blocking scene in group order: the workgroup replays (128 threads and up)
    report the count of their first wave only, and there queries 12-19 of the first group
    are in it at every width.  (On the shuffled scene the 128-thread replay reports 0 with
    every result right: its exhausted queries sit in the second wave.)"""
    switch("replay_threads", width)
    switch("call_stamps", 1)
    for k, (S, fr, nr) in enumerate(one_cell_refs):
        fg = S.frame_mp0.copy()
        ng = ORBmatcher(0.8, False).SearchByProjectionLocal(S.F, fg, S.queries, S.mps, S.trk, 1.0)
        err = capfd.readouterr().err
        assert ng == nr == 600 and np.array_equal(fg, fr), (k, _diff(fg, fr))
        line = re.search(r"\[orbx call\] n=600 nq=600 .*replay \((\d+) threads\).* (\d+) re-scored", err)
        assert line, err
        assert int(line.group(1)) == width, line.group(0)
        if k == 0:
            assert int(line.group(2)) > 0, line.group(0)


# ---- the single calls' size limits

@pytest.mark.parametrize("n,nq", E.CAPACITY)
def test_capacity(oracle, orbx_built, n, nq):
    S = E.capacity(n, nq)
    assert len(S.F.keys) == n and len(S.queries) == nq
    assert check_local(oracle, S) >= (5000 if n == 8191 else 900)


def test_capacity_frame_overload(oracle, orbx_built):
    assert check_frame(oracle, E.capacity(1000, 9000), True) >= 500


def test_capacity_refused(orbx_built):
    """n >= 8192: ORBX_ERR_UNSUPPORTED with a message naming the limit, before any device
    work (a matcher that has never run anything refuses the same way), the arrays untouched."""
    n, nq = E.CAPACITY_REFUSED
    S = E.capacity(n, nq)
    fg = S.frame_mp0.copy()
    fg[::5] = 7
    keep = fg.copy()
    m = ORBmatcher(0.8, False)
    with pytest.raises(L.OrbxError, match="8191") as e:
        m.SearchByProjectionLocal(S.F, fg, S.queries, S.mps, S.trk, 1.0)
    assert e.value.code == L.ORBX_ERR_UNSUPPORTED
    assert np.array_equal(fg, keep)
    cur = keep.copy()
    with pytest.raises(L.OrbxError, match="8191") as e:
        m.SearchByProjectionFrame(S.F, cur, E.last_frame(S), np.arange(nq, dtype=np.int32), S.mps, 15.0, True)
    assert e.value.code == L.ORBX_ERR_UNSUPPORTED and np.array_equal(cur, keep)
    # the matcher still works
    S1 = E.lines("n1")
    f1 = S1.frame_mp0.copy()
    assert m.SearchByProjectionLocal(S1.F, f1, S1.queries, S1.mps, S1.trk, 1.0) >= 1


# ---- the batched device forms on hand-uploaded tensors

# the form launch_proj_search chose, at the end of the diagnostic lines under match_stamps
FORM_RE = re.compile(r"\[orbx (stamps|seq stamps|local stamps)\] .*\| form cap=(\d+) max_nq=(\d+) nlevels=(\d+) "
                     r"footprint=(\d+) QLDS=(\d) DLDS=(\d) threads=(\d+) lds=(\d+)")


def run_local_device(m, batch, cap, sf, th=1.0):
    """search_local_points_device on E.device_batch arrays -> (frame_mp (B, cap), nmatches (B,))."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    mps = {k: up(v) for k, v in batch.mps.items()}
    B = len(batch.n)
    d_fmp, d_nm = up(np.full((B, cap), -1, np.int32)), up(np.full(B, -7, np.int32))
    d = [up(batch.kps), up(batch.desc), up(batch.n), up(batch.Tcw)]
    d_ids = up(batch.local_ids if len(batch.local_ids) else np.zeros(1, np.int32))
    torch.cuda.synchronize()
    try:
        m.search_local_points_device(mps, d[0], d[1], d[2], d[3], batch.local_off, d_ids, d_fmp, d_nm, sf, E.FX, E.FY,
                                     E.CX, E.CY, E.W, E.H, th=th)
    finally:
        torch.cuda.synchronize()
        out = d_fmp.cpu().numpy(), d_nm.cpu().numpy()
    return out


def ref_local_device(oracle, scenes, batch, cap, th=1.0, nnratio=0.8):
    B = len(scenes)
    fmp, nm = np.full((B, cap), -1, np.int32), np.zeros(B, np.int32)
    for b, S in enumerate(scenes):
        if S is None:
            continue
        f = np.full(len(S.F.keys), -1, np.int32)
        ids = batch.local_ids[batch.local_off[b]:batch.local_off[b + 1]]
        nm[b] = oracle.search_local_points(S.F, f, ids, batch.table, th, nnratio)
        fmp[b, :len(f)] = f
    return fmp, nm


def run_sequence_device(m, seq, cap, sf, th=15.0):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    B = len(seq.n)
    d_mp, d_nm = up(np.full((B, cap), -9, np.int32)), up(np.full(B, -7, np.int32))
    d = [up(seq.kps), up(seq.desc), up(seq.n), up(seq.Tcw)]
    torch.cuda.synchronize()
    try:
        m.match_sequence_device(d[0], d[1], d[2], d[3], d_mp, d_nm, sf, E.FX, E.FY, E.CX, E.CY, E.W, E.H, depth=E.Z, th=th)
    finally:
        torch.cuda.synchronize()
        out = d_mp.cpu().numpy(), d_nm.cpu().numpy()
    return out


def ref_sequence_device(oracle, frames, cap, check_ori, th=15.0):
    """Per-pair oracle of match_sequence_device: keypoint i of frame p carries MapPoint i at
    depth Z on its ray (float arithmetic as k_seq_build's, identity poses)."""
    B = len(frames)
    mp, nm = np.full((B, cap), -1, np.int32), np.zeros(B, np.int32)
    F32 = np.float32
    for p in range(B - 1):
        last, cur = frames[p], frames[p + 1]
        if last is None or cur is None:
            continue
        lk = last.keys
        Xw = np.stack([(lk["x"] - F32(E.CX)) / F32(E.FX) * F32(E.Z), (lk["y"] - F32(E.CY)) / F32(E.FY) * F32(E.Z),
                       np.full(len(lk), F32(E.Z), np.float32)], 1).astype(np.float32)
        mps = MapPoints(desc=last.desc, observations=np.ones(len(lk), np.int32), pos=Xw)
        ref = np.full(len(cur.keys), -1, np.int32)
        nm[p + 1] = oracle.sbp_frame(cur, ref, last, np.arange(len(lk), dtype=np.int32), mps, th, True, check_ori)
        mp[p + 1, :len(ref)] = ref
    return mp, nm


def _device_scenes(name):
    """B = 3 frames of different n, the middle one empty."""
    if name == "one_cell":
        return [E.one_cell(), None, E.one_cell(seed=1, half_zero=True, shuffled=True, per_group=15)], 8, 1.2
    if name == "missing_top":
        return [E.missing_top(), None, E.missing_top(seed=1, n=700)], 8, 1.2
    nlevels = int(name[1:])
    return [E.levels(nlevels), None, E.levels(nlevels, seed=1, n=500)], nlevels, 1.05


DEVICE_SCENES = ("one_cell", "missing_top") + tuple(f"L{n}" for n in E.LEVELS)


@pytest.mark.parametrize("name", DEVICE_SCENES)
def test_search_local_points_device_edges(oracle, orbx_built, name):
    scenes, nlevels, sfac = _device_scenes(name)
    cap = max(len(S.F.keys) for S in scenes if S is not None) + 13
    batch = E.device_batch(scenes, cap)
    sf = E.scale_factors(nlevels, sfac)
    want_mp, want_nm = ref_local_device(oracle, scenes, batch, cap)
    assert want_nm[0] >= 200 and want_nm[1] == 0 and want_nm[2] >= 100
    m = ORBmatcher(0.8, False)
    for footprint in range(6):
        m.set_footprint(footprint)
        mp, nm = run_local_device(m, batch, cap, sf)
        assert np.array_equal(nm, want_nm), (footprint, nm, want_nm)
        assert np.array_equal(mp, want_mp), (footprint, np.argwhere(mp != want_mp)[:10])


@pytest.mark.parametrize("name", DEVICE_SCENES)
def test_match_sequence_device_edges(oracle, orbx_built, name):
    scenes, nlevels, sfac = _device_scenes(name)
    S0, S2 = scenes[0], scenes[2]
    # pairs: (queries of S0 -> S0's frame), (-> empty), (empty -> queries of S2), (-> S2's frame)
    frames = [E.last_frame(S0), S0.F, None, E.last_frame(S2), S2.F]
    cap = max(len(F.keys) for F in frames if F is not None) + 13
    seq = E.sequence_batch(frames, cap)
    sf = E.scale_factors(nlevels, sfac)
    for check_ori in (True, False):
        want_mp, want_nm = ref_sequence_device(oracle, frames, cap, check_ori)
        # (one_cell's angles are random: the rotation check keeps three bins of thirty)
        assert want_nm[1] >= (50 if check_ori else 400) and want_nm[4] >= (50 if check_ori else 300)
        assert want_nm[2] == want_nm[3] == 0
        m = ORBmatcher(0.9, check_ori)
        for footprint in range(6):
            m.set_footprint(footprint)
            mp, nm = run_sequence_device(m, seq, cap, sf)
            assert np.array_equal(nm, want_nm), (footprint, nm, want_nm)
            assert np.array_equal(mp, want_mp), (footprint, np.argwhere(mp != want_mp)[:10])


REFUSED_CAP = 2661   # 32 levels: the first cap whose bucket tables leave no LDS layout


@pytest.mark.parametrize("cap", [REFUSED_CAP - 1, REFUSED_CAP])
def test_device_forms_32_levels_cap_limit(oracle, orbx_built, cap):
    """32 levels at the largest cap every footprint holds, and at the next: there every
    footprint but the split launches (2) returns ORBX_ERR_UNSUPPORTED and launches nothing
    -- the outputs keep the caller's bytes."""
    scenes, nlevels, sfac = _device_scenes("L32")
    batch = E.device_batch(scenes, cap)
    sf = E.scale_factors(nlevels, sfac)
    want_mp, want_nm = ref_local_device(oracle, scenes, batch, cap)
    frames = [E.last_frame(scenes[0]), scenes[0].F, None]
    seq = E.sequence_batch(frames, cap)
    swant_mp, swant_nm = ref_sequence_device(oracle, frames, cap, True)
    m, ms = ORBmatcher(0.8, False), ORBmatcher(0.9, True)
    refused = []
    for footprint in range(6):
        m.set_footprint(footprint)
        ms.set_footprint(footprint)
        fits = cap < REFUSED_CAP or footprint == 2
        try:
            mp, nm = run_local_device(m, batch, cap, sf)
            assert fits, footprint
            assert np.array_equal(nm, want_nm) and np.array_equal(mp, want_mp), (footprint, nm, want_nm)
        except L.OrbxError as e:
            assert not fits and e.code == L.ORBX_ERR_UNSUPPORTED, (footprint, str(e))
            refused.append(footprint)
        if fits:
            mp, nm = run_sequence_device(ms, seq, cap, sf)
            assert np.array_equal(nm, swant_nm) and np.array_equal(mp, swant_mp), footprint
        else:
            import torch
            dev = torch.device("cuda", 0)
            d_mp = torch.full((3, cap), -9, dtype=torch.int32, device=dev)
            d_nm = torch.full((3,), -7, dtype=torch.int32, device=dev)
            d = [torch.from_numpy(a).to(dev) for a in (seq.kps, seq.desc, seq.n, seq.Tcw)]
            torch.cuda.synchronize()
            with pytest.raises(L.OrbxError) as e:
                ms.match_sequence_device(d[0], d[1], d[2], d[3], d_mp, d_nm, sf, E.FX, E.FY, E.CX, E.CY, E.W, E.H,
                                         depth=E.Z)
            torch.cuda.synchronize()
            assert e.value.code == L.ORBX_ERR_UNSUPPORTED
            assert (d_mp.cpu().numpy() == -9).all() and (d_nm.cpu().numpy() == -7).all()
    assert refused == ([] if cap < REFUSED_CAP else [0, 1, 3, 4, 5])


def test_local_device_refusal_leaves_outputs(orbx_built):
    """The refused local-map call wrote nothing: frame_mp and nmatches keep the caller's bytes."""
    import torch
    scenes, nlevels, sfac = _device_scenes("L32")
    batch = E.device_batch(scenes, REFUSED_CAP)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    mps = {k: up(v) for k, v in batch.mps.items()}
    d_fmp, d_nm = up(np.full((3, REFUSED_CAP), 3, np.int32)), up(np.full(3, -7, np.int32))
    d = [up(batch.kps), up(batch.desc), up(batch.n), up(batch.Tcw)]
    d_ids = up(batch.local_ids)
    m = ORBmatcher(0.8, False)
    torch.cuda.synchronize()
    with pytest.raises(L.OrbxError) as e:
        m.search_local_points_device(mps, d[0], d[1], d[2], d[3], batch.local_off, d_ids, d_fmp, d_nm,
                                     E.scale_factors(nlevels, sfac), E.FX, E.FY, E.CX, E.CY, E.W, E.H)
    torch.cuda.synchronize()
    assert e.value.code == L.ORBX_ERR_UNSUPPORTED
    assert (d_fmp.cpu().numpy() == 3).all() and (d_nm.cpu().numpy() == -7).all()


# ---- which k_proj_search instantiation runs (footprint 0, 8 levels)

# (cap, max_nq, <QLDS, DLDS>): one triple well inside each form, and the last size that fits
# and the next at each switch.  max_nq == cap: match_sequence_device; else the local-map form.
FORMS = [(600, 600, (1, 1)), (1213, 1213, (1, 1)), (1214, 1214, (0, 1)), (2000, 2000, (0, 1)), (2741, 2741, (0, 1)),
         (2742, 2742, (0, 0)), (3500, 3500, (0, 0)),
         (2741, 500, (0, 1)), (2742, 500, (1, 0)), (3500, 500, (1, 0)), (4464, 500, (1, 0)), (4465, 500, (0, 0))]


@pytest.mark.parametrize("cap,max_nq,form", FORMS)
def test_forms(oracle, orbx_built, switch, capfd, cap, max_nq, form):
    sf = E.scale_factors(8, 1.2)
    switch("match_stamps", 1)
    if max_nq == cap:
        S = E.uniform(cap, cap, cap, 8)
        frames = [E.last_frame(S), S.F]
        seq = E.sequence_batch(frames, cap)
        want_mp, want_nm = ref_sequence_device(oracle, frames, cap, True)
        assert want_nm[1] >= cap // 4
        mp, nm = run_sequence_device(ORBmatcher(0.9, True), seq, cap, sf)
        kind = "stamps"
    else:
        scenes = [E.uniform(cap, cap, max_nq, 8), E.uniform(cap + 1, cap // 2, 300, 8)]
        batch = E.device_batch(scenes, cap)
        want_mp, want_nm = ref_local_device(oracle, scenes, batch, cap)
        assert want_nm[0] >= max_nq // 4
        mp, nm = run_local_device(ORBmatcher(0.8, False), batch, cap, sf)
        kind = "local stamps"
    err = capfd.readouterr().err
    assert np.array_equal(nm, want_nm), (nm, want_nm)
    assert np.array_equal(mp, want_mp), np.argwhere(mp != want_mp)[:10]
    got = [r for r in FORM_RE.findall(err) if r[0] == kind]
    assert len(got) == 1, err
    _, rcap, rnq, rlev, rfoot, qlds, dlds, threads, lds = got[0]
    assert (int(rcap), int(rlev), int(rfoot), int(threads)) == (cap, 8, 0, 1024)
    assert int(rnq) == max_nq
    assert (int(qlds), int(dlds)) == form, got[0]
    assert 0 < int(lds) <= 160 * 1024 - 256
