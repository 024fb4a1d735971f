"""Tracking::UpdateLocalMap on the device (csrc/orbx_localmap.hip) against the model
(tests/local_map_model.py), the chain UpdateLocalMap -> SearchLocalPoints from device offsets
against the existing host-offset entry point fed with the model's lists, and TrackLocalMap's
tally.  Integers only: every comparison is exact."""
from __future__ import annotations

import types

import numpy as np
import pytest

import local_map_model as LM

pytestmark = pytest.mark.gpu

BIG = 10 ** 6


@pytest.fixture(scope="module")
def torch_dev(orbx_built):
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(params=[None, 8], ids=["lds", "global"])
def lds_bound(request, orbx_built):
    """Both histogram paths: the bound lowered to 8 keyframes sends every scene through the
    global rows."""
    from orbslam2commentedbyxcm_amd import _lib as L
    if request.param is not None:
        L.debug_set("covis_lds_keyframes", request.param)
    yield request.param
    L.debug_set("covis_lds_keyframes", -1)


class Scene:
    """A case's map in HBM with the device graph, the model graph and a tracker."""

    def __init__(self, dev, name, max_mappoints=None):
        import torch

        from orbslam2commentedbyxcm_amd import CovisibilityGraph, LocalMapTracker
        self.c = c = LM.gpu_case(name)
        kf_mp, kf_n, kf_bad, mp_bad = c["map"]
        self.dev = dev
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.K, self.cap = kf_mp.shape
        self.kf_bad = kf_bad  # the model graph reads this array: a change shows in both
        self.g = CovisibilityGraph(self.K, self.cap, max_mappoints or len(mp_bad), c["max_conn"])
        self.d_kf_mp, self.d_kf_n, self.d_kf_bad, self.d_mp_bad = self.t(kf_mp), self.t(kf_n), self.t(kf_bad), self.t(mp_bad)
        torch.cuda.synchronize()
        self.g.refresh_observations(self.d_kf_mp, self.d_kf_n, self.d_kf_bad, self.d_mp_bad)
        self.g.update_connections(list(range(self.K)))
        self.m = LM.build_graph(kf_mp, kf_n, kf_bad, mp_bad, c["later_bad"], c["max_conn"])
        self.push_bad()
        self.g.refresh_observations(self.d_kf_mp, self.d_kf_n, self.d_kf_bad, self.d_mp_bad)
        self.trk = LocalMapTracker(self.g)

    def push_bad(self):
        import torch
        torch.cuda.synchronize()
        self.d_kf_bad.copy_(self.t(self.kf_bad))
        torch.cuda.synchronize()

    def run(self, frame_mp, n, lists, max_local_kf, max_points=BIG, max_total=None, parent=None):
        """One call on the device and in the model from the same in/out arrays; asserts equality
        and returns (the model's arrays, the device's)."""
        import torch
        B = len(frame_mp)
        want = LM.update_local_map_batch(self.m, frame_mp, n, *lists, max_local_kf, max_points,
                                         BIG if max_total is None else max_total, parent=parent)
        total = int(want["local_off"][-1]) + 7 if max_total is None else max_total
        buf = self.trk.buffers(B, max_local_kf, total)
        torch.cuda.synchronize()
        for name, a in zip(("local_kf", "local_kf_n", "ref_kf"), lists):
            buf[name].copy_(self.t(np.asarray(a, np.int32).reshape(buf[name].shape)))
        buf["local_ids"].fill_(-5)
        d_fm = self.t(frame_mp)
        torch.cuda.synchronize()
        self.trk.update_local_map(d_fm, self.t(np.asarray(n, np.int32)), max_local_kf, max_points, total,
                                  d_parent=None if parent is None else self.t(np.asarray(parent, np.int32)))
        got = self.trk.state()
        LM.assert_same(got, want, d_fm.cpu().numpy())
        assert (got["local_ids"][int(want["local_off"][-1]):] == -5).all()  # nothing behind the total
        return want, got

    def close(self):
        self.g.close()


TRACK_KEYS = ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status", "frame_mp", "inliers",
              "ok", "found")
TRACK_OUT_ONLY = ("local_off", "counts", "status", "inliers", "ok")     # the others are inputs as well


def track_inputs(sc, seed=0):
    """frame_mp / n of the scene's case and the tally's flags, counts and found counters."""
    c = sc.c if hasattr(sc, "c") else sc
    rng = np.random.default_rng(seed)
    fm = np.asarray(c["frame_mp"], np.int32)
    n_mp = len(c["map"][3])
    B = len(fm)
    return dict(frame_mp=fm, n=np.asarray(c["n"], np.int32), outlier=(rng.random(fm.shape) < 0.2).astype(np.uint8),
                observations=rng.integers(0, 3, n_mp).astype(np.int32), rec=(np.arange(B) % 2).astype(np.uint8),
                found=rng.integers(0, 9, n_mp).astype(np.int32))


def track_decoy(inp):
    """Another valid set of the same id range: the frames' tables dealt to other frames, other
    flags and counters; the counts are the real ones."""
    rng = np.random.default_rng(91)
    return dict(frame_mp=np.roll(inp["frame_mp"], 1, axis=0)[:, ::-1].copy(), n=inp["n"],
                outlier=(rng.random(inp["outlier"].shape) < 0.4).astype(np.uint8),
                observations=rng.integers(0, 3, len(inp["observations"])).astype(np.int32), rec=inp["rec"],
                found=rng.integers(0, 9, len(inp["found"])).astype(np.int32))


def run_track(sc, inp, io=None, decoy=None):
    """update_local_map -> tally on io's stream with nothing read back in between; the in/out
    lists start empty.  io: a stream_order I/O object (default: blocking uploads, a device
    synchronise around the calls); decoy: the inputs that are in place before an ordered run's
    real uploads."""
    import stream_order as SO
    io = io or SO.SyncIO(sc.dev)
    Q = inp if decoy is None else decoy
    mk = sc.c["max_local_kf"]
    B = len(inp["frame_mp"])
    lists = LM.initial_lists(B, mk)
    want = LM.update_local_map_batch(sc.m, inp["frame_mp"], inp["n"], *lists, mk, BIG, BIG)
    total = int(want["local_off"][-1]) + 7
    d = {k: io.up(inp[k], Q[k]) for k in inp}
    buf = sc.trk.buffers(B, mk, total)
    for name, a in zip(("local_kf", "local_kf_n", "ref_kf"), lists):
        io.put(buf[name], np.asarray(a, np.int32))
    io.put(buf["local_ids"], np.full(total, -5, np.int32))
    io.begin()
    with io.on_stream():
        sc.trk.update_local_map(d["frame_mp"], d["n"], mk, BIG, total, stream=io.stream)
        io.end()
        inl, ok = sc.trk.tally(d["frame_mp"], d["n"], d["outlier"], d["observations"], False, True, d["rec"], d["found"],
                               stream=io.stream)
        io.end()
    got = {k: io.down(buf[k]) for k in ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status")}
    got.update(frame_mp=io.down(d["frame_mp"]), inliers=io.down(inl), ok=io.down(ok), found=io.down(d["found"]), want=want)
    return got


def test_run_track_equals_the_model(torch_dev, lds_bound):
    """The runner of the stream-order tests against the model."""
    name = LM.GPU_CASES[0]
    sc = Scene(torch_dev, name)
    inp = track_inputs(sc)
    got = run_track(sc, inp)
    want = got["want"]
    LM.assert_same({k: got[k] for k in ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status")},
                   want)
    w_fm, w_inl, w_ok, w_found = LM.tally(want["frame_mp"], inp["n"], inp["outlier"], inp["observations"], False, True,
                                          inp["rec"], inp["found"])
    assert np.array_equal(got["frame_mp"], w_fm) and np.array_equal(got["inliers"], w_inl)
    assert np.array_equal(got["ok"], w_ok) and np.array_equal(got["found"], w_found)
    sc.close()


@pytest.mark.parametrize("name", LM.GPU_CASES)
def test_batch_and_single_frames_equal_the_model(torch_dev, lds_bound, name):
    sc = Scene(torch_dev, name)
    c = sc.c
    fm, n, mk = c["frame_mp"], c["n"], c["max_local_kf"]
    B = len(fm)
    for parent in c["parents"]:
        want, got = sc.run(fm, n, LM.initial_lists(B, mk), mk, parent=parent)
        assert (want["status"] & LM.CAPACITY).sum() == 0 and want["local_off"][-1] > 0
        # one frame at a time: the same bytes as its part of the batch
        for b in list(range(min(B, 6))) + [B - 1]:
            w1, g1 = sc.run(fm[b:b + 1], n[b:b + 1], LM.initial_lists(1, mk), mk, parent=parent)
            m = int(g1["local_kf_n"][0])
            assert m == got["local_kf_n"][b] and g1["local_kf"][0, :m].tobytes() == got["local_kf"][b, :m].tobytes()
            assert g1["local_ids"][:g1["local_off"][1]].tobytes() == \
                got["local_ids"][got["local_off"][b]:got["local_off"][b + 1]].tobytes()
            assert g1["ref_kf"][0] == got["ref_kf"][b] and g1["status"][0] == got["status"][b]
        # the same call again, on what the first one left
        lists = (want["local_kf"], want["local_kf_n"], want["ref_kf"])
        again, _ = sc.run(want["frame_mp"], n, lists, mk, parent=parent)
        assert np.array_equal(again["frame_mp"], want["frame_mp"]) and np.array_equal(again["local_ids"], want["local_ids"])
    sc.close()


def test_more_frames_than_workspace_rows(torch_dev):
    """A graph made for 4 Mi MapPoints: a row of marks is 16 MiB, the 256 MiB bound gives 16 rows,
    and the 40 frames share them -- every frame must leave its marks reset, twice over."""
    sc = Scene(torch_dev, "band24", max_mappoints=4 << 20)
    c = sc.c
    mk, B = c["max_local_kf"], len(c["frame_mp"])
    want, _ = sc.run(c["frame_mp"], c["n"], LM.initial_lists(B, mk), mk)
    sc.run(want["frame_mp"], c["n"], (want["local_kf"], want["local_kf_n"], want["ref_kf"]), mk)
    sc.close()


def test_one_frame_over_each_capacity_in_the_middle(torch_dev):
    sc = Scene(torch_dev, "band24")
    c = sc.c
    fm, n, mk = c["frame_mp"], c["n"], c["max_local_kf"]
    full, _ = sc.run(fm, n, LM.initial_lists(len(fm), mk), mk)
    # the keyframe list
    pick = LM.capacity_triple(full["counts"][:, 0])
    mk1 = int(full["counts"][pick[1], 0]) - 1
    w, _ = sc.run(fm[pick], n[pick], LM.initial_lists(3, mk1), mk1)
    assert w["status"].tolist() == [0, LM.CAPACITY, 0]
    # a frame's points, then the batch's
    pick = LM.capacity_triple(full["counts"][:, 1])
    npts = full["counts"][pick, 1].tolist()
    w, _ = sc.run(fm[pick], n[pick], LM.initial_lists(3, mk), mk, max_points=npts[1] - 1)
    assert w["status"].tolist() == [0, LM.CAPACITY, 0]
    w, g = sc.run(fm[pick], n[pick], LM.initial_lists(3, mk), mk, max_total=npts[0] + npts[2] + 1)
    assert w["status"].tolist() == [0, LM.CAPACITY, 0] and g["local_off"].tolist() == [0, npts[0], npts[0], npts[0] + npts[2]]
    assert g["ref_kf"][1] == LM.OLD_REF and g["local_kf_n"].tolist() == [full["counts"][pick[0], 0], 0, full["counts"][pick[2], 0]]
    # the last frame does not fit what the others left
    w, _ = sc.run(fm[pick], n[pick], LM.initial_lists(3, mk), mk, max_total=npts[0] + npts[1] + 1)
    assert w["status"].tolist() == [0, 0, LM.CAPACITY]
    sc.close()


def test_keyframes_that_went_bad_since_the_refresh(torch_dev, lds_bound):
    """kf_bad is read when the call runs: a voted keyframe that is bad now is skipped by strategy 1
    (the observation CSR still holds it), and so are neighbours, children and -- not -- parents."""
    from collections import Counter
    sc = Scene(torch_dev, "band40")
    c = sc.c
    sc.kf_bad[[8, 20, 21, 27]] = 1
    sc.push_bad()
    br = Counter()
    LM.update_local_map_batch(sc.m, c["frame_mp"], c["n"], *LM.initial_lists(40, 48), 48, BIG, BIG, br=br)
    assert br["voted_keyframe_bad"] > 0
    sc.run(c["frame_mp"], c["n"], LM.initial_lists(40, 48), 48)
    sc.close()


def test_argument_errors_that_need_a_graph(torch_dev):
    from orbslam2commentedbyxcm_amd import CovisibilityGraph, LocalMapTracker, OrbxError
    from orbslam2commentedbyxcm_amd import _lib as L
    import torch
    g = CovisibilityGraph(8, 16, 50, 8)
    trk = LocalMapTracker(g)
    fm = torch.full((2, 16), -1, dtype=torch.int32, device=torch_dev)
    n = torch.zeros((2,), dtype=torch.int32, device=torch_dev)
    with pytest.raises(OrbxError) as e:  # before any refresh
        trk.update_local_map(fm, n, 4, 10, 10)
    assert e.value.code == L.ORBX_ERR_ARG
    kf_mp = torch.full((8, 16), -1, dtype=torch.int32, device=torch_dev)
    g.refresh_observations(kf_mp, torch.zeros((8,), dtype=torch.int32, device=torch_dev), None, None, n_mappoints=50)
    with pytest.raises(OrbxError) as e:  # cap differs from the graph's
        trk.update_local_map(torch.full((2, 15), -1, dtype=torch.int32, device=torch_dev), n, 4, 10, 10)
    assert e.value.code == L.ORBX_ERR_ARG
    t = trk.update_local_map(fm, n, 4, 10, 10)  # an empty map: every counter is empty
    st = trk.state()
    assert st["status"].tolist() == [LM.EMPTY, LM.EMPTY] and st["local_off"].tolist() == [0, 0, 0] and t is not None
    g.close()


def test_tally_equals_the_model(torch_dev):
    import torch

    from orbslam2commentedbyxcm_amd import CovisibilityGraph, LocalMapTracker
    rng = np.random.default_rng(7)
    B, cap, n_mp = 9, 300, 500
    fm = rng.integers(-1, n_mp + 4, (B, cap)).astype(np.int32)
    fm[rng.random((B, cap)) < 0.3] = -1
    fm[0] = -1
    n = rng.integers(cap - 5, cap + 5, B).astype(np.int32)
    out = (rng.random((B, cap)) < 0.2).astype(np.uint8)
    out[3, 40:] = 1            # about 28 left: fails 30
    out[4, 60:] = 1            # about 42: fails 50 when recently relocalised
    obs = rng.integers(0, 3, n_mp).astype(np.int32)
    rec = np.array([0, 0, 1, 0, 1, 1, 0, 0, 0], np.uint8)
    found0 = rng.integers(0, 9, n_mp).astype(np.int32)
    g = CovisibilityGraph(4, 8, n_mp, 4)
    trk = LocalMapTracker(g)
    t = lambda a: torch.from_numpy(a).to(torch_dev)  # noqa: E731
    seen = set()
    for only_tracking, stereo in ((False, False), (False, True), (True, True)):
        w_fm, w_inl, w_ok, w_found = LM.tally(fm, n, out, obs, only_tracking, stereo, rec, found0)
        d_fm, d_found = t(fm), t(found0)
        torch.cuda.synchronize()
        inl, ok = trk.tally(d_fm, t(n), t(out), t(obs), only_tracking, stereo, t(rec), d_found)
        torch.cuda.synchronize()
        assert np.array_equal(inl.cpu().numpy(), w_inl) and np.array_equal(ok.cpu().numpy(), w_ok)
        assert np.array_equal(d_fm.cpu().numpy(), w_fm) and np.array_equal(d_found.cpu().numpy(), w_found)
        seen |= set(zip(w_ok.tolist(), rec.tolist()))
    assert seen == {(0, 0), (1, 0), (0, 1), (1, 1)}
    g.close()


# ---- the TrackLocalMap chain of INTEGRATION.md as a runner (tests/test_gpu_stream_order.py) -----------
TLM_TABLE = ("pos", "desc", "normal", "max_distance", "min_distance", "observations", "bad")
TLM_PAYLOAD = {"pos", "desc", "normal", "max_distance", "min_distance", "observations", "kps", "kp_desc", "T"}
TLM_KEYS = ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status", "frame_mp", "nmatches",
            "Tcw_opt", "outlier", "ninliers", "ninit", "inliers", "ok", "found")
TLM_OUT_ONLY = ("local_off", "counts", "status", "nmatches", "Tcw_opt", "ninliers", "ninit", "inliers", "ok")
TLM_INV_SIGMA2 = (1.2 ** (-2.0 * np.arange(8))).astype(np.float32)


def tlm_setup(B=6):
    """The scene of test_chain_update_local_map_search_local_points_tally: a posed sequence whose
    frames are also the keyframes, the graph over it, the model's UpdateLocalMap, and the host
    arrays of every device input."""
    import torch

    import covisibility_model as M
    from orbslam2commentedbyxcm_amd import CovisibilityGraph, LocalMapTracker, ORBmatcher
    from orbslam2commentedbyxcm_amd import _lib as L
    from orbslam2commentedbyxcm_amd.optimizer import PoseOptimizer
    from test_gpu_posed import _mappoint_table, _sequence_on_gpu
    seq = _sequence_on_gpu(types.SimpleNamespace(KEYPOINT_DTYPE=L.KEYPOINT_DTYPE), B, 30)
    cap, n, dev = seq["cap"], seq["n"], seq["dev"]
    tab = _mappoint_table(seq, 31)
    rng = np.random.default_rng(33)
    kf_mp = np.full((B, cap), -1, np.int32)
    for f in range(B):
        kf_mp[f, :n[f]] = f * cap + np.arange(n[f])
        if f > 0:
            sel = np.flatnonzero(rng.random(n[f]) < 0.2)[:n[f - 1]]
            kf_mp[f, sel] = (f - 1) * cap + rng.permutation(n[f - 1])[:len(sel)]
    kf_bad = np.zeros(B, np.uint8)
    mg = M.Graph(B, 16)
    mg.refresh_observations(kf_mp, n, kf_bad, tab["bad"])
    for k in range(B):
        mg.update_connections(k)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    g = CovisibilityGraph(B, cap, B * cap, 16)
    d_map = (t(kf_mp), t(n.astype(np.int32)), t(kf_bad), t(tab["bad"]))
    torch.cuda.synchronize()
    g.refresh_observations(*d_map)
    g.update_connections(list(range(B)))
    torch.cuda.synchronize()
    fmp0 = np.full((B, cap), -1, np.int32)
    for b in range(B):
        nb = [f for f in (b - 1, b + 1) if 0 <= f < B]
        pool = np.concatenate([f * cap + np.arange(n[f]) for f in nb])
        sel = np.flatnonzero(rng.random(n[b]) < 0.25)
        fmp0[b, sel] = rng.choice(pool, len(sel), replace=False)
    mk, max_points = 16, B * cap
    want = LM.update_local_map_batch(mg, fmp0, n, *LM.initial_lists(B, mk), mk, max_points, BIG)
    m = ORBmatcher(0.8, False)
    inp = dict({k: tab[k] for k in TLM_TABLE}, kps=seq["d_kps"].cpu().numpy(), kp_desc=seq["desc"],
               n=n.astype(np.int32), T=np.asarray(seq["T"], np.float32), fmp0=fmp0,
               rec=np.array([0, 1] * (B // 2), np.uint8), found=np.zeros(B * cap, np.int32))
    return dict(seq=seq, dev=dev, B=B, cap=cap, g=g, d_map=d_map, m=m, pose=PoseOptimizer(matcher=m), trk=LocalMapTracker(g),
                mk=mk, max_points=max_points, max_total=int(want["local_off"][-1]) + 11, want=want, inp=inp,
                sf=np.asarray(seq["ex"].GetScaleFactors(), np.float32))


def tlm_decoy(inp):
    """The inputs with the same ids, counts and octaves; positions, descriptors, normals,
    distances, Observations(), keypoint coordinates and poses are others."""
    d = dict(inp)
    d["pos"] = (inp["pos"] + np.float32([0.05, -0.03, 0.04])).astype(np.float32)
    d["desc"] = inp["desc"] ^ np.uint8(0x5A)
    d["kp_desc"] = inp["kp_desc"] ^ np.uint8(0x33)
    d["normal"] = np.ascontiguousarray(inp["normal"][:, ::-1])
    d["max_distance"] = (inp["max_distance"] * np.float32(1.5)).astype(np.float32)
    d["min_distance"] = (inp["min_distance"] * np.float32(0.5)).astype(np.float32)
    d["observations"] = ((inp["observations"] + 1) % 4).astype(np.int32)
    kps = inp["kps"].copy()
    xy = kps[..., :2].view(np.float32)
    xy += np.float32(2.5)
    d["kps"] = kps
    d["T"] = inp["T"].copy()
    d["T"][:, [3, 7, 11]] += np.float32([0.02, -0.01, 0.03])
    return d


def tlm_decoy_offsets(off):
    """Another valid partition of the same list: the inner boundaries halved."""
    o = np.array(off, np.int32, copy=True)
    o[1:-1] = o[1:-1] // 2
    return o


def run_track_chain(st, io=None, decoy=None, inp=None, host_offsets=False):
    """UpdateLocalMap -> SearchLocalPoints from the device offsets -> PoseOptimization -> tally on
    io's stream with nothing read back; the in/out lists start empty.  host_offsets: instead, the
    host-offset search_local_points_device alone on the model's lists (the yardstick of the chain
    test), its host offsets and scale factors given through io.host.  io: a stream_order I/O
    object (default: blocking uploads, a device synchronise around the calls); decoy: tlm_decoy's
    arrays, in place before an ordered run's real uploads."""
    import torch

    import match_scenes as S
    import stream_order as SO
    io = io or SO.SyncIO(st["dev"])
    inp = st["inp"] if inp is None else inp
    Q = inp if decoy is None else decoy
    B, cap, mk, want = st["B"], st["cap"], st["mk"], st["want"]
    d = {k: io.up(inp[k], Q[k]) for k in inp if k != "fmp0"}
    d_tab = {k: d[k] for k in TLM_TABLE}
    d_fmp = io.up(want["frame_mp"] if host_offsets else inp["fmp0"])
    d_nm = io.full((B,), -7, torch.int32)
    cam = (S.FX, S.FY, S.CX, S.CY)
    if host_offsets:
        sf = io.host(st["sf"], st["sf"][::-1].copy())
        d_ids = io.up(want["local_ids"])
        off = io.host(np.asarray(want["local_off"], np.int32), tlm_decoy_offsets(want["local_off"]))
        io.begin()
        st["m"].search_local_points_device(d_tab, d["kps"], d["kp_desc"], d["n"], d["T"], off, d_ids, d_fmp, d_nm, sf, *cam,
                                           640, 480, stream=io.stream)
        io.end()
        return dict(frame_mp=io.down(d_fmp), nmatches=io.down(d_nm))
    buf = st["trk"].buffers(B, mk, st["max_total"])
    for name, a in zip(("local_kf", "local_kf_n", "ref_kf"), LM.initial_lists(B, mk)):
        io.put(buf[name], np.asarray(a, np.int32))
    io.put(buf["local_ids"], np.full(st["max_total"], -5, np.int32))
    d_Tout = io.full((B, 12), float("nan"), torch.float32)
    d_outl = io.full((B, cap), 0, torch.uint8)
    d_ninl, d_nini = io.full((B,), -9, torch.int32), io.full((B,), -9, torch.int32)
    io.begin()
    with io.on_stream():
        lm = st["trk"].update_local_map(d_fmp, d["n"], mk, st["max_points"], st["max_total"], stream=io.stream)
        io.end()
        sf = io.host(st["sf"], st["sf"][::-1].copy())          # a host table is given just before its call:
        st["m"].search_local_points_offsets_device(d_tab, d["kps"], d["kp_desc"], d["n"], d["T"], lm["local_off"],
                                                   lm["local_ids"], d_fmp, d_nm, sf, *cam, 640, 480,
                                                   max_local_points=st["max_points"], max_total=st["max_total"],
                                                   stream=io.stream)
        io.end()                                               # io.end() overwrites it with its decoy
        sig = io.host(TLM_INV_SIGMA2, TLM_INV_SIGMA2[::-1].copy())
        st["pose"].pose_optimization_batch_device(d["kps"], d["n"], d_fmp, d["pos"], sig, *cam, 0.0, d["T"], d_Tout, d_outl,
                                                  d_ninl, d_nini, stream=io.stream)
        io.end()
        inl, ok = st["trk"].tally(d_fmp, d["n"], d_outl, d["observations"], False, False, d["rec"], d["found"],
                                  stream=io.stream)
        io.end()
    got = {k: io.down(buf[k]) for k in ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status")}
    got.update(frame_mp=io.down(d_fmp), nmatches=io.down(d_nm), Tcw_opt=io.down(d_Tout), outlier=io.down(d_outl),
               ninliers=io.down(d_ninl), ninit=io.down(d_nini), inliers=io.down(inl), ok=io.down(ok), found=io.down(d["found"]))
    return got


def tlm_close(st):
    st["m"].close()
    st["g"].close()
    st["seq"]["ex"].close() if hasattr(st["seq"]["ex"], "close") else None


def test_run_track_chain_equals_the_model_and_the_host_offset_search(torch_dev):
    """The runner of the stream-order tests: UpdateLocalMap against the model, the search's
    frame_mp and nmatches against the host-offset entry point on the model's lists, PoseOptimization's
    edge counts against the searched tables (its arithmetic is test_gpu_pose_opt.py's), and the
    tally against the model on PoseOptimization's flags."""
    st = tlm_setup()
    got = run_track_chain(st)
    ref = run_track_chain(st, host_offsets=True)
    want, inp = st["want"], st["inp"]
    LM.assert_same({k: got[k] for k in ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status")},
                   want)
    # the tally rewrites frame_mp: the search's result is what it was before the tally's discards
    w_fm, w_inl, w_ok, w_found = LM.tally(ref["frame_mp"], inp["n"], got["outlier"], inp["observations"], False, False,
                                          inp["rec"], inp["found"])
    assert got["nmatches"].tobytes() == ref["nmatches"].tobytes() and int(got["nmatches"].sum()) > 50 * st["B"]
    assert np.array_equal(got["frame_mp"], w_fm) and np.array_equal(got["inliers"], w_inl)
    assert np.array_equal(got["ok"], w_ok) and np.array_equal(got["found"], w_found) and w_inl.max() > 10
    n_mp = len(inp["pos"])
    for b in range(st["B"]):
        have = int(((ref["frame_mp"][b] >= 0) & (ref["frame_mp"][b] < n_mp))[:inp["n"][b]].sum())
        assert 0 < got["ninliers"][b] <= got["ninit"][b] <= have and np.isfinite(got["Tcw_opt"][b]).all()
    tlm_close(st)


def test_chain_update_local_map_search_local_points_tally(torch_dev):
    """UpdateLocalMap on the device, then SearchLocalPoints from its device offsets: frame_mp and
    nmatches are the bytes of the existing host-offset entry point fed with the model's lists;
    then the tally equals the model."""
    import torch

    import covisibility_model as M
    import match_scenes as S
    from orbslam2commentedbyxcm_amd import CovisibilityGraph, LocalMapTracker, ORBmatcher
    from orbslam2commentedbyxcm_amd import _lib as L
    from test_gpu_posed import _mappoint_table, _sequence_on_gpu

    B = 6
    seq = _sequence_on_gpu(types.SimpleNamespace(KEYPOINT_DTYPE=L.KEYPOINT_DTYPE), B, 30)
    cap, n, dev = seq["cap"], seq["n"], seq["dev"]
    tab = _mappoint_table(seq, 31)
    rng = np.random.default_rng(33)
    # the frames are also the keyframes: keyframe f holds its own MapPoints and, at a fifth of its
    # indices, MapPoints of keyframe f - 1
    kf_mp = np.full((B, cap), -1, np.int32)
    for f in range(B):
        kf_mp[f, :n[f]] = f * cap + np.arange(n[f])
        if f > 0:
            sel = np.flatnonzero(rng.random(n[f]) < 0.2)[:n[f - 1]]
            kf_mp[f, sel] = (f - 1) * cap + rng.permutation(n[f - 1])[:len(sel)]
    kf_bad = np.zeros(B, np.uint8)
    mg = M.Graph(B, 16)
    mg.refresh_observations(kf_mp, n, kf_bad, tab["bad"])
    for k in range(B):
        mg.update_connections(k)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    g = CovisibilityGraph(B, cap, B * cap, 16)
    d_map = (t(kf_mp), t(n.astype(np.int32)), t(kf_bad), t(tab["bad"]))
    torch.cuda.synchronize()
    g.refresh_observations(*d_map)
    g.update_connections(list(range(B)))
    # mvpMapPoints after the motion-model search: a quarter of the keypoints hold a MapPoint of a
    # neighbouring keyframe
    fmp0 = np.full((B, cap), -1, np.int32)
    for b in range(B):
        nb = [f for f in (b - 1, b + 1) if 0 <= f < B]
        pool = np.concatenate([f * cap + np.arange(n[f]) for f in nb])
        sel = np.flatnonzero(rng.random(n[b]) < 0.25)
        fmp0[b, sel] = rng.choice(pool, len(sel), replace=False)
    mk, max_points = 16, B * cap
    want = LM.update_local_map_batch(mg, fmp0, n, *LM.initial_lists(B, mk), mk, max_points, BIG)
    total = int(want["local_off"][-1])
    assert (want["status"] == 0).all() and want["counts"][:, 0].min() >= 2 and total > int(n.sum())
    sf = seq["ex"].GetScaleFactors()
    d_tab = {k: t(v) for k, v in tab.items()}
    d_T = t(seq["T"])
    m = ORBmatcher(0.8, False)
    args = (sf, S.FX, S.FY, S.CX, S.CY, 640, 480)
    # the yardstick: the existing entry point on the model's lists
    d_fmp_ref, d_nm_ref = t(want["frame_mp"]), torch.full((B,), -7, dtype=torch.int32, device=dev)
    m.search_local_points_device(d_tab, seq["d_kps"], seq["d_desc"], seq["d_n"], d_T, want["local_off"],
                                 t(want["local_ids"]), d_fmp_ref, d_nm_ref, *args)
    # the device chain, capacities in place of sizes
    trk = LocalMapTracker(g)
    d_fmp, d_nm = t(fmp0), torch.full((B,), -7, dtype=torch.int32, device=dev)
    max_total = total + 11
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev)
    lm = trk.update_local_map(d_fmp, seq["d_n"], mk, max_points, max_total, stream=s)
    m.search_local_points_offsets_device(d_tab, seq["d_kps"], seq["d_desc"], seq["d_n"], d_T, lm["local_off"],
                                         lm["local_ids"], d_fmp, d_nm, *args, max_local_points=max_points,
                                         max_total=max_total, stream=s)
    torch.cuda.synchronize()
    LM.assert_same(trk.state(), want)
    assert d_fmp.cpu().numpy().tobytes() == d_fmp_ref.cpu().numpy().tobytes()
    assert d_nm.cpu().numpy().tobytes() == d_nm_ref.cpu().numpy().tobytes() and int(d_nm.sum()) > 50 * B
    # the tally on outlier flags as PoseOptimization would leave them
    fmp = d_fmp.cpu().numpy()
    out = (rng.random((B, cap)) < 0.15).astype(np.uint8)
    rec = np.array([0, 1] * (B // 2), np.uint8)
    w_fm, w_inl, w_ok, w_found = LM.tally(fmp, n, out, tab["observations"], False, True, rec, np.zeros(B * cap, np.int32))
    d_found = torch.zeros((B * cap,), dtype=torch.int32, device=dev)
    inl, ok = trk.tally(d_fmp, seq["d_n"], t(out), d_tab["observations"], False, True, t(rec), d_found, stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(inl.cpu().numpy(), w_inl) and np.array_equal(ok.cpu().numpy(), w_ok) and w_inl.max() > 30
    assert np.array_equal(d_fmp.cpu().numpy(), w_fm) and np.array_equal(d_found.cpu().numpy(), w_found)
    m.close()
    g.close()
