"""KeyFrameCulling, the full SetBadFlag, MapPointCulling and Observations() on the device
(csrc/orbx_culling.hip) against the model (tests/culling_model.py): the same arrays go to the
device graph and to the model, one call runs in each, and the two are compared.  Integers, flags
and copied bytes only: every comparison is exact."""
from __future__ import annotations

import numpy as np
import pytest

import covisibility_model as M
import culling_model as C
import local_map_model as LM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(orbx_built):
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(params=[None, 8], ids=["lds", "global"])
def lds_bound(request, orbx_built):
    """Both histogram paths of the re-order."""
    from orbslam2commentedbyxcm_amd import _lib as L
    if request.param is not None:
        L.debug_set("covis_lds_keyframes", request.param)
    yield request.param
    L.debug_set("covis_lds_keyframes", -1)


@pytest.fixture(params=[0, 1], ids=["speculative", "serial"])
def serial(request, orbx_built):
    """Both forms of the walk."""
    from orbslam2commentedbyxcm_amd import _lib as L
    L.debug_set("cull_serial", request.param)
    yield request.param
    L.debug_set("cull_serial", -1)


class Scene:
    """A culling scene in HBM with the device graph, and the model graph over its own copy."""

    def __init__(self, dev, m, max_conn=64, io=None, decoy=None):
        """io: a stream_order I/O object for the float tables' uploads (default: blocking ones);
        decoy: the scene (decoy_scene) whose tables are in place until an ordered run's real
        uploads.  The integer map tables, which the graph is built from here, are the real ones."""
        import torch

        from orbslam2commentedbyxcm_amd import CovisibilityGraph, MapCuller
        from orbslam2commentedbyxcm_amd import _lib as L
        self.m = C.copy_maps(m)
        self.mg = C.build_graph(self.m, max_conn)
        self.dev = dev
        self.t = t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        K, cap = m["kf_mp"].shape
        keys = np.zeros((K, cap), L.KEYPOINT_DTYPE)
        keys["octave"] = m["octave"]
        self.d = {"kf_mp": t(m.get("kf_mp0", m["kf_mp"])), "kf_bad": t(m["kf_bad"]), "mp_bad": t(m["mp_bad"]),
                  "kf_keys_un": t(keys.view(np.uint8).reshape(K, cap, 28)),
                  **{dk: t(m[mk]) if io is None else io.up(m[mk], (decoy or m)[mk])
                     for dk, mk in (("kf_u_right", "u_right"), ("kf_depth", "depth"), ("kf_th_depth", "th_depth"))},
                  "kf_not_erase": None if m["not_erase"] is None else t(m["not_erase"]),
                  "kf_to_be_erased": t(m["to_be_erased"])}
        self.d_kf_n = t(m["kf_n"])
        self.g = CovisibilityGraph(K, cap, len(m["mp_bad"]), max_conn)
        torch.cuda.synchronize()
        self.refresh()
        self.g.update_connections(list(range(K)))
        if "kf_mp0" in m:
            torch.cuda.synchronize()
            self.d["kf_mp"].copy_(t(m["kf_mp"]))
            torch.cuda.synchronize()
            self.refresh()
            self.g.update_connections(m["update_ids"])
        self.cull = MapCuller(self.g, self.d)

    def refresh(self):
        self.g.refresh_observations(self.d["kf_mp"], self.d_kf_n, self.d["kf_bad"], self.d["mp_bad"])

    def check_state(self):
        """The map's arrays and every array of the graph equal the model's."""
        import torch
        torch.cuda.synchronize()
        for dk, mk in (("kf_mp", "kf_mp"), ("kf_bad", "kf_bad"), ("mp_bad", "mp_bad"), ("kf_to_be_erased", "to_be_erased")):
            got = self.d[dk].cpu().numpy()
            assert np.array_equal(got, self.m[mk]), (dk, np.argwhere(got != self.m[mk])[:5])
        st = self.g.state()
        M.assert_same_state(self.mg, st)
        assert np.array_equal(st["mp"], self.mg.clean), "cleaned table"
        off, kf, idx = M.observation_csr(self.mg.obs)
        assert np.array_equal(st["obs_off"], off) and np.array_equal(st["obs_kf"], kf) and np.array_equal(st["obs_idx"], idx)
        return st

    def keyframe_culling(self, monocular=None):
        """One call on the device and in the model; asserts equality and returns the model's result."""
        m = self.m
        mono = m["monocular"] if monocular is None else monocular
        want = C.key_frame_culling(self.mg, m, m["cur"], mono, m["not_erase"])
        self.cull.keyframe_culling(m["cur"], mono)
        got = self.cull.state()
        n = len(want["cand"])
        assert int(got["n_cand"][0]) == n and got["cand"][:n].tolist() == want["cand"].tolist()
        assert got["cand_counts"][:n].tolist() == want["cand_counts"].tolist()
        assert int(got["n_culled"][0]) == len(want["culled"])
        assert got["culled"][:len(want["culled"])].tolist() == want["culled"].tolist()
        assert int(got["n_new_bad_mp"][0]) == want["n_new_bad_mp"] and int(got["status"][0]) == want["status"]
        self.check_state()
        return want

    def set_bad_flag(self, ids, not_erase="scene"):
        ne = self.m["not_erase"] if isinstance(not_erase, str) else not_erase
        nb = st = 0
        for k in ids:
            _, s, b = C.set_bad_flag(self.mg, self.m, int(k), ne)
            nb, st = nb + b, st | s
        self.cull.set_bad_flag(ids)
        got = self.cull.state()
        assert int(got["n_new_bad_mp"][0]) == nb and int(got["status"][0]) == st
        return self.check_state()

    def map_point_culling(self, recent, found, visible, first, cur_id, monocular, max_recent):
        import torch
        kept, n = C.map_point_culling(self.mg, self.m, recent, cur_id, monocular, found, visible, first)
        buf = np.full(max_recent, -7, np.int32)
        buf[:len(recent)] = recent
        d_recent, d_n = self.t(buf), self.t(np.array([len(recent)], np.int32))
        torch.cuda.synchronize()
        d_c = self.cull.map_point_culling(cur_id, monocular, d_recent, d_n, self.t(first), self.t(found), self.t(visible))
        torch.cuda.synchronize()
        assert int(d_n[0]) == len(kept) and d_recent.cpu().numpy()[:len(kept)].tolist() == kept and int(d_c[0]) == n
        self.check_state()
        return kept, n

    def close(self):
        self.g.close()


CULL_KEYS = ("cand", "cand_counts", "n_cand", "culled", "n_culled", "n_new_bad_mp", "status", "counts", "kf_mp", "kf_bad",
             "mp_bad", "kf_to_be_erased")
CULL_PAYLOAD = ("u_right", "depth", "th_depth")


def decoy_scene(m):
    """The culling scene with the same map and octaves; other stereo flags, depths and close-point
    thresholds (any mixture is a valid scene: they only decide which points count)."""
    d = dict(m)
    d["u_right"] = np.where(m["u_right"] >= 0, np.float32(-1.0), np.float32(5.0)).astype(np.float32)
    d["depth"] = (np.asarray(m["depth"], np.float32)[:, ::-1] * np.float32(3.0) + np.float32(0.5)).astype(np.float32)
    d["th_depth"] = (np.asarray(m["th_depth"], np.float32) * np.float32(0.25) + np.float32(0.125)).astype(np.float32)
    return d


SET_BAD_IDS = (9, 0, 12)
SET_BAD_DECOY_IDS = (10, 0, 13)            # in the caller's array once set_bad_flag has returned
MAX_RECENT = 150


def recent_inputs(m, max_conn=64):
    """map_point_culling's tables for the scene and their decoy: the same length of list, other
    valid ids in it, other found / visible counters and first keyframes."""
    mm = C.copy_maps(m)
    recent, found, visible, first = C.recent_case(mm, C.build_graph(mm, max_conn), 3, MAX_RECENT)
    buf = np.full(MAX_RECENT, -7, np.int32)
    buf[:len(recent)] = recent
    real = dict(recent=buf, n=np.array([len(recent)], np.int32), first=np.asarray(first, np.int32),
                found=np.asarray(found, np.int32), visible=np.asarray(visible, np.int32))
    dbuf = buf.copy()
    dbuf[:len(recent)] = np.asarray(recent)[::-1]
    decoy = dict(recent=dbuf, n=real["n"], first=np.roll(real["first"], 7), found=real["visible"][::-1].copy(),
                 visible=(real["found"][::-1] + 1).astype(np.int32))
    return real, decoy


def run_culling(dev, m, io=None, decoy=None, mode="keyframe"):
    """On io's stream over a fresh graph (culling changes it), nothing read back in between:
    mode "keyframe": covis_observation_counts_device -> keyframe_culling_device;
    mode "set_bad": covis_set_bad_flag_device of SET_BAD_IDS (a host array);
    mode "map_points": map_point_culling_device of recent_inputs(m).
    io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    calls); decoy: decoy_scene(m) (and recent_inputs' decoy) in place before the real uploads."""
    import torch

    import stream_order as SO
    io = io or SO.SyncIO(dev)
    sc = Scene(dev, m, io=io, decoy=decoy)
    counts = io.full((len(m["mp_bad"]),), -9, torch.int32)
    mono = m["monocular"]
    extra = {}
    if mode == "map_points":
        real, other = recent_inputs(m)
        r = {k: io.up(real[k], other[k] if decoy is not None else None) for k in real}
    io.begin()
    with io.on_stream():
        if mode == "keyframe":
            sc.cull.observation_counts(counts, stream=io.stream)
            io.end()
            t = sc.cull.keyframe_culling(m["cur"], mono, stream=io.stream)
        elif mode == "set_bad":
            ids = io.host(np.asarray(SET_BAD_IDS, np.int32), np.asarray(SET_BAD_DECOY_IDS, np.int32))
            t = sc.cull.set_bad_flag(ids, stream=io.stream)
        else:
            n_culled = sc.cull.map_point_culling(10, mono, r["recent"], r["n"], r["first"], r["found"], r["visible"],
                                                 stream=io.stream)
            t = sc.cull._buffers()
            extra = dict(recent=io.down(r["recent"]), n_recent=io.down(r["n"]), n_mp_culled=io.down(n_culled))
        io.end()
    got = {k: io.down(t[k]) for k in ("cand", "cand_counts", "n_cand", "culled", "n_culled", "n_new_bad_mp", "status")}
    got.update(counts=io.down(counts), **{k: io.down(sc.d[k]) for k in ("kf_mp", "kf_bad", "mp_bad", "kf_to_be_erased")})
    got.update(extra)
    got["scene"] = sc                                 # the graph lives until the caller has synchronised
    return got


def test_run_culling_set_bad_and_map_points_equal_the_model(torch_dev):
    """The other two modes of the stream-order tests' runner against the model."""
    m = C.SCENES["band"]()
    got = run_culling(torch_dev, m, mode="set_bad")
    sc = got["scene"]
    nb = st = 0
    for k in SET_BAD_IDS:
        _, s_, b_ = C.set_bad_flag(sc.mg, sc.m, int(k), m["not_erase"])
        nb, st = nb + b_, st | s_
    assert int(got["n_new_bad_mp"][0]) == nb and int(got["status"][0]) == st
    sc.check_state()
    sc.close()
    got = run_culling(torch_dev, m, mode="map_points")
    sc = got["scene"]
    real, _ = recent_inputs(m)
    n0 = int(real["n"][0])
    kept, n = C.map_point_culling(sc.mg, sc.m, real["recent"][:n0], 10, m["monocular"], real["found"], real["visible"],
                                  real["first"])
    assert int(got["n_recent"][0]) == len(kept) and got["recent"][:len(kept)].tolist() == list(kept)
    assert int(got["n_mp_culled"][0]) == n
    sc.check_state()
    sc.close()


def test_run_culling_equals_the_model(torch_dev):
    """The runner of the stream-order tests against the model."""
    m = C.SCENES["band"]()
    got = run_culling(torch_dev, m)
    sc = got["scene"]
    want = C.key_frame_culling(sc.mg, sc.m, m["cur"], m["monocular"], m["not_erase"])
    n = len(want["cand"])
    assert int(got["n_cand"][0]) == n and got["cand"][:n].tolist() == want["cand"].tolist()
    assert got["cand_counts"][:n].tolist() == want["cand_counts"].tolist()
    assert got["culled"][:len(want["culled"])].tolist() == want["culled"].tolist() and len(want["culled"]) > 0
    assert int(got["n_new_bad_mp"][0]) == want["n_new_bad_mp"] and int(got["status"][0]) == want["status"]
    sc.check_state()
    sc.close()


@pytest.mark.parametrize("name", list(C.SCENES))
def test_keyframe_culling_equals_the_model(torch_dev, lds_bound, serial, name):
    sc = Scene(torch_dev, C.SCENES[name]())
    sc.check_state()
    sc.keyframe_culling()
    sc.keyframe_culling()  # again, on what the first call left
    sc.close()


@pytest.mark.parametrize("name", ["bounds", "band"])
def test_keyframe_culling_with_the_other_sensor(torch_dev, serial, name):
    m = C.SCENES[name]()
    sc = Scene(torch_dev, m)
    sc.keyframe_culling(monocular=not m["monocular"])
    sc.close()


def test_rows_past_one_pass_and_a_long_recent_list(torch_dev, lds_bound, serial):
    """cap = 1100: the strided loop over a row, observers at indices >= 1024, and 1500 recent points."""
    m = C.big_scene()
    sc = Scene(torch_dev, m)
    want = sc.keyframe_culling()
    assert len(want["culled"]) >= 2
    recent, found, visible, first = C.recent_case(sc.m, sc.mg, 9, 1500)
    kept, n = sc.map_point_culling(recent, found, visible, first, 10, False, 1600)
    assert n > 100 and len(kept) > 100 and max(recent.tolist().index(p) for p in kept) >= 1024
    sc.close()


@pytest.mark.parametrize("monocular", [False, True])
def test_map_point_culling_equals_the_model(torch_dev, monocular):
    sc = Scene(torch_dev, C.SCENES["band"]())
    recent, found, visible, first = C.recent_case(sc.m, sc.mg, 3, 150)
    sc.map_point_culling(recent, found, visible, first, 10, monocular, 150)
    sc.map_point_culling(np.zeros(0, np.int32), found, visible, first, 10, monocular, 150)  # an empty list
    sc.close()


@pytest.mark.parametrize("name,ids", [("late", [C.LATE["X"], C.LATE["B"]]), ("tree", [C.TREE["B"], C.TREE["C5"]]),
                                      ("band", [9, 0, 12])])
def test_set_bad_flag_of_a_list_equals_single_calls(torch_dev, lds_bound, name, ids):
    a = Scene(torch_dev, C.SCENES[name]())
    b = Scene(torch_dev, C.SCENES[name]())
    st_a = a.set_bad_flag(ids)
    for k in ids:
        st_b = b.set_bad_flag([k])
    for key in st_a:
        assert np.array_equal(st_a[key], st_b[key]), key
    assert np.array_equal(a.d["kf_mp"].cpu().numpy(), b.d["kf_mp"].cpu().numpy())
    if name == "late":
        assert a.mg.parent[C.LATE["C"]] == C.LATE["Cp"]
    a.close()
    b.close()


def test_set_erase_after_culling_marked_a_keyframe(torch_dev, serial):
    import torch
    sc = Scene(torch_dev, C.SCENES["bounds"]())
    sc.keyframe_culling()
    assert sc.m["to_be_erased"][7] == 1 and not sc.m["kf_bad"][7]
    torch.cuda.synchronize()
    sc.d["kf_not_erase"].zero_()  # SetErase: mbNotErase = false, then SetBadFlag since mbToBeErased
    torch.cuda.synchronize()
    sc.set_bad_flag([7], not_erase=None)
    assert sc.m["kf_bad"][7] == 1
    sc.close()


def test_culled_keyframe_without_parent_sets_the_status_bit(torch_dev):
    """A keyframe that sees only points of its own was never connected: its parent is still -1."""
    m = C.SCENES["tree"]()
    m["kf_mp"][13] = -1
    m["kf_mp"][13, :3] = [1197, 1198, 1199]
    sc = Scene(torch_dev, m)
    assert sc.mg.parent[13] == -1
    sc.set_bad_flag([13])
    assert int(sc.cull.state()["status"][0]) == C.NO_PARENT and sc.m["kf_bad"][13] == 1
    sc.close()


def test_observation_counts_equal_the_model(torch_dev):
    sc = Scene(torch_dev, C.SCENES["band"]())
    stereo = sc.cull.observation_counts().cpu().numpy()
    assert np.array_equal(stereo, C.observation_counts(sc.mg, sc.m["u_right"]))
    sc.cull.tables["kf_u_right"] = None
    mono = sc.cull.observation_counts().cpu().numpy()
    assert np.array_equal(mono, C.observation_counts(sc.mg, None)) and (stereo > mono).any()
    sc.close()


def test_chain_cull_then_update_local_map_with_the_graphs_own_parents(torch_dev, serial):
    """After a cull the graph's own `parent` is the spanning tree: UpdateLocalMap with no parent
    array equals the local-map model on the model graph after the model's cull."""
    import torch

    from orbslam2commentedbyxcm_amd import LocalMapTracker
    sc = Scene(torch_dev, C.SCENES["band"]())
    want_cull = sc.keyframe_culling()
    assert len(want_cull["culled"]) >= 1
    fm, n = LM.frames(sc.m["kf_mp"], sc.m["mp_bad"], 12, seed=4)
    mk = 48
    want = LM.update_local_map_batch(sc.mg, fm, n, *LM.initial_lists(len(fm), mk), mk, 10 ** 6, 10 ** 6)
    trk = LocalMapTracker(sc.g)
    total = int(want["local_off"][-1]) + 5
    buf = trk.buffers(len(fm), mk, total)
    torch.cuda.synchronize()
    for name, a in zip(("local_kf", "local_kf_n", "ref_kf"), LM.initial_lists(len(fm), mk)):
        buf[name].copy_(sc.t(np.asarray(a, np.int32).reshape(buf[name].shape)))
    d_fm = sc.t(fm)
    torch.cuda.synchronize()
    trk.update_local_map(d_fm, sc.t(n), mk, 10 ** 6, total, d_parent=None)
    LM.assert_same(trk.state(), want, d_fm.cpu().numpy())
    assert (want["status"] & LM.CAPACITY).sum() == 0 and want["counts"][:, 0].max() >= 3
    sc.close()


def test_second_call_finds_nothing_and_leaves_every_byte(torch_dev, serial):
    sc = Scene(torch_dev, C.SCENES["cascade"]())
    sc.keyframe_culling()
    before = sc.check_state()
    tables = {k: v.cpu().numpy().copy() for k, v in sc.d.items() if v is not None}
    want = sc.keyframe_culling()
    assert len(want["culled"]) == 0 and want["n_new_bad_mp"] == 0
    after = sc.check_state()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    for k, v in tables.items():
        assert v.tobytes() == sc.d[k].cpu().numpy().tobytes(), k
    sc.close()


def test_argument_errors_that_need_a_graph(torch_dev):
    import torch

    from orbslam2commentedbyxcm_amd import CovisibilityGraph, MapCuller, OrbxError
    from orbslam2commentedbyxcm_amd import _lib as L
    K, cap, n = 8, 16, 50
    g = CovisibilityGraph(K, cap, n, 8)
    i32 = dict(dtype=torch.int32, device=torch_dev)
    u8 = dict(dtype=torch.uint8, device=torch_dev)
    kf_mp, kf_n = torch.full((K, cap), -1, **i32), torch.zeros((K,), **i32)
    kf_bad, mp_bad = torch.zeros((K,), **u8), torch.zeros((n,), **u8)
    tables = {"kf_mp": kf_mp, "kf_bad": kf_bad, "mp_bad": mp_bad, "kf_keys_un": torch.zeros((K, cap, 28), **u8)}
    cull = MapCuller(g, tables)

    def rejected(f, *a):
        with pytest.raises(OrbxError) as e:
            f(*a)
        assert e.value.code == L.ORBX_ERR_ARG

    rejected(cull.keyframe_culling, 1, True)  # before any refresh
    rejected(cull.set_bad_flag, [1])
    g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
    rejected(cull.keyframe_culling, 1, False)  # no depth tables
    rejected(cull.keyframe_culling, K, True)   # an id outside the graph
    rejected(cull.set_bad_flag, [1, K])
    rejected(cull.set_bad_flag, [2, 2])        # a repeated id
    cull.tables["kf_bad"] = torch.zeros((K,), **u8)  # not the array the graph kept
    rejected(cull.keyframe_culling, 1, True)
    cull.tables["kf_bad"] = kf_bad
    cull.keyframe_culling(1, True)             # an empty map: nothing to do
    cull.set_bad_flag([])
    assert int(cull.state()["n_cand"][0]) == 0
    # the host form owns a copy of the map
    h_mp, h_n = np.full((K, cap), -1, np.int32), np.zeros(K, np.int32)
    h_kb, h_mb = np.zeros(K, np.uint8), np.zeros(n, np.uint8)
    L.check(L.lib().orbx_covis_refresh_observations(g._h, K, L.i32ptr(h_mp), L.i32ptr(h_n), L.u8ptr(h_kb), n, L.u8ptr(h_mb)))
    rejected(cull.keyframe_culling, 1, True)
    g.close()
