"""The device covisibility graph (csrc/orbx_covis.hip) against the model
(tests/covisibility_model.py): the observation CSR, the full state after scripted sequences of
UpdateConnections / erase, the getters, LocalBundleAdjustment's graph assembly and the chain
assemble -> LocalBA -> apply.  Integers and copied float bytes: every comparison is exact."""
from __future__ import annotations

import numpy as np
import pytest

import covisibility_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(orbx_built):
    import torch
    return torch.device("cuda", 0)


class Map:
    """A scene's tables in HBM and a graph over them."""

    def __init__(self, dev, kf_mp, kf_n, kf_bad, mp_bad, max_conn=64, K=None):
        import torch

        from orbslam2commentedbyxcm_amd import CovisibilityGraph
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.kf_mp, self.kf_n, self.kf_bad, self.mp_bad = (np.array(a, copy=True) for a in (kf_mp, kf_n, kf_bad, mp_bad))
        self.K = K or len(kf_mp)
        self.g = CovisibilityGraph(self.K, kf_mp.shape[1], len(mp_bad), max_conn)
        self.m = M.Graph(self.K, max_conn)
        self.d_kf_mp = self.t(self.kf_mp)
        self.d_kf_n, self.d_kf_bad, self.d_mp_bad = self.t(self.kf_n), self.t(self.kf_bad), self.t(self.mp_bad)

    def refresh(self, nk=None):
        nk = len(self.kf_mp) if nk is None else nk
        self.d_kf_mp.copy_(self.t(self.kf_mp))
        self.d_kf_bad.copy_(self.t(self.kf_bad))
        import torch
        torch.cuda.synchronize()
        self.g.refresh_observations(self.d_kf_mp[:nk], self.d_kf_n[:nk], self.d_kf_bad[:nk], self.d_mp_bad)
        self.m.refresh_observations(self.kf_mp[:nk], self.kf_n[:nk], self.kf_bad[:nk], self.mp_bad)

    def update(self, ids):
        self.g.update_connections(ids)
        for k in ids:
            self.m.update_connections(int(k))

    def erase(self, k):
        self.g.erase_keyframe(k)
        self.m.erase_keyframe(k)

    def check(self):
        st = self.g.state()
        M.assert_same_state(self.m, st)
        return st

    def check_observations(self):
        st = self.g.state()
        off, kf, idx = M.observation_csr(self.m.obs)
        assert np.array_equal(st["obs_off"], off)
        assert np.array_equal(st["obs_kf"], kf) and np.array_equal(st["obs_idx"], idx)
        assert np.array_equal(st["mp"][:len(self.m.clean)], self.m.clean)
        assert np.array_equal(st["status"], np.array(self.m.status, np.int32))
        return st

    def close(self):
        self.g.close()


RUN_KEYS = ("best", "best_n", "by_weight", "by_weight_n")


def run_graph(g, tables, ids, io=None, decoy=None, N=10, w=15, erase=None, decoy_ids=None):
    """refresh -> update_connections(ids) -> erase_keyframe -> the two getters, all on io's
    stream with nothing read back in between.  io: a stream_order I/O object (default: blocking
    uploads, a device synchronise around the calls); decoy: the tables that fill the inputs
    before an ordered run's real uploads."""
    import torch

    import stream_order as SO
    dev = torch.device("cuda", g.device)
    io = io or SO.SyncIO(dev)
    d = [io.up(a, b) for a, b in zip(tables, tables if decoy is None else decoy)]
    K = g.max_keyframes
    best, best_n = io.full((K, N), -9, torch.int32), io.full((K,), -9, torch.int32)
    byw, byw_n = io.full((K, g.max_conn), -9, torch.int32), io.full((K,), -9, torch.int32)
    io.begin()
    g.refresh_observations(*d, stream=io.stream)
    io.end()
    h_ids = io.host(np.asarray(ids, np.int32), decoy_ids)
    g.update_connections(h_ids, stream=io.stream)
    io.end()
    if erase is not None:
        g.erase_keyframe(erase, stream=io.stream)
        io.end()
    g.best_covisibles(N, best, best_n, stream=io.stream)
    io.end()
    g.covisibles_by_weight(w, byw, byw_n, stream=io.stream)
    io.end()
    return dict(best=io.down(best), best_n=io.down(best_n), by_weight=io.down(byw), by_weight_n=io.down(byw_n))


CHAIN_KEYS = ("poses", "mp_pos", "kf_mp", "kf_Tcw_opt", "pt_pos_opt", "erase", "level1", "n_erase", "trace", "status")


def chain_decoy(sc):
    """geometric_scene with the same map tables; poses, positions and keypoints moved."""
    d = dict(sc)
    d["poses"] = sc["poses"].copy()
    d["poses"][:, [3, 7, 11]] += np.float32([0.02, -0.01, 0.015])
    d["mp_pos"] = (sc["mp_pos"] + np.float32([0.03, 0.02, -0.04])).astype(np.float32)
    d["xy"] = (sc["xy"] + np.float32([1.25, -0.75])).astype(np.float32)
    d["u_right"] = np.where(sc["u_right"] >= 0, sc["u_right"] + np.float32(0.75), sc["u_right"]).astype(np.float32)
    return d


def chain_arrays(sc):
    """The uploads of run_local_mapping."""
    K, cap = sc["kf_mp"].shape
    kps = keypoints(sc["xy"], sc["octave"]).view(np.uint8).reshape(K, cap, 28)
    return dict(kf_mp=sc["kf_mp"], kf_n=sc["kf_n"], kf_bad=sc["kf_bad"], mp_bad=sc["mp_bad"], poses=sc["poses"],
                mp_pos=sc["mp_pos"], kps=kps, u_right=sc["u_right"])


def run_local_mapping(g, lba, sc, cur=5, io=None, decoy=None):
    """LocalMapping's calls on one stream with nothing read back: refresh_observations ->
    update_connections (all) -> local_ba_assemble -> LocalBundleAdjustment -> local_ba_apply.
    io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    calls); decoy: the scene whose arrays fill the inputs before an ordered run's real uploads."""
    import torch

    import stream_order as SO
    dev = torch.device("cuda", g.device)
    io = io or SO.SyncIO(dev)
    A, Q = chain_arrays(sc), chain_arrays(sc if decoy is None else decoy)
    d = {k: io.up(A[k], Q[k]) for k in A}
    K, cap = sc["kf_mp"].shape
    n_mp = len(sc["mp_bad"])
    rows = {"B": (1,), "B1": (2,), "B3": (1, 3), "K": (K,), "K12": (K, 12), "P": (n_mp,), "P1": (n_mp + 1,),
            "P3": (n_mp, 3), "O": (K * cap,)}
    tables = {name: io.full(rows[shape], 0, getattr(torch, dtype)) for name, shape, dtype in lba.ASSEMBLY_TABLES}
    out = {"kf_Tcw_opt": io.full((K, 12), float("nan"), torch.float32), "pt_pos_opt": io.full((n_mp, 3), float("nan"), torch.float32),
           "erase": io.full((K * cap,), 9, torch.uint8), "level1": io.full((K * cap,), 9, torch.uint8),
           "n_erase": io.full((1,), -9, torch.int32), "trace": io.full((1, 2, 2), -9, torch.int32),
           "status": io.full((1,), -9, torch.int32)}
    fx, fy, cx, cy, bf = sc["cam"]
    io.begin()
    g.refresh_observations(d["kf_mp"], d["kf_n"], d["kf_bad"], d["mp_bad"], stream=io.stream)
    io.end()
    g.update_connections(np.arange(K, dtype=np.int32), stream=io.stream)
    io.end()
    h_cur = io.host(np.asarray([cur], np.int32), np.asarray([cur + 1], np.int32))
    lba.assemble_batch_device(g, h_cur, d["poses"], d["mp_pos"], K, n_mp, K * cap, tables=tables, stream=io.stream)
    io.end()
    sig = io.host(np.asarray(sc["inv_sigma2"], np.float32), np.asarray(sc["inv_sigma2"], np.float32)[::-1])
    lba.local_ba_assembled_device(tables, d["kps"], d["u_right"], sig, fx, fy, cx, cy, bf, out=out, stream=io.stream)
    io.end()
    lba.apply_batch_device(g, tables, out["kf_Tcw_opt"], out["pt_pos_opt"], out["erase"], d["poses"], d["mp_pos"],
                           d["kf_mp"], stream=io.stream)
    io.end()
    got = {k: io.down(v) for k, v in out.items()}
    got.update(poses=io.down(d["poses"]), mp_pos=io.down(d["mp_pos"]), kf_mp=io.down(d["kf_mp"]))
    return got


def model_run(K, max_conn, tables, ids, N=10, w=15, erase=None):
    """run_graph on the model."""
    m = M.Graph(K, max_conn)
    m.refresh_observations(*tables)
    for k in sorted(ids):
        m.update_connections(int(k))
    if erase is not None:
        m.erase_keyframe(erase)
    best, byw = np.full((K, N), -1, np.int32), np.full((K, max_conn), -9, np.int32)
    best_n, byw_n = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for k in range(K):
        a, b = m.best_covisibles(k, N), m.covisibles_by_weight(k, w)
        best[k, :len(a)], best_n[k] = a, len(a)
        byw[k, :len(b)], byw_n[k] = b, len(b)
    return dict(best=best, best_n=best_n, by_weight=byw, by_weight_n=byw_n)


def test_run_graph_equals_model(torch_dev, lds_bound):
    """The runner of the stream-order tests against the model."""
    tables = M.scene(**M.GPU_SCENES["band24"])
    K, cap = tables[0].shape
    from orbslam2commentedbyxcm_amd import CovisibilityGraph
    g = CovisibilityGraph(K, cap, len(tables[3]), 64)
    got = run_graph(g, tables, list(range(K)), erase=7)
    want = model_run(K, 64, tables, list(range(K)), erase=7)
    assert np.array_equal(got["best"], want["best"]) and np.array_equal(got["best_n"], want["best_n"])
    assert np.array_equal(got["by_weight_n"], want["by_weight_n"])
    for k in range(K):
        n = want["by_weight_n"][k]
        assert np.array_equal(got["by_weight"][k, :n], want["by_weight"][k, :n])
    assert want["best_n"].max() > 1 and want["by_weight_n"].max() > 1
    g.close()


@pytest.fixture(params=[None, 8], ids=["lds", "global"])
def lds_bound(request, orbx_built):
    """K on both sides of the LDS-histogram bound: the bound lowered to 8 keyframes sends every
    scene through the global dense rows."""
    from orbslam2commentedbyxcm_amd import _lib as L
    if request.param is not None:
        L.debug_set("covis_lds_keyframes", request.param)
    yield request.param
    L.debug_set("covis_lds_keyframes", -1)


def random_table(rng, K, cap, n_mp):
    kf_mp = rng.integers(-1, n_mp, (K, cap)).astype(np.int32)          # duplicates within rows
    kf_mp[rng.random((K, cap)) < 0.3] = -1
    kf_mp[rng.random((K, cap)) < 0.05] = n_mp + 3                     # out of range
    kf_mp[rng.random((K, cap)) < 0.02] = -7
    kf_n = rng.integers(cap - 3, cap + 3, K).astype(np.int32)         # clamped into [0, cap]
    if K > 1:
        kf_mp[K // 2] = -1                                            # an all-NULL row
    kf_bad = (rng.random(K) < 0.15).astype(np.uint8)
    return kf_mp, kf_n, kf_bad


@pytest.mark.parametrize("cap", [63, 64, 65, 256])
@pytest.mark.parametrize("K", [1, 2, 40])
def test_observation_csr_equals_model(torch_dev, K, cap):
    rng = np.random.default_rng(100 * K + cap)
    n_mp = 3 * cap
    kf_mp, kf_n, kf_bad = random_table(rng, K, cap, n_mp)
    mp = Map(torch_dev, kf_mp, kf_n, kf_bad, np.zeros(n_mp, np.uint8))
    mp.refresh()
    st = mp.check_observations()
    if K == 40:
        assert (st["status"] & M.DUPLICATE).any() and st["obs_off"][-1] > 0
    # a second refresh of a changed table rewrites the duplicate bits and the CSR
    mp.kf_mp[:, ::2] = -1
    mp.refresh()
    mp.check_observations()
    mp.close()


def test_duplicate_lowest_index_wins_and_observer_counts(torch_dev):
    """A point with 1, 64 and 65 observers (K = 70), and a row naming a point three times."""
    K, cap = 70, 8
    kf_mp = np.full((K, cap), -1, np.int32)
    kf_mp[:64, 3] = 1      # 64 observers
    kf_mp[:65, 5] = 2      # 65
    kf_mp[69, 0] = 0       # 1
    kf_mp[10, [1, 4, 6]] = 7
    mp = Map(torch_dev, kf_mp, np.full(K, cap, np.int32), np.zeros(K, np.uint8), np.zeros(9, np.uint8))
    mp.refresh()
    st = mp.check_observations()
    assert np.diff(st["obs_off"]).tolist() == [1, 64, 65, 0, 0, 0, 0, 1, 0]
    assert st["obs_idx"][st["obs_off"][7]] == 1 and st["mp"][10].tolist() == [-1, 7, -1, 1, -1, 2, -1, -1]
    assert st["status"][10] == M.DUPLICATE and st["status"].sum() == M.DUPLICATE
    mp.close()


@pytest.mark.parametrize("name", sorted(M.GPU_SCENES))
def test_single_calls_in_insertion_order(torch_dev, lds_bound, name):
    """As LocalMapping makes them: keyframe k arrives, the observations are refreshed, k is updated."""
    mp = Map(torch_dev, *M.scene(**M.GPU_SCENES[name]))
    for k in range(mp.K):
        mp.refresh(k + 1)
        mp.update([k])
        if k % 8 == 7:
            mp.check()
    mp.check()
    mp.close()


@pytest.mark.parametrize("name", sorted(M.GPU_SCENES))
def test_batches_refresh_and_erase(torch_dev, lds_bound, name):
    mp = Map(torch_dev, *M.scene(**M.GPU_SCENES[name]))
    mp.refresh()
    mp.update(list(range(mp.K))[::-1])       # one batch of all keyframes (the bad one is skipped)
    st = mp.check()
    assert (st["status"] & M.BAD_KEYFRAME).any()
    mp.kf_mp = M.mutate(mp.kf_mp, M.GPU_SUBSET, np.random.default_rng(5))
    mp.refresh()
    mp.update(M.GPU_SUBSET)                  # a second batch of a subset on the changed map
    mp.check()
    mp.erase(0)                              # a no-op
    mp.erase(7)
    mp.check()
    mp.kf_bad[7] = 1
    mp.refresh()
    mp.update([6, 8])
    mp.check()
    # the getters
    import torch
    for N in (1, 10):
        out, out_n = mp.g.best_covisibles(N)  # asynchronous on the graph's stream
        torch.cuda.synchronize()
        out, out_n = out.cpu().numpy(), out_n.cpu().numpy()
        for k in range(mp.K):
            want = mp.m.best_covisibles(k, N)
            assert out_n[k] == len(want) and out[k, :len(want)].tolist() == want and (out[k, len(want):] == -1).all()
    for w in (1, 15, 16, 30, 1000):
        out, out_n = mp.g.covisibles_by_weight(w)
        torch.cuda.synchronize()
        out, out_n = out.cpu().numpy(), out_n.cpu().numpy()
        for k in range(mp.K):
            want = mp.m.covisibles_by_weight(k, w)
            assert out_n[k] == len(want) and out[k, :len(want)].tolist() == want
    for k in (0, 9, mp.K - 1):
        kf, w = mp.g.ordered(k)
        assert kf.tolist() == mp.m.ordered[k] and w.tolist() == mp.m.weights[k]
    mp.close()


def fan_scene(n_a=63, n_b=64):
    """Keyframe 66 is connected to n_a keyframes and keyframe 67 to n_b, with weights 15 and 16,
    and each to the other: lists of 64 and 65 entries, which cross a wave boundary.  Keyframe
    j < 65 owns the 16 points 16 j .. 16 j + 15."""
    K, cap = 70, 65 * 16
    kf_mp = np.full((K, cap), -1, np.int32)
    for j in range(65):
        kf_mp[j, :16] = np.arange(16 * j, 16 * j + 16)
    for q, n in ((66, n_a), (67, n_b)):
        row = [p for j in range(n) for p in range(16 * j, 16 * j + 15 + (j + q) % 2)]
        kf_mp[q, :len(row)] = row
    return kf_mp, np.full(K, cap, np.int32), np.zeros(K, np.uint8), np.zeros(65 * 16, np.uint8)


def test_lists_of_64_and_65_and_capacity(torch_dev, lds_bound):
    mp = Map(torch_dev, *fan_scene(), max_conn=128)
    mp.refresh()
    mp.update([66, 67])
    st = mp.check()
    assert st["ordered_n"][66] == 64 and st["ordered_n"][67] == 65
    mp.update(list(range(70)))
    mp.check()
    mp.close()
    # max_conn = 64: keyframe 67's row of 65 entries does not fit; 66's does
    mp = Map(torch_dev, *fan_scene(), max_conn=64)
    mp.refresh()
    mp.update([67, 66])
    st = mp.check()
    # 67 is left as it was (its only entry is what 66 sent it afterwards)
    assert st["status"][67] == M.CAPACITY and st["row_kf"][67, :st["row_n"][67]].tolist() == [66] and st["first"][67] == 1
    assert st["row_n"][66] == 64 and st["status"][66] == 0
    mp.close()


def test_a_message_that_overflows_a_row(torch_dev):
    a, b, c = list(range(0, 20)), list(range(100, 120)), list(range(200, 220))
    kf_mp = np.full((4, 60), -1, np.int32)
    for k, r in enumerate((a + b + c, a, b, c)):
        kf_mp[k, :len(r)] = r
    mp = Map(torch_dev, kf_mp, np.full(4, 60, np.int32), np.zeros(4, np.uint8), np.zeros(220, np.uint8), max_conn=2)
    mp.refresh()
    for k in (1, 2, 3, 0):
        mp.update([k])
        mp.check()
    st = mp.check()
    assert st["status"][0] == M.CAPACITY and st["row_n"][0] == 2 and st["ordered_kf"][0, :2].tolist() == [2, 1]
    mp.close()


def test_a_keyframe_alone_and_inside_a_batch(torch_dev):
    """Batch independence: a keyframe's own results are the same bytes alone and in a batch."""
    rows = {}
    for ids in ([9], [3, 9, 10, 11], list(range(24))):
        mp = Map(torch_dev, *M.scene(**M.GPU_SCENES["band24"]))
        mp.refresh()
        mp.update(ids)
        st = mp.check()
        n, no = st["row_n"][9], st["ordered_n"][9]
        rows[len(ids)] = (st["row_kf"][9, :n].tobytes(), st["row_w"][9, :n].tobytes(), st["ordered_kf"][9, :no].tobytes(),
                          st["ordered_w"][9, :no].tobytes(), int(st["parent"][9]), int(st["first"][9]))
        mp.close()
    assert rows[1] == rows[4] == rows[24] and rows[1][0]


# ---- LocalBundleAdjustment's graph assembly ----

TABLES = ("kf_off", "pt_off", "kf_id", "pt_id", "kf_Tcw", "kf_fixed", "kf_slot", "pt_pos", "obs_off", "obs_kf", "obs_kp",
          "counts", "status")


def assert_tables(got, want):
    g = {k: v.cpu().numpy() for k, v in got.items()}
    nk, npt = int(want["kf_off"][-1]), int(want["pt_off"][-1])
    no = int(want["obs_off"][-1])
    size = {"kf_id": nk, "kf_Tcw": nk, "kf_fixed": nk, "kf_slot": nk, "pt_id": npt, "pt_pos": npt, "obs_off": npt + 1,
            "obs_kf": no, "obs_kp": no}
    for name in TABLES:
        a = g[name][:size[name]] if name in size else g[name]
        assert a.dtype == want[name].dtype and a.tobytes() == want[name].tobytes(), name


@pytest.fixture(scope="module")
def lba(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import LocalBundleAdjuster
    o = LocalBundleAdjuster()
    yield o
    o.close()


def assembly_map(torch_dev, name):
    """A scene after a batch of all keyframes in which keyframe 5 went bad afterwards: it is
    still in its neighbours' lists."""
    kf_mp, kf_n, kf_bad, mp_bad = M.scene(**M.GPU_SCENES[name])
    kf_bad[:] = 0
    mp = Map(torch_dev, kf_mp, kf_n, kf_bad, mp_bad)
    mp.refresh()
    mp.update(list(range(mp.K)))
    mp.kf_bad[5] = 1
    mp.refresh()
    assert any(5 in o for o in mp.m.ordered)
    rng = np.random.default_rng(3)
    poses = rng.normal(size=(mp.K, 12)).astype(np.float32)
    pos = rng.normal(size=(len(mp_bad), 3)).astype(np.float32)
    return mp, poses, pos


@pytest.mark.parametrize("name", sorted(M.GPU_SCENES))
def test_assembly_equals_model(torch_dev, lba, name):
    import torch
    mp, poses, pos = assembly_map(torch_dev, name)
    K = mp.K
    d_poses, d_pos = mp.t(poses), mp.t(pos)
    # no neighbours (the last keyframe), id 0 among the locals, bad neighbours (4, 6)
    for cur in ([K - 1], [0], [4], [1, 6, K - 1, 12, 0]):
        want = M.assemble_batch(mp.m, cur, poses, pos, 10 ** 6, 10 ** 6, 10 ** 6)
        caps = (int(want["kf_off"][-1]) + 3, int(want["pt_off"][-1]) + 5, int(want["obs_off"][-1]) + 7)
        got = lba.assemble_batch_device(mp.g, cur, d_poses, d_pos, *caps)
        torch.cuda.synchronize()
        assert_tables(got, want)
        assert (want["status"] == 0).all() and want["counts"].min() > 0
    assert len(M.assemble_local_ba(mp.m, K - 1, poses, pos)["kf_id"]) == 1
    t = M.assemble_local_ba(mp.m, 1, poses, pos)
    assert 0 in t["kf_id"][1:].tolist() and t["kf_fixed"][t["kf_id"].tolist().index(0)] == 1
    # a capacity overflow in the middle problem: the problems on either side are unaffected
    cur = [1, 12, 6]
    each = [M.assemble_local_ba(mp.m, c, poses, pos) for c in cur]
    for which, caps in (("kf", (len(each[0]["kf_id"]) + len(each[2]["kf_id"]) + 1, 10 ** 5, 10 ** 5)),
                        ("pt", (10 ** 4, len(each[0]["pt_id"]) + len(each[2]["pt_id"]) + 1, 10 ** 5)),
                        ("obs", (10 ** 4, 10 ** 5, len(each[0]["obs_kf"]) + len(each[2]["obs_kf"]) + 1))):
        want = M.assemble_batch(mp.m, cur, poses, pos, *caps)
        assert want["status"].tolist() == [0, M.CAPACITY, 0], which
        got = lba.assemble_batch_device(mp.g, cur, d_poses, d_pos, *caps)
        torch.cuda.synchronize()
        assert_tables(got, want)
    # the marks are back to none: the first problem again, alone
    want = M.assemble_batch(mp.m, [1], poses, pos, 10 ** 4, 10 ** 5, 10 ** 5)
    got = lba.assemble_batch_device(mp.g, [1], d_poses, d_pos, 10 ** 4, 10 ** 5, 10 ** 5)
    torch.cuda.synchronize()
    assert_tables(got, want)
    mp.close()


def keypoints(xy, octv):
    from orbslam2commentedbyxcm_amd import _lib as L
    k = np.zeros(xy.shape[:-1], L.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = xy[..., 0], xy[..., 1], octv
    return k


def test_chain_assemble_local_ba_apply(torch_dev, lba):
    """Assemble -> local_ba_batch_device -> apply on the device against the model's assembly ->
    the host form of LocalBundleAdjustment -> the same write-back on the host: poses, positions,
    erase and the resulting kf_mp are the same bytes; UpdateConnections on the changed map
    equals the model."""
    import torch
    sc = M.geometric_scene(0)
    K, cap = sc["kf_mp"].shape
    mp = Map(torch_dev, sc["kf_mp"], sc["kf_n"], sc["kf_bad"], sc["mp_bad"])
    mp.refresh()
    mp.update(list(range(K)))
    cur = 5
    kps = keypoints(sc["xy"], sc["octave"])
    fx, fy, cx, cy, bf = sc["cam"]
    # the host chain
    t = M.assemble_local_ba(mp.m, cur, sc["poses"], sc["mp_pos"])
    assert t["kf_fixed"].sum() >= 1 and (t["kf_fixed"] == 0).sum() >= 2
    r = lba.LocalBundleAdjustment(t["kf_Tcw"], t["kf_fixed"], t["kf_slot"], t["pt_pos"], t["obs_off"], t["obs_kf"],
                                  t["obs_kp"], kps, sc["u_right"], sc["inv_sigma2"], fx, fy, cx, cy, bf)
    assert r["status"] == 0 and r["trace"][0, 0] > 0
    poses, pos, kf_mp = sc["poses"].copy(), sc["mp_pos"].copy(), sc["kf_mp"].copy()
    free = t["kf_fixed"] == 0
    poses[t["kf_id"][free]] = r["Tcw"][free]
    pos[t["pt_id"]] = r["pos"]
    pt_of = np.repeat(np.arange(len(t["pt_id"])), np.diff(t["obs_off"]))
    for o in np.flatnonzero(r["erase"]):
        assert kf_mp[t["kf_id"][t["obs_kf"][o]], t["obs_kp"][o]] == t["pt_id"][pt_of[o]]
        kf_mp[t["kf_id"][t["obs_kf"][o]], t["obs_kp"][o]] = -1
    # the device chain, with capacities in place of sizes
    d_poses, d_pos = mp.t(sc["poses"]), mp.t(sc["mp_pos"])
    d_kps = mp.t(kps.view(np.uint8).reshape(K, cap * 28)).view(K, cap, 28)
    tab = lba.assemble_batch_device(mp.g, [cur], d_poses, d_pos, len(t["kf_id"]) + 4, len(t["pt_id"]) + 9,
                                    len(t["obs_kf"]) + 11)
    s = torch.cuda.current_stream(torch_dev)
    torch.cuda.synchronize()
    out = lba.local_ba_assembled_device(tab, d_kps, mp.t(sc["u_right"]), sc["inv_sigma2"], fx, fy, cx, cy, bf, stream=s)
    torch.cuda.synchronize()
    lba.apply_batch_device(mp.g, tab, out["kf_Tcw_opt"], out["pt_pos_opt"], out["erase"], d_poses, d_pos, mp.d_kf_mp)
    torch.cuda.synchronize()
    no = len(t["obs_kf"])
    assert out["erase"].cpu().numpy()[:no].tobytes() == r["erase"].tobytes()
    assert int(out["n_erase"][0]) == r["n_erase"] and int(out["status"][0]) == 0
    assert d_poses.cpu().numpy().tobytes() == poses.tobytes()
    assert d_pos.cpu().numpy().tobytes() == pos.tobytes()
    assert mp.d_kf_mp.cpu().numpy().tobytes() == kf_mp.tobytes()
    # after apply and a refresh, UpdateConnections equals the model on the mutated map
    mp.kf_mp = kf_mp
    mp.refresh()
    mp.update([cur] + mp.m.ordered[cur])
    mp.check()
    mp.close()
