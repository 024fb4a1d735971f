"""CorrectLoop on the device (csrc/orbx_correctloop.hip) against the model
(tests/correct_loop_model.py): the same arrays go to the device graph and to the model, the chain
runs in each, and the two are compared -- integers, flags and copied bytes exactly, float outputs
within 8 x the scene's spread between the model's arithmetic variants (floor 2 float32 ulps)."""
from __future__ import annotations

import numpy as np
import pytest

import correct_loop_model as M
import covisibility_model as CM

pytestmark = pytest.mark.gpu

FLOATS = {"corr_S": "corr_S", "kf_Tcw": "poses", "mp_pos": "mp_pos", "normal": "normal", "max_distance": "max_distance",
          "min_distance": "min_distance"}
MAP_INTS = ("mp_corrected_by_kf", "mp_corrected_ref")


@pytest.fixture(scope="module")
def model(orbx_built):
    """Every scene once in the model, with its spread: shared by the tests, never changed."""
    out = {}
    for name in M.SCENES:
        sc, st, asm, g, g_after = M.run(name)
        out[name] = dict(sc=sc, st=st, asm=asm, g=g, g_after=g_after, spread=M.spread(name))
    return out


@pytest.fixture(params=[None, 8], ids=["lds", "global"])
def lds_bound(request, orbx_built):
    """Both histogram paths of the row kernels."""
    from orbslam2commentedbyxcm_amd import _lib as L
    if request.param is not None:
        L.debug_set("covis_lds_keyframes", request.param)
    yield request.param
    L.debug_set("covis_lds_keyframes", -1)


class Dev:
    """A scene in HBM with the device graph after UpdateConnections of every keyframe."""

    def __init__(self, name, io=None, decoy=None):
        """io: a stream_order I/O object for the state's uploads (default: blocking ones); decoy:
        the state (decoy_state) that is in place until an ordered run's real uploads.  The map
        tables, which the graph is built from here, are the real ones either way."""
        import torch

        from orbslam2commentedbyxcm_amd import CovisibilityGraph, LoopCorrector
        from orbslam2commentedbyxcm_amd import _lib as L
        self.sc, self.st0 = sc, st = M.scene(name)
        K, cap = sc["kf_mp"].shape
        self.g = CovisibilityGraph(K, cap, len(sc["mp_bad"]), sc["max_conn"])
        self.dev = dev = torch.device("cuda", 0)
        self.t = t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        keys = np.zeros((K, cap), L.KEYPOINT_DTYPE)
        keys["octave"] = st["octave"]
        self.kf_mp, self.kf_n, self.kf_bad, self.mp_bad = t(sc["kf_mp"]), t(sc["kf_n"]), t(sc["kf_bad"]), t(sc["mp_bad"])
        ds = st if decoy is None else decoy
        up = (lambda k: t(st[k])) if io is None else (lambda k: io.up(st[k], ds[k]))
        self.d = {"kf_Tcw": up("poses"), "mp_pos": up("mp_pos"), "mp_corrected_by_kf": t(st["mp_corrected_by_kf"]),
                  "mp_corrected_ref": t(st["mp_corrected_ref"]), "mp_ref_kf": t(st["mp_ref_kf"]),
                  "kf_keys_un": t(keys.view(np.uint8).reshape(K, cap, 28)), "normal": up("normal"),
                  "max_distance": up("max_distance"), "min_distance": up("min_distance")}
        torch.cuda.synchronize()
        self.refresh()
        self.g.update_connections(list(range(K)))
        self.lc = LoopCorrector(self.g, self.d, st["scale"])
        off = np.zeros(K + 1, np.int32)
        ids = []
        for k in range(K):
            ids += sc["loop_edges"].get(k, [])
            off[k + 1] = len(ids)
        self.loop_off, self.loop_ids = t(off), t(np.array(ids + [0], np.int32))

    def refresh(self):
        self.g.refresh_observations(self.kf_mp, self.kf_n, self.kf_bad, self.mp_bad)

    def propagate(self, **kw):
        import torch
        if not kw:
            kw = dict(Scw=self.t(self.sc["Scw"]))
        self.lc.propagate(self.sc["cur"], **kw)
        torch.cuda.synchronize()
        got = self.lc.state()
        got.update({k: v.cpu().numpy() for k, v in self.d.items()})
        return got

    def fuse(self):
        """The caller's seam: a host edit of kf_mp, then a refresh."""
        import torch
        torch.cuda.synchronize()
        self.kf_mp.copy_(self.t(self.sc["kf_mp_fused"]))
        torch.cuda.synchronize()
        self.refresh()

    def assemble(self, **kw):
        import torch
        self.lc.assemble(self.sc["loop"], self.loop_off, self.loop_ids, self.sc["min_feat"], **kw)
        torch.cuda.synchronize()
        return self.lc.state()


STATE_PAYLOAD = ("poses", "mp_pos", "normal", "max_distance", "min_distance")
CHAIN_KEYS = ("conn", "n_conn", "corr_S", "kf_corr", "kf_Tcw_nc", "propagate_status", "kf_Tcw", "mp_pos", "normal",
              "max_distance", "min_distance", "mp_corrected_by_kf", "mp_corrected_ref", "kf_ids", "n_rows", "edge_v",
              "edge_kind", "n_edges", "pt_ref", "assemble_status", "kf_Tcw_opt", "pt_pos_opt", "Scw_opt", "trace", "chi2",
              "status", "nd_status")


def decoy_state(name):
    """(state, Scw) of the scene with the same ids, octaves and reference keyframes; poses,
    positions, normals, distances and the corrected Sim3 moved."""
    sc, st = M.scene(name)
    d = dict(st)
    d["poses"] = np.array(st["poses"], np.float32, copy=True)
    d["poses"][:, [3, 7, 11]] += np.float32([0.03, -0.02, 0.01])
    d["mp_pos"] = (st["mp_pos"] + np.float32([0.02, 0.03, -0.01])).astype(np.float32)
    d["normal"] = np.ascontiguousarray(st["normal"][:, ::-1]) + np.float32(0.125)
    d["max_distance"] = (st["max_distance"] * np.float32(1.25) + np.float32(0.5)).astype(np.float32)
    d["min_distance"] = (st["min_distance"] * np.float32(0.75) + np.float32(0.25)).astype(np.float32)
    Scw = np.array(sc["Scw"], np.float64, copy=True)
    Scw[4:7] += [0.05, -0.02, 0.03]
    return d, Scw


def run_chain(name, opt, io=None, decoy=False, decoy_only=False, env_blocks=None):
    """The CorrectLoop chain on one stream with nothing read back: propagate -> refresh (on the
    fused map) -> essential-graph assembly -> OptimizeEssentialGraph -> UpdateNormalAndDepth of
    every point at the optimised positions.  A fresh graph per run (propagation changes it).
    io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    calls); decoy: the decoy state is in place before an ordered run's real uploads; decoy_only:
    run on the decoy state.  env_blocks None: read back after the assembly (a synchronisation)."""
    import stream_order as SO
    sc, st = M.scene(name)
    dst, dScw = decoy_state(name)
    d = Dev(name, io=io, decoy=dst if decoy else None) if not decoy_only else None
    if decoy_only:
        d = Dev(name)
        for k_dev, k_st in (("kf_Tcw", "poses"), ("mp_pos", "mp_pos"), ("normal", "normal"),
                            ("max_distance", "max_distance"), ("min_distance", "min_distance")):
            d.d[k_dev].copy_(d.t(dst[k_st]))
    io = io or SO.SyncIO(d.dev)
    Scw = np.asarray(sc["Scw"], np.float64)
    d_Scw = io.up(dScw if decoy_only else Scw, dScw if decoy else None)
    d_fused = io.up(sc["kf_mp_fused"])
    io.begin()
    with io.on_stream():
        p = d.lc.propagate(sc["cur"], Scw=d_Scw, stream=io.stream)
        io.end()
        d.g.refresh_observations(d_fused, d.kf_n, d.kf_bad, d.mp_bad, stream=io.stream)
        io.end()
        a = d.lc.assemble(sc["loop"], d.loop_off, d.loop_ids, sc["min_feat"], stream=io.stream)
        io.end()
        if env_blocks is None:
            env_blocks = max(1, int(a["env_blocks"].cpu()[0]))
        o = d.lc.optimize(opt, fix_scale=False, max_env_blocks=env_blocks, stream=io.stream)
        io.end()
        nd = d.lc.update_normal_and_depth(stream=io.stream, tables={"mp_pos": o["pt_pos_opt"]})
        io.end()
    got = {k: io.down(p[k]) for k in ("conn", "n_conn", "corr_S", "kf_corr", "kf_Tcw_nc")}
    got["propagate_status"] = io.down(p["status"])
    got.update({k: io.down(d.d[k]) for k in ("kf_Tcw", "mp_pos", "normal", "max_distance", "min_distance",
                                            "mp_corrected_by_kf", "mp_corrected_ref")})
    got.update({k: io.down(a[k]) for k in ("kf_ids", "n_rows", "edge_v", "edge_kind", "n_edges", "pt_ref")})
    got["assemble_status"] = io.down(a["status"])
    got.update({k: io.down(o[k]) for k in ("kf_Tcw_opt", "pt_pos_opt", "Scw_opt", "trace", "chi2", "status")})
    got["nd_status"] = io.down(nd)
    got["env_blocks"] = env_blocks
    got["dev"] = d                                    # the graph lives until the caller has synchronised
    return got


def test_run_chain_equals_the_model_up_to_the_assembly(model):
    """The runner of the stream-order tests: its propagation and assembly against the model."""
    from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer
    opt = EssentialGraphOptimizer()
    got = run_chain("hand", opt)
    m = model["hand"]
    asm = m["asm"]
    nr = len(asm["kf_ids"])
    assert int(got["n_rows"][0]) == nr and np.array_equal(got["kf_ids"][:nr], asm["kf_ids"])
    ne = len(asm["edge_v"])
    assert int(got["n_edges"][0]) == ne and np.array_equal(got["edge_v"][:ne], asm["edge_v"])
    assert np.array_equal(got["edge_kind"][:ne], asm["edge_kind"]) and np.array_equal(got["pt_ref"], asm["pt_ref"])
    assert got["trace"][0, 0] > 0
    got["dev"].g.close()
    opt.close()


def close(got, want, spread):
    want = np.asarray(want)
    d = np.abs(np.asarray(got, np.float64) - want.astype(np.float64))
    tol = M.tolerance(spread, want)
    assert np.all(d <= tol), (float(d.max()), float(tol.flat[np.argmax(d - tol)]))


def check_propagation(got, m):
    st, n = m["st"], len(m["st"]["conn"])
    assert int(got["n_conn"][0]) == n and got["conn"][:n].tolist() == st["conn"].tolist()
    assert np.array_equal(got["kf_corr"], st["kf_corr"])
    for k in MAP_INTS:
        assert np.array_equal(got[k], st[k]), k
    assert int(got["status"][0]) == st["status"]
    assert got["kf_Tcw_nc"][:n].tobytes() == st["kf_Tcw_nc"].tobytes()  # a copy of the input poses
    for dk, mk in FLOATS.items():
        g = got[dk][:n] if dk == "corr_S" else got[dk]
        close(g, st[mk], m["spread"][mk])


def check_assembly(got, asm):
    n, nr, ne = len(asm["lc_member"]), len(asm["kf_ids"]), len(asm["edge_v"])
    assert got["lc_member"][:n].tolist() == asm["lc_member"].tolist()
    assert got["lc_off"][:n + 1].tolist() == asm["lc_off"].tolist()
    nl = int(asm["lc_off"][-1])
    assert got["lc_kf"][:nl].tolist() == asm["lc_kf"].tolist() and got["lc_w"][:nl].tolist() == asm["lc_w"].tolist()
    assert int(got["n_rows"][0]) == nr and got["kf_off"].tolist() == [0, nr]
    assert got["kf_ids"][:nr].tolist() == asm["kf_ids"].tolist() and np.array_equal(got["kf_row"], asm["kf_row"])
    assert int(got["loop_row"][0]) == asm["loop_row"]
    assert got["kf_corr_rows"][:nr].tolist() == asm["kf_corr_rows"].tolist()
    assert int(got["n_edges"][0]) == ne and got["edge_off"].tolist() == [0, ne]
    assert got["edge_v"][:ne].tolist() == asm["edge_v"].tolist(), "essential_graph_edges"
    assert got["edge_kind"][:ne].tolist() == asm["edge_kind"].tolist()
    assert np.array_equal(got["pt_ref"], asm["pt_ref"]) and got["pt_off"].tolist() == [0, len(asm["pt_ref"])]
    assert int(got["env_blocks"][0]) == asm["env_blocks"], "orbx_essential_graph_envelope"
    assert int(got["status"][0]) == 0


@pytest.mark.parametrize("name", M.SCENES)
def test_propagate_and_assemble_equal_the_model(model, lds_bound, name):
    m = model[name]
    d = Dev(name)
    got = d.propagate()
    check_propagation(got, m)
    CM.assert_same_state(m["g_after"], d.g.state())
    d.fuse()
    got = d.assemble(max_edges=len(m["asm"]["edge_v"]), max_lc=int(m["asm"]["lc_off"][-1]))
    check_assembly(got, m["asm"])
    nr = len(m["asm"]["kf_ids"])
    assert got["kf_Tcw_rows"][:nr].tobytes() == np.array(
        [got["kf_Tcw_nc"][got["kf_corr"][k]] if got["kf_corr"][k] >= 0 else d.d["kf_Tcw"].cpu().numpy()[k]
         for k in m["asm"]["kf_ids"]], np.float32).tobytes()
    st = d.g.state()
    CM.assert_same_state(m["g"], st)
    assert np.array_equal(st["mp"], m["g"].clean)


def run_bytes(name):
    d = Dev(name)
    a = d.propagate()
    d.fuse()
    b = d.assemble()
    st = d.g.state()
    return {**{"p_" + k: v.tobytes() for k, v in a.items()}, **{"a_" + k: v.tobytes() for k, v in b.items()},
            **{"g_" + k: v.tobytes() for k, v in st.items()}}


@pytest.mark.parametrize("name", ["hand", "band24"])
def test_histogram_paths_and_a_second_run_give_the_same_bytes(orbx_built, name):
    from orbslam2commentedbyxcm_amd import _lib as L
    first = run_bytes(name)
    assert run_bytes(name) == first  # determinism
    L.debug_set("covis_lds_keyframes", 8)
    try:
        other = run_bytes(name)
    finally:
        L.debug_set("covis_lds_keyframes", -1)
    assert other.keys() == first.keys()
    for k in first:
        assert other[k] == first[k], k


def test_edge_and_loop_connection_capacity(model):
    m = model["hand"]
    asm = m["asm"]
    need, need_lc, K = len(asm["edge_v"]), int(asm["lc_off"][-1]), len(m["sc"]["kf_n"])
    d = Dev("hand")
    d.propagate()
    d.fuse()
    t = d.lc.assembly_tables(K, max_edges=need - 1)
    t["edge_v"].fill_(-7)  # the guard element sits behind the capacity
    t["edge_kind"].fill_(-7)
    got = d.assemble(max_edges=need - 1)
    assert int(got["status"][0]) == M.ASM_CAPACITY
    assert int(got["n_edges"][0]) == need and got["edge_off"].tolist() == [0, need - 1]
    assert got["edge_v"][:need - 1].tolist() == asm["edge_v"][:need - 1].tolist()
    assert got["edge_v"][need - 1].tolist() == [-7, -7] and int(got["edge_kind"][need - 1]) == -7
    # the LoopConnections one short: CAPACITY, the need in lc_off, nothing past the capacity, no edges
    d = Dev("hand")
    d.propagate()
    d.fuse()
    t = d.lc.assembly_tables(K, max_lc=need_lc - 1)
    t["lc_kf"].fill_(-7)
    got = d.assemble(max_lc=need_lc - 1)
    assert int(got["status"][0]) & M.ASM_CAPACITY
    assert int(got["lc_off"][len(asm["lc_member"])]) == need_lc and int(got["lc_kf"][need_lc - 1]) == -7
    assert int(got["n_edges"][0]) == 0 and got["edge_off"].tolist() == [0, 0]


def test_composed_scw_equals_the_given_form(model):
    """LoopClosing.cc:359-362 on the device: Sim3(R, t, s) * Sim3(Rmw, tmw, 1) from OptimizeSim3's
    float outputs.  The composed estimate is the model's within tolerance, and feeding it back as
    the given form gives every output's bytes again."""
    sc, st0 = M.scene("geo10")
    rng = np.random.default_rng(2)
    R = (M._rot(rng, 5.0)).astype(np.float32)
    tt = rng.normal(0, 0.3, 3).astype(np.float32)
    s = np.array([1.03], np.float32)
    d = Dev("geo10")
    a = d.propagate(sim3=(d.t(R.reshape(-1)), d.t(tt), d.t(s)), matched_kf=sc["loop"])
    n = int(a["n_conn"][0])
    want = M.compose_scw(R, tt, s[0], st0["poses"][sc["loop"]])
    got = a["corr_S"][n - 1]  # cur is the last member: its CorrectedSim3 is Scw itself
    assert np.all(np.abs(got - want) <= M.tolerance(0.0, want)), (got, want)
    d2 = Dev("geo10")
    b = d2.propagate(Scw=d2.t(got.copy()))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_argument_errors_with_a_graph(orbx_built):
    """An id outside the graph and a call before a refresh are ORBX_ERR_ARG."""
    import torch

    from orbslam2commentedbyxcm_amd import CovisibilityGraph, LoopCorrector, OrbxError
    from orbslam2commentedbyxcm_amd import _lib as L
    d = Dev("geo10")
    K = len(d.sc["kf_n"])
    for kw in (dict(cur_kf=K), dict(cur_kf=-1)):
        with pytest.raises(OrbxError) as e:
            d.lc.propagate(kw["cur_kf"], Scw=d.t(d.sc["Scw"]))
        assert e.value.code == L.ORBX_ERR_ARG
    with pytest.raises(OrbxError) as e:
        d.lc.propagate(d.sc["cur"], sim3=(d.t(np.eye(3, dtype=np.float32)), d.t(np.zeros(3, np.float32)), d.t(np.ones(1, np.float32))),
                       matched_kf=K + 3)
    assert e.value.code == L.ORBX_ERR_ARG
    d.propagate()
    with pytest.raises(OrbxError) as e:
        d.lc.assemble(K, d.loop_off, d.loop_ids)
    assert e.value.code == L.ORBX_ERR_ARG
    g = CovisibilityGraph(K, d.sc["kf_mp"].shape[1], len(d.sc["mp_bad"]), 16)  # never refreshed
    torch.cuda.synchronize()
    fresh = LoopCorrector(g, d.d, d.st0["scale"])
    for call in (lambda: fresh.propagate(d.sc["cur"], Scw=d.t(d.sc["Scw"])), lambda: fresh.update_normal_and_depth()):
        with pytest.raises(OrbxError) as e:
            call()
        assert e.value.code == L.ORBX_ERR_ARG and "refresh" in str(e.value)


def test_update_normal_and_depth_ids_and_status(model):
    m = model["hand"]
    d = Dev("hand")
    import torch
    st = dict(d.st0)
    g = M.graph_of(d.sc)
    n = len(d.sc["mp_bad"])
    ids = np.array([5, 700, 3, n + 4, -1, 900], np.int32)
    want = M.update_normal_and_depth(g, st, ids)
    status = d.lc.update_normal_and_depth(d.t(ids))
    torch.cuda.synchronize()
    sp = m["spread"]
    assert int(status.cpu()[0]) == want[3] and want[3] & M.BAD_INDEX
    close(d.d["normal"].cpu().numpy(), want[0], sp["normal"])
    close(d.d["max_distance"].cpu().numpy(), want[1], sp["max_distance"])
    close(d.d["min_distance"].cpu().numpy(), want[2], sp["min_distance"])
    untouched = np.setdiff1d(np.arange(n), ids[(ids >= 0) & (ids < n)])
    assert not d.d["normal"].cpu().numpy()[untouched].any()  # only the listed points are written
    want = M.update_normal_and_depth(g, st)
    status = d.lc.update_normal_and_depth()
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == want[3] and want[3] & M.REF_NOT_OBSERVER
    close(d.d["normal"].cpu().numpy(), want[0], sp["normal"])
    close(d.d["max_distance"].cpu().numpy(), want[1], sp["max_distance"])
    close(d.d["min_distance"].cpu().numpy(), want[2], sp["min_distance"])
    bad = np.flatnonzero(d.sc["mp_bad"])
    assert not d.d["normal"].cpu().numpy()[bad].any() and not d.d["max_distance"].cpu().numpy()[bad].any()


@pytest.mark.parametrize("name", ["hand", "band24"])
def test_chain_equals_the_host_form(model, name):
    """propagate -> a host edit of kf_mp (the hand scene's fused table; for band24 the model's fuse()
    followed by covisibility_model.mutate) -> refresh -> assemble -> essential_graph_batch_device gives
    the bytes of the host form OptimizeEssentialGraph fed with the host-assembled tables from the
    same corr_S; then UpdateNormalAndDepth over all points equals the model on the optimised state."""
    import torch

    from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer
    m = model[name]
    asm = m["asm"]
    d = Dev(name)
    p = d.propagate()
    d.fuse()
    d.assemble(max_edges=len(asm["edge_v"]) + 5)
    opt = EssentialGraphOptimizer()
    try:
        o = d.lc.optimize(opt, fix_scale=False)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items() if hasattr(v, "cpu")}
        n = int(p["n_conn"][0])
        nr = len(asm["kf_ids"])
        Tnc = np.array([p["kf_Tcw_nc"][p["kf_corr"][k]] if p["kf_corr"][k] >= 0 else p["kf_Tcw"][k] for k in asm["kf_ids"]],
                       np.float32)
        host = opt.OptimizeEssentialGraph(Tnc, asm["kf_corr_rows"], p["corr_S"][:n], asm["loop_row"], asm["edge_v"],
                                          asm["edge_kind"], p["mp_pos"], asm["pt_ref"], fix_scale=False)
    finally:
        opt.close()
    assert got["kf_Tcw_opt"][:nr].tobytes() == host["Tcw"].tobytes()
    assert got["pt_pos_opt"].tobytes() == host["pos"].tobytes()
    assert got["trace"].reshape(-1).tolist() == host["trace"].tolist() and int(got["status"][0]) == host["status"]
    assert host["trace"][0] > 0
    # a bad point has pt_ref = -1: the optimiser leaves its bytes alone and reports BAD_INDEX
    bad = np.flatnonzero(m["sc"]["mp_bad"])
    assert len(bad) and np.all(asm["pt_ref"][bad] == -1)
    assert got["pt_pos_opt"][bad].tobytes() == p["mp_pos"][bad].tobytes()
    assert int(got["status"][0]) & 4  # ORBX_ESSENTIAL_GRAPH_STATUS_BAD_INDEX
    moved = np.flatnonzero(asm["pt_ref"] >= 0)
    assert (got["pt_pos_opt"][moved] != p["mp_pos"][moved]).any()
    # cc:1148 on the optimised state: poses of the rows' keyframes, every position
    poses = p["kf_Tcw"].copy()
    poses[asm["kf_ids"]] = host["Tcw"]
    st = dict(m["st"], poses=poses, mp_pos=host["pos"], normal=p["normal"], max_distance=p["max_distance"],
              min_distance=p["min_distance"])
    want = M.update_normal_and_depth(m["g"], st)
    d.d["kf_Tcw"].copy_(d.t(poses))
    d.d["mp_pos"].copy_(o["pt_pos_opt"])
    torch.cuda.synchronize()
    status = d.lc.update_normal_and_depth()
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == want[3]
    sp = m["spread"]
    close(d.d["normal"].cpu().numpy(), want[0], sp["normal"])
    close(d.d["max_distance"].cpu().numpy(), want[1], sp["max_distance"])
    close(d.d["min_distance"].cpu().numpy(), want[2], sp["min_distance"])
