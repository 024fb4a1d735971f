"""The asynchronous stream contract of the device entry points (include/orbx.h: "Asynchronous on
`stream` (or the handle's)", "may be reused on return", "successive calls on one matcher must
use one stream", "a call on another stream first waits for the last one").

Every test first runs its calls the way the parity tests do (blocking uploads, a device
synchronise around the call) and times them, then runs them again on the same handle behind a
hold on one stream (tests/stream_order.py): decoy inputs in place, the real inputs, the
call(s) and the downloads queued behind the hold, only that stream synchronised.  Every
output must equal the synchronous run byte for byte, and every call must have returned while
the hold was still running.  Before a module's tests its liveness probe shows that a call on
the wrong stream does give other bytes on the held stream that the tests then use.

Scenes: the smallest of the parity tests that take every launch path (their names are the
models').  The synchronous runs are compared with the models in the parity tests' own files.
"""
from __future__ import annotations

import numpy as np
import pytest

import covisibility_model as CM
import essential_graph_model as EM
import global_ba_model as GM
import kfdb_model as KM
import local_ba_model as LM
import optimize_sim3_model as SM
import pose_opt_model as PM
import stream_order as SO
import test_gpu_correct_loop as CL
import test_gpu_covisibility as CV
import test_gpu_culling as CU
import test_gpu_essential_graph as EG
import test_gpu_global_ba as GB
import test_gpu_kfdb as KF
import test_gpu_local_ba as LB
import test_gpu_local_map as TL
import test_gpu_match as MT
import test_gpu_optimize_sim3 as S3
import test_gpu_pose_opt as PO
import test_gpu_posed as PD
import test_gpu_triangulate as TR
import triangulate_model as TM

pytestmark = pytest.mark.gpu

PO_SCENES = ("mono-9", "mixed-257")
LB_SCENES = ("mixed", "edges-65")
PO_KEYS = ("Tcw", "outlier", "ninliers", "ninit", "trace", "mp")
LB_KEYS = ("Tcw", "pos", "erase", "level1", "n_erase", "status", "trace")
PO_PAYLOAD = {"kps", "ur", "tcw", "pos"}
LB_PAYLOAD = {"Tcw", "pos", "kps_xy", "u_right", "kps"}
GB_SCENES = ("mixed-out10", "banded-64")
GB_KEYS = ("Tcw", "pos", "pt_included", "status", "trace", "chi2")
S3_SCENES = ("n10-out1-free", "n65-fix")
S3_KEYS = ("R12", "t12", "s12", "m12", "ninliers", "ncorr", "nbad", "trace")
S3_PAYLOAD = {"kps1", "kps2", "pos", "Tcw1", "Tcw2", "R12", "t12", "s12"}
EG_SCENES = ("ring-9", "ring-65")
EG_PAYLOAD = {"Tcw", "corr_S", "pos"}
TR_SCENES = ("n65", "n257")
TR_KEYS = TR.NAMES
CV_SCENE = "band24"
CV_IDS = list(range(0, 24, 2))     # the even keyframes are updated; the decoy ids are the odd ones
CV_ERASE = 8
CHAIN_FLOOR_MS = 300.0    # several calls and their host work behind one hold


# ---- the cases and their decoys (tests/test_stream_order_decoys.py checks the decoy rule) --------
def po_case(names):
    scenes = [PM.scene(n) for n in names]
    return scenes, [SO.decoy_pose_opt(s) for s in scenes]


def lb_case(names):
    scenes = [LM.scene(n) for n in names]
    return scenes, [SO.decoy_local_ba(s) for s in scenes]


def gb_case(names):
    scenes = [GM.scene(n) for n in names]
    return scenes, [SO.decoy_local_ba(s) for s in scenes]


def s3_case(names):
    scenes = [SM.scene(n) for n in names]
    return scenes, [SO.decoy_optimize_sim3(s) for s in scenes]


def eg_case(names):
    scenes = [EM.scene(n) for n in names]
    return scenes, [SO.decoy_essential_graph(s) for s in scenes]


def cv_case():
    tables = CM.scene(**CM.GPU_SCENES[CV_SCENE])
    return tables, SO.decoy_covisibility(*tables)


def cv_decoy_ids(ids):
    """Other valid, distinct keyframe ids of the same count."""
    return np.asarray([(int(k) + 1) % 24 for k in ids], np.int32)


def kf_case():
    rng = np.random.default_rng(265)
    bows = [KM.random_bow(rng, (1, 300, 64, 65)[i] if i < 4 else int(rng.integers(1, 301))) for i in range(65)]
    query = KM.random_bow(rng, 150)
    reloc = [KM.perturbed(rng, bows[7], 0.7, 20), KM.random_bow(rng, 200)]
    ids = [int(i) for i in rng.permutation(65)]
    return dict(bows=bows, query=query, reloc=reloc, ids=ids, decoy_bows=SO.decoy_bows(bows),
                decoy_query=SO.decoy_bows([query], 79)[0], decoy_reloc=SO.decoy_bows(reloc, 80))


# ---- runners: run(io, decoy_only) -> outputs ----------------------------------------------------
def po_runner(opt, names):
    scenes, decoys = po_case(names)

    def run(io, decoy_only=False):
        return PO.run_batch(opt, decoys, io=io) if decoy_only else PO.run_batch(opt, scenes, io=io, decoy=decoys)
    return run


def lb_runner(opt, names):
    scenes, decoys = lb_case(names)

    def run(io, decoy_only=False):
        return LB.run_batch(opt, decoys, io=io) if decoy_only else LB.run_batch(opt, scenes, io=io, decoy=decoys)
    return run


def gb_runner(opt, name):
    scenes, decoys = gb_case([name])
    kw = GM.params(name)

    def run(io, decoy_only=False):
        if decoy_only:
            return GB.run_batch(opt, decoys, io=io, **kw)
        return GB.run_batch(opt, scenes, io=io, decoy=decoys, **kw)
    return run


def s3_runner(opt, names):
    scenes, decoys = s3_case(names)

    def run(io, decoy_only=False):
        return S3.run_batch(opt, decoys, io=io) if decoy_only else S3.run_batch(opt, scenes, io=io, decoy=decoys)
    return run


def eg_runner(opt, name):
    scenes, decoys = eg_case([name])
    k = EM.exact_iterations(name)

    def run(io, decoy_only=False):
        out = EG.run_batch(opt, decoys, iterations=k, io=io) if decoy_only else \
            EG.run_batch(opt, scenes, iterations=k, io=io, decoy=decoys)
        got = dict(out[0])
        got["status"] = np.asarray(got["status"], np.int32).reshape(1)       # a view of an ordered run's buffer
        return got
    return run


EG_KEYS = ("Tcw", "pos", "Scw", "status", "trace", "chi2")


def tr_runner(tri, name):
    sc = TM.scene(name)

    def run(io, decoy_only=False):
        if decoy_only:
            return TR.run_batch(tri, sc, io=io, packed=TR.decoy_pack(TM.pack(sc)))
        return TR.run_batch(tri, sc, io=io, decoy=True)
    return run


def cv_runner(g, ids=CV_IDS, erase=CV_ERASE):
    tables, decoys = cv_case()

    def run(io, decoy_only=False):
        if decoy_only:
            return CV.run_graph(g, decoys, ids, io=io, erase=erase)
        return CV.run_graph(g, tables, ids, io=io, decoy=decoys, erase=erase, decoy_ids=cv_decoy_ids(ids))
    return run


def ordered_equals_sync(dev, run, keys, what, stream, floor_ms=SO.HOLD_MIN_MS, clobber=False):
    """The synchronous run, then the ordered run on the same handle: the same bytes, and no
    call waited for the hold."""
    sio = SO.SyncIO(dev)
    want = run(sio)
    io = SO.OrderedIO(dev, sio.call_ms, what, stream=stream, floor_ms=floor_ms, clobber=clobber)
    got = run(io)
    io.finish()
    SO.same_bytes(got, want, what, keys)
    return want, got


@pytest.fixture(scope="module")
def dev(orbx_built):
    import torch
    return torch.device("cuda", 0)


# ---- PoseOptimization -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def po(dev):
    from orbslam2commentedbyxcm_amd.optimizer import PoseOptimizer
    o = PoseOptimizer()
    stream, _, _ = SO.probe(dev, po_runner(o, PO_SCENES[1:]), PO_KEYS, "PoseOptimization")
    yield o, stream
    o.close()


@pytest.mark.parametrize("name", PO_SCENES)
def test_pose_optimization_behind_a_hold(dev, po, name):
    opt, stream = po
    want, _ = ordered_equals_sync(dev, po_runner(opt, [name]), PO_KEYS, f"pose_optimization_batch_device {name}", stream)
    sc, r = PO.assert_guard(name)
    PO.assert_frame(want, 0, sc, r, name)


def test_pose_optimization_level_table_may_be_reused_on_return(dev, po):
    opt, stream = po
    ordered_equals_sync(dev, po_runner(opt, PO_SCENES), PO_KEYS, "pose_optimization inv_level_sigma2 reuse", stream,
                        clobber=True)


# ---- LocalBundleAdjustment ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lb(dev):
    from orbslam2commentedbyxcm_amd.optimizer import LocalBundleAdjuster
    o = LocalBundleAdjuster()
    stream, _, _ = SO.probe(dev, lb_runner(o, LB_SCENES[:1]), LB_KEYS, "LocalBundleAdjustment")
    yield o, stream
    o.close()


@pytest.mark.parametrize("name", LB_SCENES)
def test_local_ba_behind_a_hold(dev, lb, name):
    opt, stream = lb
    want, _ = ordered_equals_sync(dev, lb_runner(opt, [name]), LB_KEYS, f"local_bundle_adjustment_batch_device {name}",
                                  stream)
    sc, r = LB.assert_guard(name)
    LB.assert_problem(LB.part(want, 0), sc, r, name)


def test_local_ba_level_table_may_be_reused_on_return(dev, lb):
    opt, stream = lb
    ordered_equals_sync(dev, lb_runner(opt, LB_SCENES), LB_KEYS, "local_ba inv_sigma2 reuse", stream, clobber=True)


# ---- GlobalBundleAdjustment, OptimizeSim3, the essential graph, triangulate_pairs --------------------
@pytest.fixture(scope="module")
def gb(dev):
    from orbslam2commentedbyxcm_amd.optimizer import GlobalBundleAdjuster
    o = GlobalBundleAdjuster()
    stream, _, _ = SO.probe(dev, gb_runner(o, GB_SCENES[0]), GB_KEYS, "GlobalBundleAdjustment")
    yield o, stream
    o.close()


@pytest.mark.parametrize("name", GB_SCENES)
def test_global_ba_behind_a_hold(dev, gb, name):
    opt, stream = gb
    want, _ = ordered_equals_sync(dev, gb_runner(opt, name), GB_KEYS, f"global_bundle_adjustment_batch_device {name}",
                                  stream, clobber=True)
    sc, r, sp = GB.assert_guard(name)
    GB.assert_problem(GB.part(want, 0), r, sp, name)


@pytest.fixture(scope="module")
def s3(dev):
    from orbslam2commentedbyxcm_amd.optimizer import Sim3Optimizer
    o = Sim3Optimizer()
    stream, _, _ = SO.probe(dev, s3_runner(o, S3_SCENES[1:]), [k for k in S3_KEYS if k != "m12"], "OptimizeSim3")
    yield o, stream
    o.close()


@pytest.mark.parametrize("name", S3_SCENES)
def test_optimize_sim3_behind_a_hold(dev, s3, name):
    """The level tables and K1 / K2 are overwritten on return."""
    opt, stream = s3
    want, _ = ordered_equals_sync(dev, s3_runner(opt, [name]), S3_KEYS, f"optimize_sim3_batch_device {name}", stream,
                                  clobber=True)
    sc, r = S3.assert_guard(name)
    S3.assert_candidate(want, 0, sc, r, name)


@pytest.fixture(scope="module")
def eg(dev):
    from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer
    o = EssentialGraphOptimizer()
    stream, _, _ = SO.probe(dev, eg_runner(o, EG_SCENES[0]), EG_KEYS, "OptimizeEssentialGraph")
    yield o, stream
    o.close()


@pytest.mark.parametrize("name", EG_SCENES)
def test_essential_graph_behind_a_hold(dev, eg, name):
    opt, stream = eg
    want, _ = ordered_equals_sync(dev, eg_runner(opt, name), EG_KEYS, f"optimize_essential_graph_batch_device {name}",
                                  stream)
    r = EG.model(name, EM.exact_iterations(name))
    assert np.array_equal(want["trace"], r["trace"]) and int(want["status"][0]) == r["status"]
    EG.assert_close(want, r, "k", name)


def test_correct_loop_chain_behind_a_hold(dev, eg):
    """correct_loop_propagate_device -> refresh_observations -> essential_graph_assemble_device ->
    optimize_essential_graph_batch_device -> update_normal_and_depth_device behind one hold, on the
    held stream the essential graph's probe kept (the chain's two handles have streams of their
    own, which are not ordered with each other, so the chain itself cannot be probed)."""
    opt, stream = eg
    sio = SO.SyncIO(dev)
    want = CL.run_chain("hand", opt, io=sio)
    decoy = CL.run_chain("hand", opt, decoy_only=True)
    assert SO.differs(want, decoy, ("corr_S", "kf_Tcw_opt", "pt_pos_opt", "normal"))
    io = SO.OrderedIO(dev, sio.call_ms, "CorrectLoop chain", stream=stream, floor_ms=CHAIN_FLOOR_MS)
    got = CL.run_chain("hand", opt, io=io, decoy=True, env_blocks=want["env_blocks"])
    io.finish()
    SO.same_bytes(got, want, "CorrectLoop chain", CL.CHAIN_KEYS)
    assert want["trace"][0, 0] > 0 and int(want["n_edges"][0]) > 0
    for r in (want, decoy, got):
        r["dev"].g.close()


@pytest.fixture(scope="module")
def tr(dev):
    from orbslam2commentedbyxcm_amd.mapping import Triangulator
    t = Triangulator()
    stream, _, _ = SO.probe(dev, tr_runner(t, TR_SCENES[0]), TR_KEYS, "triangulate_pairs")
    yield t, stream
    t.close()


@pytest.mark.parametrize("name", TR_SCENES)
def test_triangulate_pairs_behind_a_hold(dev, tr, name):
    """The host pair table is overwritten on return."""
    tri, stream = tr
    want, _ = ordered_equals_sync(dev, tr_runner(tri, name), TR_KEYS, f"triangulate_pairs_batch_device {name}", stream,
                                  clobber=True)
    sc, ref = TR.assert_guard(name)
    for j, r in enumerate(ref):
        TR.assert_row(want, j, r, sc["cap"], f"{name}[{j}]")


# ---- the work area of one matcher handle in stream order -----------------------------------------
def test_six_calls_on_one_handle_behind_one_hold(dev):
    """Six successive calls wrap the handle's four staging slots and restart its arena six
    times while the first call has not begun: LocalBA and PoseOptimization alternate, each over
    two problems.  Each call's outputs are those of its run alone."""
    from orbslam2commentedbyxcm_amd.matcher import ORBmatcher
    from orbslam2commentedbyxcm_amd.optimizer import LocalBundleAdjuster, PoseOptimizer
    m = ORBmatcher(0.6, True)
    ba, pose = LocalBundleAdjuster(matcher=m), PoseOptimizer(matcher=m)
    runs = [(lb_runner(ba, ["mixed"]), LB_KEYS), (po_runner(pose, ["mono-9"]), PO_KEYS),
            (lb_runner(ba, ["edges-65"]), LB_KEYS), (po_runner(pose, ["mixed-257"]), PO_KEYS),
            (lb_runner(ba, ["mixed"]), LB_KEYS), (po_runner(pose, ["mono-9"]), PO_KEYS)]
    stream, _, _ = SO.probe(dev, runs[0][0], LB_KEYS, "matcher work area")
    sio = SO.SyncIO(dev)
    alone = [run(sio) for run, _ in runs]
    io = SO.OrderedIO(dev, sio.call_ms, "six calls on one matcher", stream=stream, floor_ms=CHAIN_FLOOR_MS)
    got = [run(io) for run, _ in runs]
    io.finish()
    assert io.calls == 6
    for i, (_, keys) in enumerate(runs):
        SO.same_bytes(got[i], alone[i], f"call {i}", keys)
    m.close()


# ---- the covisibility graph -----------------------------------------------------------------------
@pytest.fixture(scope="module", params=[None, 8], ids=["lds", "global"])
def cv(request, dev):
    """The graph on both histogram paths (test_gpu_covisibility.lds_bound)."""
    from orbslam2commentedbyxcm_amd import CovisibilityGraph
    from orbslam2commentedbyxcm_amd import _lib as L
    if request.param is not None:
        L.debug_set("covis_lds_keyframes", request.param)
    tables, _ = cv_case()
    K, cap = tables[0].shape
    g = CovisibilityGraph(K, cap, len(tables[3]), 64)
    stream, _, _ = SO.probe(dev, cv_runner(g), CV.RUN_KEYS, f"covisibility graph ({request.param or 'lds'})")
    yield g, stream
    g.close()
    L.debug_set("covis_lds_keyframes", -1)


def test_covisibility_calls_behind_a_hold(dev, cv):
    """refresh_observations, update_connections, erase_keyframe, best_covisibles and
    covisibles_by_weight; update_connections' host ids are overwritten on return."""
    g, stream = cv
    want, _ = ordered_equals_sync(dev, cv_runner(g), CV.RUN_KEYS, "covisibility graph", stream,
                                  floor_ms=CHAIN_FLOOR_MS, clobber=True)
    tables, _ = cv_case()
    model = CV.model_run(g.max_keyframes, g.max_conn, tables, CV_IDS, erase=CV_ERASE)
    assert np.array_equal(want["best"], model["best"]) and np.array_equal(want["by_weight_n"], model["by_weight_n"])


def lm_case():
    sc = CM.geometric_scene(0)
    return sc, CV.chain_decoy(sc)


def lm_runner(g, lba):
    sc, decoy = lm_case()

    def run(io, decoy_only=False):
        return CV.run_local_mapping(g, lba, decoy, io=io) if decoy_only else CV.run_local_mapping(g, lba, sc, io=io, decoy=decoy)
    return run


def test_local_mapping_chain_behind_a_hold(dev):
    """refresh_observations -> update_connections -> local_ba_assemble -> LocalBundleAdjustment ->
    local_ba_apply behind one hold; the host keyframe id and level table are overwritten on
    return.  (test_gpu_covisibility.test_chain_assemble_local_ba_apply compares the chain with
    the model and the host form.)"""
    from orbslam2commentedbyxcm_amd import CovisibilityGraph
    from orbslam2commentedbyxcm_amd.optimizer import LocalBundleAdjuster
    sc, _ = lm_case()
    K, cap = sc["kf_mp"].shape
    g, lba = CovisibilityGraph(K, cap, len(sc["mp_bad"]), 64), LocalBundleAdjuster()
    run = lm_runner(g, lba)
    # the chain has two handles, whose own streams are not ordered with each other: the probe is LocalBA's
    stream, _, _ = SO.probe(dev, lb_runner(lba, LB_SCENES[:1]), LB_KEYS, "LocalMapping chain (LocalBA)")
    want, _ = ordered_equals_sync(dev, run, CV.CHAIN_KEYS, "LocalMapping chain", stream, floor_ms=CHAIN_FLOOR_MS,
                                  clobber=True)
    assert want["status"][0] == 0 and want["trace"][0, 0, 0] > 0
    assert want["poses"].tobytes() != sc["poses"].tobytes() and want["mp_pos"].tobytes() != sc["mp_pos"].tobytes()
    lba.close()
    g.close()


def test_covisibility_stream_switch_waits_for_the_last_stream(dev, cv):
    """refresh_observations on a held stream, update_connections on a second stream at once:
    the second call waits for the first stream (orbx.h, the graph's stream rule) and gives the
    synchronised sequence's bytes."""
    import torch
    g, s1 = cv
    tables, decoys = cv_case()
    sio = SO.SyncIO(dev)
    want = CV.run_graph(g, tables, CV_IDS, io=sio, erase=None)
    io = SO.OrderedIO(dev, sio.call_ms, "covisibility stream switch", stream=s1)
    d = [io.up(a, b) for a, b in zip(tables, decoys)]
    K = g.max_keyframes
    best, best_n = io.full((K, 10), -9, torch.int32), io.full((K,), -9, torch.int32)
    byw, byw_n = io.full((K, g.max_conn), -9, torch.int32), io.full((K,), -9, torch.int32)
    s2 = torch.cuda.Stream(dev)
    io.begin()
    g.refresh_observations(*d, stream=s1)
    held_after_a = not s1.query()
    g.update_connections(np.asarray(CV_IDS, np.int32), stream=s2)
    s1_done_after_b = s1.query()
    g.best_covisibles(10, best, best_n, stream=s2)
    g.covisibles_by_weight(15, byw, byw_n, stream=s2)
    s2.synchronize()
    with torch.cuda.stream(s2):
        got = dict(best=best.cpu().numpy(), best_n=best_n.cpu().numpy(), by_weight=byw.cpu().numpy(),
                   by_weight_n=byw_n.cpu().numpy())
    io.finish(expect_async=False)
    assert held_after_a, "refresh_observations waited for the hold"
    assert s1_done_after_b, "the call on the second stream did not wait for the first"
    SO.same_bytes(got, want, "stream switch", CV.RUN_KEYS)


# ---- KeyFrameCulling ---------------------------------------------------------------------------------
def test_keyframe_culling_behind_a_hold(dev, cv):
    """covis_observation_counts_device -> keyframe_culling_device (with its SetBadFlag) behind one
    hold, on the held stream the graph's probe kept; a fresh graph per run."""
    import culling_model as CUM
    _, stream = cv
    m = CUM.SCENES["band"]()
    decoy = CU.decoy_scene(m)
    sio = SO.SyncIO(dev)
    want = CU.run_culling(dev, m, io=sio)
    other = CU.run_culling(dev, decoy)
    assert SO.differs(want, other, ("cand_counts", "culled", "counts"))
    io = SO.OrderedIO(dev, sio.call_ms, "observation counts + keyframe_culling_device", stream=stream,
                      floor_ms=CHAIN_FLOOR_MS)
    got = CU.run_culling(dev, m, io=io, decoy=decoy)
    io.finish()
    SO.same_bytes(got, want, "KeyFrameCulling", CU.CULL_KEYS)
    assert int(want["n_culled"][0]) > 0
    for r in (want, other, got):
        r["scene"].close()


@pytest.mark.parametrize("mode", ["set_bad", "map_points"])
def test_set_bad_flag_and_map_point_culling_behind_a_hold(dev, cv, mode):
    """covis_set_bad_flag_device (its host ids overwritten on return) and map_point_culling_device,
    each on its own behind a hold; a fresh graph per run."""
    import culling_model as CUM
    _, stream = cv
    m = CUM.SCENES["band"]()
    decoy = CU.decoy_scene(m)
    keys = CU.CULL_KEYS + (("recent", "n_recent", "n_mp_culled") if mode == "map_points" else ())
    sio = SO.SyncIO(dev)
    want = CU.run_culling(dev, m, io=sio, mode=mode)
    io = SO.OrderedIO(dev, sio.call_ms, f"culling {mode}", stream=stream, floor_ms=CHAIN_FLOOR_MS, clobber=True)
    got = CU.run_culling(dev, m, io=io, decoy=decoy, mode=mode)
    io.finish()
    SO.same_bytes(got, want, mode, keys)
    if mode == "set_bad":
        assert want["kf_bad"][list(CU.SET_BAD_IDS)].any()
    else:
        assert int(want["n_mp_culled"][0]) > 0
    for r in (want, got):
        r["scene"].close()


# ---- TrackLocalMap: UpdateLocalMap and the tally -----------------------------------------------------
TL_CASE = "band24"


def test_update_local_map_and_tally_behind_a_hold(dev):
    """update_local_map_device -> track_local_map_tally_device with nothing read back; the
    in/out lists and frame tables hold a decoy until the stream reaches the real uploads."""
    sc = TL.Scene(dev, TL_CASE)
    inp = TL.track_inputs(sc)
    decoy = TL.track_decoy(inp)

    def run(io, decoy_only=False):
        return TL.run_track(sc, decoy, io=io) if decoy_only else TL.run_track(sc, inp, io=io, decoy=decoy)
    stream, _, _ = SO.probe(dev, run, TL.TRACK_OUT_ONLY, "UpdateLocalMap + tally", floor_ms=CHAIN_FLOOR_MS)
    want, _ = ordered_equals_sync(dev, run, TL.TRACK_KEYS, "update_local_map_device + track_local_map_tally_device",
                                  stream, floor_ms=CHAIN_FLOOR_MS)
    assert want["local_off"][-1] > 0 and want["inliers"].max() > 0
    sc.close()


# ---- the TrackLocalMap chain, the host-offset search, new MapPoints, the triangulation search -----------
@pytest.fixture(scope="module")
def tlm(dev):
    st = TL.tlm_setup()
    st["decoy"] = TL.tlm_decoy(st["inp"])

    def run(io, decoy_only=False):
        if decoy_only:
            return TL.run_track_chain(st, io=io, inp=st["decoy"])
        return TL.run_track_chain(st, io=io, decoy=st["decoy"])

    def search(io, decoy_only=False):
        if decoy_only:
            return TL.run_track_chain(st, io=io, inp=st["decoy"], host_offsets=True)
        return TL.run_track_chain(st, io=io, decoy=st["decoy"], host_offsets=True)
    # the chain runs on two handles (the graph's tracker and the matcher); the probe is the matcher's search
    stream, _, _ = SO.probe(dev, search, ("nmatches",), "SearchLocalPoints (host offsets)")
    yield st, stream, run, search
    TL.tlm_close(st)


def test_track_local_map_chain_behind_a_hold(dev, tlm):
    """INTEGRATION.md's four asynchronous calls on one stream, nothing read back:
    update_local_map_device -> search_local_points_offsets_device -> pose_optimization_batch_device
    -> track_local_map_tally_device behind one hold; the scale factors and the level table are
    overwritten on return."""
    st, stream, run, _ = tlm
    want, got = ordered_equals_sync(dev, run, TL.TLM_KEYS, "TrackLocalMap chain", stream, floor_ms=CHAIN_FLOOR_MS,
                                    clobber=True)
    assert int(want["nmatches"].sum()) > 50 * st["B"] and want["inliers"].max() > 10


def test_search_local_points_host_offsets_may_be_reused_on_return(dev, tlm):
    """search_local_points_device: its host offsets and scale factors are overwritten on return."""
    st, stream, _, search = tlm
    want, _ = ordered_equals_sync(dev, search, ("frame_mp", "nmatches"), "search_local_points_device host offsets", stream,
                                  clobber=True)
    assert int(want["nmatches"].sum()) > 50 * st["B"]


def test_create_mappoints_and_update_last_frame_behind_a_hold(dev, tlm):
    """create_mappoints_device (its host scale factors overwritten on return) and
    update_last_frame_device on the chain's sequence.  Both take no handle: stream NULL is the
    null stream, which the probe's call then uses."""
    st = tlm[0]
    real, decoy = PD.new_point_inputs(st["seq"])

    def run(io, decoy_only=False):
        return PD.run_new_points(st["seq"], decoy, io=io) if decoy_only else PD.run_new_points(st["seq"], real, io=io,
                                                                                              decoy=decoy)
    stream, _, _ = SO.probe(dev, run, PD.NEW_POINT_KEYS, "create_mappoints + update_last_frame")
    want, _ = ordered_equals_sync(dev, run, PD.NEW_POINT_KEYS, "create_mappoints_device + update_last_frame_device",
                                  stream, clobber=True)
    n = st["seq"]["n"]
    assert (want["bad"][:n[0]] == 0).any() and want["has_mp"][0, :n[0]].any()


def test_search_for_triangulation_behind_a_hold(dev, oracle):
    """search_for_triangulation_batch_device: the host tables pairs and F12 are overwritten on
    return; pair 0 of the synchronous run against the oracle."""
    from orbslam2commentedbyxcm_amd.matcher import ORBmatcher
    case = MT._kf_views(oracle, 0)
    m = ORBmatcher(0.6, False)

    def run(io, decoy_only=False):
        return MT.run_search_for_triangulation(m, case, io=io, decoy=not decoy_only, decoy_only=decoy_only)
    stream, _, _ = SO.probe(dev, run, MT.SFT_KEYS, "SearchForTriangulation")
    want, _ = ordered_equals_sync(dev, run, MT.SFT_KEYS, "search_for_triangulation_batch_device", stream, clobber=True)
    views, has, fvs = case
    i, j = want["host_pairs"][0]
    pr = oracle.search_for_triangulation(views[i], has[i], fvs[i], views[j], has[j], fvs[j], want["F12"][0], False, False)
    assert want["npairs"][0] == len(pr) > 0 and np.array_equal(want["pairs"][0, :len(pr)], pr)
    m.close()


# ---- the keyframe database ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kf(dev):
    from orbslam2commentedbyxcm_amd import KeyFrameDatabase
    from orbslam2commentedbyxcm_amd.vocabulary import ORBVocabulary
    import vocab_scenes as VS
    V = ORBVocabulary(0)
    assert V.loadFromText(VS.make_vocab(71, k=10, L=3).text())
    db = KeyFrameDatabase(V, 65, 320)
    c = kf_case()
    KF.run_add(db, list(range(65)), c["bows"])

    def run(io, decoy_only=False):
        if decoy_only:
            return KF.run_queries(db, c["decoy_query"], c["ids"], c["decoy_reloc"], io=io, max_cand=65,
                                  min_score=KF.DECOY_MIN_SCORE)
        return KF.run_queries(db, c["query"], c["ids"], c["reloc"], io=io, decoy=(c["decoy_query"], c["decoy_reloc"]),
                              max_cand=65)
    stream, _, _ = SO.probe(dev, run, KF.QUERY_KEYS, "KeyFrameDatabase")
    yield db, stream, c, run
    db.close()
    V.close()


def test_kfdb_score_and_detect_behind_a_hold(dev, kf):
    """kfdb_score_device, detect_relocalization_candidates_device and detect_loop_candidates_device."""
    db, stream, c, run = kf
    want, _ = ordered_equals_sync(dev, run, KF.QUERY_KEYS, "kfdb_score_device + the two detections", stream)
    model = KM.Database()
    for i, b in enumerate(c["bows"]):
        model.add(i, b)
    assert np.array_equal(KF._u32(want["score"]), KF._u32(model.score(c["query"], c["ids"])))
    assert want["ncand"].max() > 0 and want["loop_ncand"].max() > 0


def test_kfdb_stream_switch_waits_for_the_last_stream(dev, kf):
    """kfdb_score_device on a held stream, the detections on a second stream at once: the first
    call on the second stream waits for the first stream (orbx.h, the database's stream rule).
    The score is used for the first call because kfdb_add_batch_device reads its counts back and
    so drains its stream itself: add then score could not show a missing wait."""
    import torch
    db, s1, c, run = kf
    sio = SO.SyncIO(dev)
    want = run(sio)
    io = SO.OrderedIO(dev, sio.call_ms, "database stream switch", stream=s1)
    s2 = torch.cuda.Stream(dev)
    with torch.cuda.stream(s2):
        io2 = SO.StreamIO(dev)
        got = KF.run_queries(db, c["query"], c["ids"], c["reloc"], io=io, decoy=(c["decoy_query"], c["decoy_reloc"]),
                             max_cand=65, switch_io=io2)
    io.finish(expect_async=False)
    assert io.returned_early == [True], "kfdb_score_device waited for the hold"
    assert io2.first_stream_done, "the call on the second stream did not wait for the first"
    SO.same_bytes(got, want, "score on a held stream, detections on a second", KF.QUERY_KEYS)


def test_kfdb_add_behind_a_hold(dev, kf):
    """kfdb_add_batch_device behind a hold, its host ids overwritten on return.  The call reads
    the counts back (the header says so: it synchronises its stream), so it is the one covered
    call that may return after the hold; this test does not exercise the stream-switch wait."""
    db, s1, c, run = kf
    want = run(SO.SyncIO(dev))
    db.clear()
    ids = np.arange(65, dtype=np.int32)
    io = SO.OrderedIO(dev, 0.5, "kfdb_add_batch_device", stream=s1, clobber=True)
    KF.run_add(db, ids, c["bows"], io=io, decoy=c["decoy_bows"], decoy_ids=ids[::-1].copy())
    io.finish(expect_async=False)
    got = run(SO.SyncIO(dev))
    SO.same_bytes(got, want, "queries after an add behind a hold", KF.QUERY_KEYS)
