"""The decoy rule of the stream-order tests (tests/stream_order.py), on the CPU: for every decoy
test_gpu_stream_order.py uses, index and offset arrays equal the real input's, every payload
array differs, and the model gives another result for the decoy -- so a run that read a decoy,
or any element-wise mixture, stays in bounds and comes out wrong."""
from __future__ import annotations

import numpy as np
import pytest

import covisibility_model as CM
import kfdb_model as KM
import local_ba_model as LM
import pose_opt_model as PM
import stream_order as SO
import test_gpu_covisibility as CV
import test_gpu_kfdb as KF
import test_gpu_local_ba as LB
import test_gpu_pose_opt as PO
import test_gpu_stream_order as T


def arrays(d):
    return {k: v for k, v in d.items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("name", T.PO_SCENES)
def test_pose_optimization_decoy(name):
    scenes, decoys = T.po_case([name])
    P, Q = PO.pack(scenes), PO.pack(decoys)
    payload = T.PO_PAYLOAD - ({"ur"} if P["ur"] is None else set())
    SO.check_decoy(arrays(P), arrays(Q), payload, name)
    assert np.array_equal(P["kps"]["octave"], Q["kps"]["octave"])
    a, b = PM.run_model(scenes[0]), PM.run_model(decoys[0])
    assert not np.array_equal(a["Tcw"], b["Tcw"])


@pytest.mark.parametrize("name", T.LB_SCENES)
def test_local_ba_decoy(name):
    scenes, decoys = T.lb_case([name])
    A, Q = LB.upload_arrays(scenes), LB.upload_arrays(decoys)
    SO.check_decoy(arrays(A), arrays(Q), T.LB_PAYLOAD, name)
    a, b = LM.local_ba(scenes[0]), LM.local_ba(decoys[0])
    assert not np.array_equal(a["Tcw"], b["Tcw"]) and not np.array_equal(a["pos"], b["pos"])


@pytest.mark.parametrize("name", T.GB_SCENES)
def test_global_ba_decoy(name):
    import global_ba_model as GM
    import test_gpu_global_ba as GB
    scenes, decoys = T.gb_case([name])
    A, Q = GB.upload_arrays(scenes), GB.upload_arrays(decoys)
    payload = T.LB_PAYLOAD - (set() if not np.array_equal(A["u_right"], Q["u_right"]) else {"u_right"})
    SO.check_decoy(arrays(A), arrays(Q), payload, name)
    assert payload >= {"Tcw", "pos", "kps_xy", "kps"}
    kw = GM.params(name)
    a, b = GM.global_ba(scenes[0], **kw), GM.global_ba(decoys[0], **kw)
    assert not np.array_equal(a["Tcw"], b["Tcw"])


@pytest.mark.parametrize("name", T.S3_SCENES)
def test_optimize_sim3_decoy(name):
    import optimize_sim3_model as SM
    scenes, decoys = T.s3_case([name])
    SO.check_decoy(arrays(SM.pack(scenes)), arrays(SM.pack(decoys)), T.S3_PAYLOAD, name)
    P, Q = SM.pack(scenes), SM.pack(decoys)
    assert np.array_equal(P["kps1"]["octave"], Q["kps1"]["octave"]) and P["cap1"] == Q["cap1"]
    R = Q["R12"][0].reshape(3, 3).astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5                           # still a rotation
    a, b = SM.optimize_sim3(scenes[0]), SM.optimize_sim3(decoys[0])
    assert not np.array_equal(a["R12"], b["R12"]) or not np.array_equal(a["t12"], b["t12"])


@pytest.mark.parametrize("name", T.EG_SCENES)
def test_essential_graph_decoy(name):
    import essential_graph_model as EM
    scenes, decoys = T.eg_case([name])
    SO.check_decoy(arrays(EM.pack(scenes)), arrays(EM.pack(decoys)), T.EG_PAYLOAD, name)
    k = EM.exact_iterations(name)
    a, b = EM.essential_graph(scenes[0], iterations=k), EM.essential_graph(decoys[0], iterations=k)
    assert not np.array_equal(a["Tcw"], b["Tcw"])


@pytest.mark.parametrize("name", T.TR_SCENES)
def test_triangulate_decoy(name):
    import test_gpu_triangulate as TR
    import triangulate_model as TM
    sc = TM.scene(name)
    P = TM.pack(sc)
    Q = TR.decoy_pack(P)
    for k in ("pairs", "d_pairs", "npairs"):
        assert np.array_equal(P[k], Q[k]), k
    for K, D in zip(P["kfs"], Q["kfs"]):
        present = {k for k in ("keys_un", "keys") if K[k] is not None}
        present |= {k for k in ("u_right", "depth") if K[k] is not None and (K[k] > 0).any()}   # -1: none to move
        SO.check_decoy({k: K[k] for k in K if K[k] is not None}, {k: D[k] for k in D if D[k] is not None}, present,
                       name)
        assert np.array_equal(K["keys_un"]["octave"], D["keys_un"]["octave"])
    pairs = np.asarray(P["pairs"]).reshape(-1, 2)
    assert not np.array_equal(pairs, pairs[:, ::-1]) and pairs[:, ::-1].max() < len(P["kfs"])


def test_level_table_decoy_is_another_valid_table():
    sig = np.asarray(PM.INV_SIGMA2, np.float32)
    assert (sig[::-1] > 0).all() and not np.array_equal(sig, sig[::-1])
    sc = PM.scene("mixed-257")
    fx, fy, cx, cy, bf = sc["cam"]
    n = sc["n"]
    a = PM.run_model(sc)
    b = PM.pose_optimization(sc["keys_xy"][:n], sc["octave"][:n], sc["u_right"][:n], sc["mp"][:n], sc["pos"], sig[::-1],
                             fx, fy, cx, cy, bf, sc["tcw"])
    assert not np.array_equal(a["Tcw"], b["Tcw"])


def test_covisibility_decoy():
    tables, decoys = T.cv_case()
    names = ("kf_mp", "kf_n", "kf_bad", "mp_bad")
    SO.check_decoy(dict(zip(names, tables)), dict(zip(names, decoys)), {"kf_mp", "mp_bad"}, "covisibility")
    kf_mp, n = decoys[0], len(tables[3])
    assert kf_mp.min() >= -1 and kf_mp.max() < n and tables[0].max() < n     # the same id range
    K = len(kf_mp)
    real = CV.model_run(K, 64, tables, T.CV_IDS, erase=T.CV_ERASE)
    other = CV.model_run(K, 64, decoys, T.CV_IDS, erase=T.CV_ERASE)
    assert SO.differs(real, other, CV.RUN_KEYS)
    ids2 = T.cv_decoy_ids(T.CV_IDS)
    assert len(set(ids2.tolist())) == len(T.CV_IDS) and ids2.min() >= 0 and ids2.max() < K
    assert SO.differs(real, CV.model_run(K, 64, tables, ids2.tolist(), erase=T.CV_ERASE), CV.RUN_KEYS)


def test_correct_loop_decoy():
    import correct_loop_model as CLM
    import test_gpu_correct_loop as CL
    sc, st = CLM.scene("hand")
    dst, dScw = CL.decoy_state("hand")
    real = {k: np.asarray(v) for k, v in st.items() if isinstance(v, np.ndarray)}
    other = {k: np.asarray(v) for k, v in dst.items() if isinstance(v, np.ndarray)}
    SO.check_decoy(real, other, set(CL.STATE_PAYLOAD), "CorrectLoop state")
    assert not np.array_equal(dScw, sc["Scw"]) and dScw.shape == np.asarray(sc["Scw"]).shape
    assert np.array_equal(dScw[:4], np.asarray(sc["Scw"])[:4]) and dScw[7] == sc["Scw"][7]     # the rotation and scale
    a = CLM.propagate(CLM.graph_of(sc), {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in st.items()},
                      sc["cur"], np.asarray(sc["Scw"]))
    b = CLM.propagate(CLM.graph_of(sc), {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in dst.items()},
                      sc["cur"], dScw)
    for k in ("corr_S", "poses", "mp_pos", "normal", "kf_Tcw_nc"):
        assert not np.array_equal(a[k], b[k]), k


def test_culling_decoy():
    import culling_model as CUM
    import test_gpu_culling as CU
    m = CUM.SCENES["band"]()
    d = CU.decoy_scene(m)
    real = {k: np.asarray(v) for k, v in m.items() if isinstance(v, np.ndarray)}
    other = {k: np.asarray(v) for k, v in d.items() if isinstance(v, np.ndarray)}
    SO.check_decoy(real, other, set(CU.CULL_PAYLOAD), "culling")
    a, b = CUM.copy_maps(m), CUM.copy_maps(d)
    ra = CUM.key_frame_culling(CUM.build_graph(a, 64), a, m["cur"], m["monocular"], m["not_erase"])
    rb = CUM.key_frame_culling(CUM.build_graph(b, 64), b, m["cur"], m["monocular"], m["not_erase"])
    assert ra["cand_counts"].tolist() != rb["cand_counts"].tolist() or ra["culled"].tolist() != rb["culled"].tolist()


def test_map_point_culling_and_set_bad_flag_decoys():
    import culling_model as CUM
    import test_gpu_culling as CU
    m = CUM.SCENES["band"]()
    real, decoy = CU.recent_inputs(m)
    SO.check_decoy(real, decoy, {"recent", "first", "found", "visible"}, "map_point_culling")
    n0 = int(real["n"][0])
    assert sorted(decoy["recent"][:n0].tolist()) == sorted(real["recent"][:n0].tolist())      # valid ids
    K = len(m["kf_bad"])
    assert decoy["first"].min() >= real["first"].min() and decoy["first"].max() <= real["first"].max()
    assert decoy["found"].min() >= 0 and decoy["visible"].min() >= 1
    a, b = CUM.copy_maps(m), CUM.copy_maps(m)
    ra = CUM.map_point_culling(CUM.build_graph(a, 64), a, real["recent"][:n0], 10, m["monocular"], real["found"],
                               real["visible"], real["first"])
    rb = CUM.map_point_culling(CUM.build_graph(b, 64), b, decoy["recent"][:n0], 10, m["monocular"], decoy["found"],
                               decoy["visible"], decoy["first"])
    assert list(ra[0]) != list(rb[0]) or ra[1] != rb[1]
    ids, other = CU.SET_BAD_IDS, CU.SET_BAD_DECOY_IDS
    assert len(ids) == len(other) and all(0 <= k < K for k in other) and len(set(other)) == len(other)
    a, b = CUM.copy_maps(m), CUM.copy_maps(m)
    ga, gb = CUM.build_graph(a, 64), CUM.build_graph(b, 64)
    for k, k2 in zip(ids, other):
        CUM.set_bad_flag(ga, a, k, m["not_erase"])
        CUM.set_bad_flag(gb, b, k2, m["not_erase"])
    assert not np.array_equal(a["kf_bad"], b["kf_bad"])


def _keypoint_words(rng, shape):
    """Keypoint records as seven int32 words: x, y, size, angle, response (floats), octave, class_id."""
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    k = np.zeros(shape, KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(20, 600, shape), rng.uniform(20, 440, shape)
    k["octave"] = rng.integers(0, 8, shape)
    return k.view(np.int32).reshape(shape + (7,)).copy(), k


def test_front_end_decoys_keep_counts_octaves_and_ids():
    """The decoys of the TrackLocalMap chain, of create_mappoints / update_last_frame and of the
    triangulation search, on arrays of the GPU tests' layout (those tests' inputs come from the
    extractor; their probes assert on the device that the decoy gives other outputs)."""
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    import test_gpu_local_map as TL
    import test_gpu_match as MT
    import test_gpu_posed as PD
    rng = np.random.default_rng(3)
    B, cap = 3, 40
    N = B * cap
    words, k = _keypoint_words(rng, (B, cap))
    inp = dict(pos=rng.normal(size=(N, 3)).astype(np.float32), desc=rng.integers(0, 256, (N, 32), dtype=np.uint8),
               normal=rng.normal(size=(N, 3)).astype(np.float32), max_distance=rng.uniform(2, 9, N).astype(np.float32),
               min_distance=rng.uniform(0.5, 2, N).astype(np.float32), observations=rng.integers(0, 4, N).astype(np.int32),
               bad=(rng.random(N) < 0.1).astype(np.uint8), kps=words, kp_desc=rng.integers(0, 256, (B, cap, 32), dtype=np.uint8),
               n=np.full(B, cap - 2, np.int32), T=rng.normal(size=(B, 12)).astype(np.float32),
               fmp0=rng.integers(-1, N, (B, cap)).astype(np.int32), rec=np.zeros(B, np.uint8), found=np.zeros(N, np.int32))
    d = TL.tlm_decoy(inp)
    SO.check_decoy(inp, d, TL.TLM_PAYLOAD, "TrackLocalMap chain")
    kd = d["kps"].view(np.uint8).reshape(B, cap, 28).view(KEYPOINT_DTYPE).reshape(B, cap)
    assert np.array_equal(kd["octave"], k["octave"]) and not np.array_equal(kd["x"], k["x"])
    assert d["observations"].min() >= 0 and d["observations"].max() <= 3
    off = np.array([0, 10, 25, 40, 41], np.int32)
    o2 = TL.tlm_decoy_offsets(off)
    assert o2[0] == 0 and o2[-1] == off[-1] and (np.diff(o2) >= 0).all() and not np.array_equal(o2, off)
    real = dict(kps=words, n=inp["n"], T=inp["T"], depth=np.where(rng.random((B, cap)) < 0.2, -1.0, 5.0).astype(np.float32))
    nd = PD.new_point_decoy(real)
    SO.check_decoy(real, nd, {"kps", "T", "depth"}, "new MapPoints")
    assert np.array_equal(nd["depth"] > 0, real["depth"] > 0)
    tabs = dict(kp=words[0], de=inp["kp_desc"][0], hm=inp["bad"][:cap], node=np.arange(cap, dtype=np.int32),
                ur=np.where(rng.random(cap) < 0.3, -1.0, 100.0).astype(np.float32))
    kd = {name: MT._kf_decoy(name, a) for name, a in tabs.items()}
    SO.check_decoy(tabs, kd, {"kp", "de", "ur"}, "triangulation search")
    assert np.array_equal(kd["ur"] >= 0, tabs["ur"] >= 0) and np.array_equal(kd["kp"][:, 5], words[0][:, 5])


def test_track_local_map_decoy():
    import local_map_model as LMM
    import test_gpu_local_map as TL
    c = LMM.gpu_case(T.TL_CASE)
    inp = TL.track_inputs(c)
    decoy = TL.track_decoy(inp)
    SO.check_decoy(inp, decoy, {"frame_mp", "outlier", "observations", "found"}, "TrackLocalMap")
    n_mp = len(c["map"][3])
    assert decoy["frame_mp"].max() <= inp["frame_mp"].max() and decoy["frame_mp"].min() >= inp["frame_mp"].min()
    assert decoy["observations"].max() <= 2 and n_mp == len(decoy["found"])
    m = LMM.build_graph(*c["map"], c["later_bad"], c["max_conn"])
    mk, B = c["max_local_kf"], len(inp["frame_mp"])
    a = LMM.update_local_map_batch(m, inp["frame_mp"], inp["n"], *LMM.initial_lists(B, mk), mk, 10 ** 6, 10 ** 6)
    m2 = LMM.build_graph(*c["map"], c["later_bad"], c["max_conn"])
    b = LMM.update_local_map_batch(m2, decoy["frame_mp"], inp["n"], *LMM.initial_lists(B, mk), mk, 10 ** 6, 10 ** 6)
    assert not np.array_equal(a["counts"], b["counts"]) and not np.array_equal(a["local_off"], b["local_off"])
    ta = LMM.tally(a["frame_mp"], inp["n"], inp["outlier"], inp["observations"], False, True, inp["rec"], inp["found"])
    tb = LMM.tally(a["frame_mp"], inp["n"], decoy["outlier"], decoy["observations"], False, True, inp["rec"], decoy["found"])
    assert not np.array_equal(ta[1], tb[1]) and not np.array_equal(ta[3], tb[3])


def test_keyframe_database_decoys():
    c = T.kf_case()
    SO.check_decoy(KF.bow_tables(c["bows"]), KF.bow_tables(c["decoy_bows"]), {"value"}, "bows")
    SO.check_decoy(KF.bow_tables([c["query"]]), KF.bow_tables([c["decoy_query"]]), {"value"}, "query")
    SO.check_decoy(KF.bow_tables(c["reloc"]), KF.bow_tables(c["decoy_reloc"]), {"value"}, "reloc queries")
    real, other = KM.Database(), KM.Database()
    for i in range(65):
        real.add(i, c["bows"][i])
        other.add(i, c["decoy_bows"][i])
    want = real.score(c["query"], c["ids"])
    assert not np.array_equal(want, other.score(c["query"], c["ids"]))        # decoy keyframes
    assert not np.array_equal(want, real.score(c["decoy_query"], c["ids"]))   # decoy query
    rev = KM.Database()
    for i in range(65):
        rev.add(64 - i, c["bows"][i])                                          # decoy ids of the add
    assert not np.array_equal(want, rev.score(c["query"], c["ids"]))
