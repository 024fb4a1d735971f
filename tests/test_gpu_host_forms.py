"""The single host forms on one live handle: small, large, small.

Every host form stages its problem in a grow-only device buffer that the handle keeps
(csrc/orbx_host.h).  Three calls of 8, about 300 and 8 keypoints on one handle cover what the
per-feature tests reach only by accident: the buffer growing while the handle is live, a
smaller problem in a larger buffer (stale bytes beyond n), and the arrays that are uploaded
into the result block (outlier, matches12).  Each call must give, byte for byte, what the
batch form gives for the same input on a fresh handle.

The scenes and the batch calls are the per-feature tests' own.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import initializer_model as MI
import optimize_sim3_model as MO
import pose_opt_model as MP
import sim3_model as MS
import test_gpu_initializer as TI
import test_gpu_optimize_sim3 as TO
import test_gpu_pose_opt as TP
import test_gpu_sim3 as TS
import test_gpu_triangulate as TT
import triangulate_model as MT

pytestmark = pytest.mark.gpu


def test_pose_optimization(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import PoseOptimizer
    live = PoseOptimizer()
    for seed, nedges in ((1, 6), (2, 225), (3, 6)):
        sc = MP.make_scene(seed, nedges, kind="mixed", **MP.KINDS["mixed"])
        n = sc["n"]
        assert n == (8 if nedges == 6 else 300) == sc["cap"]
        fresh = PoseOptimizer()
        want = TP.run_batch(fresh, [sc], outlier_init=1)
        fresh.close()
        P = want["packed"]                               # the ids as the batch call was given them
        fx, fy, cx, cy, bf = sc["cam"]
        h = live.PoseOptimization(P["kps"][0], P["ur"][0], P["mp"][0], P["pos"], MP.INV_SIGMA2, fx, fy, cx, cy, bf,
                                  sc["tcw"], outlier=np.ones(n, np.uint8))
        assert h["Tcw"].tobytes() == want["Tcw"][0].tobytes(), n
        assert h["outlier"].tobytes() == want["outlier"][0].tobytes(), n
        assert h["trace"].tobytes() == want["trace"][0].tobytes(), n
        assert (h["ninliers"], h["ninit"]) == (want["ninliers"][0], want["ninit"][0]), n
    live.close()


def test_optimize_sim3(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import Sim3Optimizer
    live = Sim3Optimizer()
    for seed, npairs in ((1, 5), (2, 225), (3, 5)):
        sc = MO.make_scene(seed, npairs, nout=npairs // 10)
        n1, n2 = sc["n1"], sc["n2"]
        assert n1 == (8 if npairs == 5 else 300) == sc["cap1"]
        assert (sc["matches12"][:n1] < 0).any()     # holes that must arrive as they are
        fresh = Sim3Optimizer()
        want = TO.run_batch(fresh, [sc])
        fresh.close()
        P = want["packed"]                               # the ids as the batch call was given them
        h = live.OptimizeSim3(P["kps1"][0, :n1], P["mp1"][0, :n1], P["m12"][0, :n1], P["idx2"][0, :n1],
                              P["kps2"][0, :n2], P["pos"], sc["Tcw1"], sc["Tcw2"], sc["inv_sigma2_1"],
                              sc["inv_sigma2_2"], sc["K1"], sc["K2"], sc["R12"], sc["t12"], sc["s12"], sc["th2"],
                              sc["fix_scale"])
        got = np.concatenate([h["R12"], h["t12"], [h["s12"]]]).astype(np.float32)
        assert got.tobytes() == TO.s12_of(want, 0).tobytes(), n1
        assert np.asarray(h["matches12"], np.int32).tobytes() == want["m12"][0, :n1].tobytes(), n1
        assert h["trace"].tobytes() == want["trace"][0].tobytes(), n1
        assert (h["ninliers"], h["ncorr"], h["nbad"]) == (want["ninliers"][0], want["ncorr"][0], want["nbad"][0]), n1
    live.close()


def test_triangulate_pairs(orbx_built):
    from orbslam2commentedbyxcm_amd.mapping import Triangulator
    live = Triangulator()

    def host(K):
        return dict(keys_un=MT.keypoints(K["un"], K["oct"]), Tcw=np.asarray(K["Tcw"]).reshape(3, 4), u_right=K["u_right"],
                    depth=K["depth"], keys=None if K["raw"] is None else MT.keypoints(K["raw"], K["oct"]))

    for seed, count in ((1, 8), (2, 300), (3, 8)):
        sc = MT.make_scene(seed, 2, ((0, 1, count),), 320)
        assert sc["kfs"][0]["n"] == sc["kfs"][1]["n"] == count
        fresh = Triangulator()
        want = TT.run_batch(fresh, sc)
        fresh.close()
        h = live.triangulate_pairs(host(sc["kfs"][0]), host(sc["kfs"][1]), MT.cam(), sc["matched"][0])
        for nm in TT.NAMES[:-2]:
            assert h[nm].tobytes() == want[nm][0, :count].tobytes(), (count, nm)
        nnew = int(want["nnew"][0])
        assert 0 < nnew < count and h["nnew"] == nnew
        assert np.asarray(h["new_idx"], np.int32).tobytes() == want["new_idx"][0, :nnew].tobytes(), count
    live.close()


def _sim3_set(handle, sc):
    """orbx_sim3_set of the scene's n1 slots, with cap = n1: the staging is sized by it."""
    from orbslam2commentedbyxcm_amd import _lib as L
    n1 = int(sc["n1"])
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    keep = dict(n1=np.array([n1], np.int32), mp1=i32(sc["mp1"][:n1]), mp2=i32(sc["mp2"][:n1]), oct1=i32(sc["oct1"][:n1]),
                oct2=i32(sc["oct2"][:n1]), mp_pos=f32(sc["mp_pos"]), Tcw1=f32(sc["Tcw1"]), Tcw2=f32(sc["Tcw2"]),
                draws=i32(sc["draws"]), level_sigma2=f32(sc["level_sigma2"]), K1=f32(sc["K1"]), K2=f32(sc["K2"]))
    q = L.Sim3Batch()
    q.batch, q.cap, q.n_mp, q.nlevels = 1, n1, len(keep["mp_pos"]), len(keep["level_sigma2"])
    for k in ("n1", "mp1", "mp2", "oct1", "oct2", "mp_pos", "Tcw1", "Tcw2", "draws"):
        setattr(q, k, C.c_void_p(keep[k].ctypes.data))
    for k in ("level_sigma2", "K1", "K2"):
        setattr(q, k, keep[k].ctypes.data_as(C.POINTER(C.c_float)))
    q.fix_scale, q.probability = int(sc["fix_scale"]), float(sc["probability"])
    q.min_inliers, q.max_iterations = int(sc["min_inliers"]), int(sc["max_iterations"])
    L.check(L.lib().orbx_sim3_set(handle, C.byref(q)))


def _sim3_iterate(handle, n1, n_iterations):
    from orbslam2commentedbyxcm_amd import _lib as L
    o = {k: np.full(1, -9, np.int32) for k in TS.INT_KEYS}
    o["inliers"] = np.full(n1, TS.FILL, np.uint8)
    for k, n in TS.F32_KEYS:
        o[k] = np.full(n, -5.0, np.float32)
    r = L.Sim3Result()
    for k, a in o.items():
        setattr(r, k, C.c_void_p(a.ctypes.data))
    L.check(L.lib().orbx_sim3_iterate(handle, int(n_iterations), C.byref(r)))
    return o


def test_sim3(orbx_built):
    from orbslam2commentedbyxcm_amd.sim3 import Sim3Solver
    its = 8
    live = Sim3Solver(max_batch=1, cap=512, max_iterations=its)
    schedule = (3, "find")   # two iterates after one set: the handle's result block is read twice
    for seed, n_valid, n_slots in ((1, 6, 8), (2, 230, None), (3, 6, 8)):
        sc = MS.build_scene(seed, n_valid, cap=512, outliers=0.2 if n_valid > 6 else 0.0, min_inliers=3,
                            max_iterations=its, n_slots=n_slots)
        n1 = int(sc["n1"])
        assert n1 == (8 if n_valid == 6 else 306)
        fresh = Sim3Solver(max_batch=1, cap=512, max_iterations=its)
        want = TS.run_batch(fresh, [sc], schedule)
        fresh.close()
        _sim3_set(live._h, sc)
        for c, w in zip(schedule, want):
            h = _sim3_iterate(live._h, n1, its if c == "find" else c)
            w0 = TS.one(w, 0)
            for k in h:
                a = w0[k][:n1] if k == "inliers" else w0[k]
                assert np.asarray(h[k]).reshape(-1).tobytes() == np.asarray(a).reshape(-1).tobytes(), (n1, c, k)
    assert live.last_call_us() > 0
    live.close()


def test_initializer(orbx_built):
    from orbslam2commentedbyxcm_amd.initializer import Initializer
    live = Initializer(max_batch=1, kcap=TI.KCAP, max_iterations=8)
    for seed, N, extra, its in ((1, 8, 0, 1), (2, 270, None, 8), (3, 8, 0, 1)):
        sc = MI.make_scene(seed, N, outliers=0.2 if N > 8 else 0.0, iterations=its, extra=extra)
        n1 = len(sc["keys1"])
        assert n1 == (8 if N == 8 else 303)
        fresh = Initializer(max_batch=1, kcap=TI.KCAP, max_iterations=8)
        want = {k: v[0] for k, v in TI.run_batch(fresh, [sc]).items()}
        fresh.close()
        o = live.initialize_host(MI.keypoints(sc["keys1"]), MI.keypoints(sc["keys2"]), sc["matches12"], MI.K4,
                                 sc["sets"], max_iterations=its)
        for k, v in o.items():
            w = want[k][:n1] if np.ndim(want[k]) and want[k].shape[0] == TI.KCAP else want[k]
            assert np.asarray(v).reshape(-1).tobytes() == np.asarray(w).reshape(-1).tobytes(), (n1, k)
    live.close()
