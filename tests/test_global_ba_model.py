"""tests/global_ba_model.py against closed forms and Optimizer::BundleAdjustment's rules
(src/Optimizer.cc:41-281), and the host-only pieces of the library's global bundle adjustment.
No GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import global_ba_model as G
import local_ba_model as M
from pose_opt_model import se3_from_tcw, se3_to_tcw


@pytest.mark.parametrize("name", list(G.SPECS))
def test_every_named_scene_passes_its_guard(name):
    sc, vs, (ok, why), _ = G.checked(name)
    assert ok, (name, why)
    assert vs[0]["status"] == 0 and vs[0]["trace"][0] > 0


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_noise_free_scene_returns_to_the_truth(kind):
    """Without noise the minimum is the truth up to the float32 rounding of the observations and
    of the fixed poses (local_ba_model's bound: 1e-4 from 0.3 deg / 2 cm off)."""
    sc = M.make_scene(3, n_free=2, n_fixed=2, n_pts=30, kind=kind, noise=0.0)
    r = G.global_ba(sc, iterations=10, robust=False)
    free = ~np.asarray(sc["fixed"]).astype(bool)
    assert np.abs(sc["Tcw"][free].astype(np.float64) - sc["Tcw_true"][free]).max() > 1e-3
    assert np.abs(r["Tcw64"][free] - sc["Tcw_true"][free]).max() < 1e-4
    assert np.abs(r["pos64"] - sc["pos_true"]).max() < 1e-4
    assert r["pt_included"].all() and r["chi2"][1] < 1e-3 * r["chi2"][0]


def test_monocular_delta_is_sqrt_5_99():
    """cc:115: thHuber2D = sqrt(5.99), a float; the local BA's sqrt(5.991) gives another result
    where a robust edge is past the threshold."""
    assert G.DELTA_MONO == float(np.float32(np.sqrt(5.99))) and G.DELTA_MONO != M.DELTA_MONO
    sc = G.scene("mixed-out10")
    a = G.global_ba(sc, **G.params("mixed-out10"))
    b = G.global_ba(sc, delta_mono=M.DELTA_MONO, **G.params("mixed-out10"))
    assert sc["gross"].any() and a["chi2"][0] != b["chi2"][0]
    assert a["pos64"].tobytes() != b["pos64"].tobytes()
    c = G.global_ba(sc, iterations=10, robust=False)
    d = G.global_ba(sc, iterations=10, robust=False, delta_mono=M.DELTA_MONO)
    assert c["pos64"].tobytes() == d["pos64"].tobytes()       # bRobust = false: no kernel, no delta


def test_fixed_keyframe_comes_back_as_its_quaternion_round_trip():
    """cc:236-254 writes every keyframe: a fixed pose is toCvMat(toSE3Quat(pose))."""
    sc, vs, _, _ = G.checked("mixed")
    r = vs[0]
    fixed = np.asarray(sc["fixed"]).astype(bool)
    assert fixed.sum() == 2
    for k in np.nonzero(fixed)[0]:
        assert r["Tcw"][k].tobytes() == se3_to_tcw(*se3_from_tcw(sc["Tcw"][k])).astype(np.float32).tobytes()
    assert np.abs(r["Tcw"][fixed].astype(np.float64) - sc["Tcw"][fixed]).max() < 1e-6
    # a fixed pose whose float rotation is not orthonormal (here 0.1 % too long) shows the trip
    sc = dict(sc)
    k = int(np.nonzero(fixed)[0][0])
    T = sc["Tcw"].copy().reshape(-1, 3, 4)
    T[k, :, :3] *= np.float32(1.001)
    sc["Tcw"] = T.reshape(-1, 12)
    r = G.global_ba(sc, iterations=1, robust=False)
    assert r["Tcw"][k].tobytes() == se3_to_tcw(*se3_from_tcw(sc["Tcw"][k])).astype(np.float32).tobytes()
    assert r["Tcw"][k].tobytes() != sc["Tcw"][k].tobytes()
    assert np.abs(np.linalg.det(r["Tcw"][k].reshape(3, 4)[:, :3].astype(np.float64)) - 1.0) < 1e-6


def test_points_without_an_edge_and_idle_keyframes():
    sc, vs, _, _ = G.checked("odd")
    r = vs[0]
    cnt = np.diff(sc["obs_off"])
    assert (cnt == 1).any() and (cnt == 0).any()
    assert np.array_equal(r["pt_included"], (cnt > 0).astype(np.uint8))
    assert r["pos"][cnt == 0].tobytes() == sc["pos"][cnt == 0].tobytes()
    fixed = np.asarray(sc["fixed"]).astype(bool)
    assert fixed.tolist() == [True, False, False, True, False]
    assert r["active_kf"][0] == [1, 2]                                # the last keyframe may move but has no edge
    assert r["Tcw"][4].tobytes() == se3_to_tcw(*se3_from_tcw(sc["Tcw"][4])).astype(np.float32).tobytes()
    assert not np.array_equal(np.sort(sc["slot"]), sc["slot"]) and (np.diff(sc["obs_kp"]) < 0).any()


def test_problems_that_return_their_inputs():
    none = G.global_ba(M.make_scene(0, n_free=0, n_fixed=3, n_pts=12))
    assert none["status"] == G.STATUS_NO_FREE_KF and not none["trace"].any() and not none["pt_included"].any()
    sc = G.scene("banded-63")
    blocks = G.envelope_blocks(sc)
    over = G.global_ba(sc, max_env_blocks=blocks - 1)
    assert over["status"] == G.STATUS_CAPACITY and over["Tcw"].tobytes() == sc["Tcw"].tobytes()
    fits = G.global_ba(sc, iterations=1, robust=False, max_env_blocks=blocks)
    assert fits["status"] == 0 and fits["trace"][0] == 1


def test_sparse_factorisation_is_the_dense_one():
    rng = np.random.default_rng(5)
    n = 30
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(i, min(i + 4, n)):
            A[i, j] = rng.normal()
        A[i, i] = 10.0 + rng.uniform()
    A[1, n - 1] = A[2, n - 2] = 0.5
    b = rng.normal(size=n)
    for perm in ("natural", "reversed", 7):
        x0, p0 = M.ldlt_solve(A, b, perm)
        x1, p1 = G.ldlt_solve_sparse(A, b, perm)
        assert x0.tobytes() == x1.tobytes() and p0.tobytes() == p1.tobytes()
    assert np.abs((np.triu(A) + np.triu(A, 1).T) @ x0 - b).max() < 1e-12


@pytest.mark.parametrize("name", G.BANDED)
def test_envelope_of_a_banded_map_is_small_and_the_librarys(orbx_built, name):
    """The brute-force count against orbx_global_ba_envelope (host only, no GPU)."""
    from orbslam2commentedbyxcm_amd.optimizer import global_ba_envelope
    sc = G.scene(name)
    F = int((~np.asarray(sc["fixed"]).astype(bool)).sum())
    blocks = G.envelope_blocks(sc)
    assert blocks < F * (F + 1) // 4
    assert global_ba_envelope(sc["fixed"], sc["obs_off"], sc["obs_kf"]) == blocks
    first_loop = int(sc["obs_off"][-4])                              # the loop points make two long columns
    assert sc["obs_kf"][first_loop:first_loop + 4].tolist() == [1, 2, len(sc["fixed"]) - 2, len(sc["fixed"]) - 1]


def test_envelope_of_small_and_dense_maps(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import global_ba_envelope
    for name in ("1+1-6pts", "odd", "mixed", "pts-257"):
        sc = G.scene(name)
        assert global_ba_envelope(sc["fixed"], sc["obs_off"], sc["obs_kf"]) == G.envelope_blocks(sc), name
    assert global_ba_envelope(np.zeros(0, np.uint8), np.zeros(1, np.int32), np.zeros(0, np.int32)) == 0


def test_argument_checks_need_no_gpu(orbx_built):
    """orbx_global_bundle_adjustment_batch_device / orbx_global_bundle_adjustment reject bad
    arguments before any GPU call."""
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)
    sig = (C.c_float * 8)(*M.INV_SIGMA2)

    def batch(**kw):
        q = L.GlobalBaBatch(batch=2, kf_off=fake, n_kf=4, kf_Tcw=fake, kf_fixed=fake, kf_slot=fake, pt_off=fake, n_pt=8,
                            pt_pos=fake, obs_off=fake, n_obs=16, obs_kf=fake, obs_kp=fake, n_slots=4, cap=16, kps=fake,
                            u_right=None, inv_level_sigma2=sig, nlevels=8, fx=500.0, fy=500.0, cx=320.0, cy=240.0,
                            bf=40.0, iterations=10, robust=1, max_env_blocks=10, dense=0, kf_Tcw_opt=fake,
                            pt_pos_opt=fake, pt_included=fake, trace=None, chi2=None, status=fake)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    h = C.c_void_p(0x2000)      # never dereferenced: the checks come first
    dev, host = lib.orbx_global_bundle_adjustment_batch_device, lib.orbx_global_bundle_adjustment
    assert dev(None, C.byref(batch()), None) == L.ORBX_ERR_ARG
    assert dev(h, None, None) == L.ORBX_ERR_ARG
    for kw in (dict(batch=-1), dict(cap=0), dict(nlevels=0), dict(nlevels=99), dict(n_obs=-1), dict(iterations=-1),
               dict(max_env_blocks=-1), dict(max_env_blocks=1 << 31), dict(inv_level_sigma2=None), dict(kf_off=None),
               dict(status=None), dict(kf_Tcw_opt=None), dict(pt_pos=None), dict(pt_included=None), dict(kps=None),
               dict(obs_kp=None), dict(n_slots=1 << 20, cap=1 << 12)):
        assert dev(h, C.byref(batch(**kw)), None) == L.ORBX_ERR_ARG, kw
        if "batch" not in kw:
            assert host(h, C.byref(batch(batch=1, **kw))) == L.ORBX_ERR_ARG, kw
    assert host(h, C.byref(batch())) == L.ORBX_ERR_ARG          # batch 2
    assert b"one problem" in lib.orbx_last_error()
    off = (C.c_int32 * 2)(0, 3)
    q = batch(batch=1, kf_off=C.cast(off, C.c_void_p), pt_off=C.cast(off, C.c_void_p))
    assert host(h, C.byref(q)) == L.ORBX_ERR_ARG                 # kf_off[1] != n_kf
    assert b"offsets" in lib.orbx_last_error()
    n = C.c_int64(0)
    assert lib.orbx_global_ba_envelope(-1, None, 0, None, None, 0, C.byref(n)) == L.ORBX_ERR_ARG
    assert lib.orbx_global_ba_envelope(0, None, 0, None, None, 0, None) == L.ORBX_ERR_ARG
