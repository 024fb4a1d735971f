"""tests/pose_opt_model.py, the float64 restatement of Optimizer::PoseOptimization that the
GPU tests compare with, checked on its own (no GPU): Jacobians against central differences,
recovery of the true pose, outlier flags, the two early exits; and the new C ABI's argument
checks, which run before any device call."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import pose_opt_model as M


def _edges(sc):
    n = sc["n"]
    ur = None if sc["u_right"] is None else sc["u_right"][:n]
    return M.Edges(sc["keys_xy"][:n], sc["octave"][:n], ur, sc["mp"][:n], sc["pos"], M.INV_SIGMA2)


@pytest.mark.parametrize("kind", ["mono", "mixed"])
def test_analytic_jacobians_equal_central_differences(kind):
    """J is d error / d x at x = 0 of error(exp(x) * pose), the error being obs - projection.
    Monocular: h = 1e-6, bound 1e-4 (truncation h^2 |J'''| / 6 and rounding 1e-16 * 1e3 / h, on
    entries of up to a few thousand).  Stereo: the projection rounds 1 / z to float
    (types_six_dof_expmap.cpp:300), a noise of 2^-24 * fx * x / z ~ 3e-5 px in the error, so
    h = 1e-3 and the bound 3e-5 / h + truncation = 0.1."""
    sc = M.make_scene(3, 40, kind=kind, **M.KINDS[kind])
    E = _edges(sc)
    pose = M.se3_from_tcw(sc["tcw"])
    _, Xc = M.edge_errors(E, sc["cam"], pose)
    J = M.edge_jacobians(E, sc["cam"], Xc)
    assert E.stereo.any() == (kind == "mixed")
    for stereo, h, bound in ((False, 1e-6, 1e-4), (True, 1e-3, 0.1)):
        sel = E.stereo == stereo
        if not sel.any():
            continue
        for j in range(6):
            x = np.zeros(6)
            x[j] = h
            ep, _ = M.edge_errors(E, sc["cam"], M.se3_mul(M.se3_exp(x), pose))
            em, _ = M.edge_errors(E, sc["cam"], M.se3_mul(M.se3_exp(-x), pose))
            num = (ep - em) / (2 * h)
            assert np.abs(num[sel] - J[sel, :, j]).max() < bound, (stereo, j)


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_noiseless_scene_returns_the_true_pose(kind):
    """Start 2 degrees and 5 cm off, no pixel noise: the true pose, no outliers.  The
    MapPoints are stored as float (relative 6e-8 of coordinates of a few metres, and the stereo
    projection's float 1 / z), which bounds the recovered pose's error well below 1e-5."""
    for seed in (1, 2):
        sc = M.make_scene(seed, 120, kind=kind, noise=0.0, off_deg=2.0, off_m=0.05, **M.KINDS[kind])
        r = M.run_model(sc)
        assert r["ninit"] == 120 and r["ninliers"] == 120 and not r["outlier"].any()
        assert np.abs(r["Tcw64"] - sc["tcw_true"]).max() < 1e-5
        assert np.abs(M.se3_from_tcw(sc["tcw"])[1] - sc["tcw_true"].reshape(3, 4)[:, 3]).max() > 1e-2


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_gross_outliers_are_exactly_the_flagged_ones(kind):
    sc = M.make_scene(4, 150, kind=kind, noise=0.0, outlier_frac=0.3, **M.KINDS[kind])
    r = M.run_model(sc)
    n = sc["n"]
    assert sc["gross"].sum() == 45
    assert np.array_equal(r["outlier"].astype(bool), sc["gross"][:n])
    assert r["ninliers"] == 150 - 45
    assert np.abs(r["Tcw64"] - sc["tcw_true"]).max() < 1e-5


@pytest.mark.parametrize("kind", ["mono", "mixed"])
def test_early_return_and_break(kind):
    """Optimizer.cc:428 (fewer than 3 correspondences: return 0, pose untouched) and cc:491
    (fewer than 10 edges: one round only)."""
    for ne in (2, 3, 9, 10):
        r = M.run_model(M.scene(f"{kind}-{ne}"))
        sc = M.scene(f"{kind}-{ne}")
        assert r["ninit"] == ne
        if ne < 3:
            assert r["ninliers"] == 0 and not r["trace"].any() and r["chi2"] == []
            assert r["Tcw"].tobytes() == sc["tcw"].tobytes()
        elif ne < 10:
            assert len(r["chi2"]) == 1 and r["trace"][0, 0] > 0 and not r["trace"][1:].any()
            assert r["Tcw"].tobytes() != sc["tcw"].tobytes()
        else:
            assert len(r["chi2"]) == 4 and (r["trace"][:, 0] > 0).all()


def test_each_round_restarts_from_the_input_pose_and_huber_is_dropped_in_the_last():
    """Round 1 has the same active set as round 0 when round 0 flags nothing, and starts
    from the same pose (cc:441): the same trace.  Round 3 runs without the kernel."""
    sc = M.make_scene(2, 60, kind="mono", noise=0.0, **M.KINDS["mono"])
    r = M.run_model(sc)
    assert not r["outlier"].any()
    assert r["accepts"][0] == r["accepts"][1] == r["accepts"][2]
    E = _edges(sc)
    chi2 = np.full(E.n, 100.0)
    assert (M.huber(E, chi2, True)[0] < chi2).all() and (M.huber(E, chi2, False)[0] == chi2).all()


def test_summation_orders_differ_by_rounding_only():
    sc = M.scene("mixed-257")
    vs = M.variants(sc)
    ok, why = M.guard(vs)
    assert ok, why
    assert len({v["Tcw64"].tobytes() for v in vs}) > 1          # the orders are really different sums
    assert M.pose_spread(vs) < 1e-12


def test_scene_guards_hold_for_the_small_scenes():
    """Every GPU test asserts its own scene's guard; here the small ones, on the CPU."""
    for name in M.scene_specs():
        if M.scene_specs()[name]["nedges"] <= 65:
            ok, why = M.guard(M.variants(M.scene(name)))
            assert ok, (name, why)


def test_rejected_trials_and_reentering_edges_scenes():
    r = M.run_model(M.scene("mixed-off3"))
    assert any(not a for acc in r["accepts"] for a in acc)     # the trace holds rejected trials
    for name in ("mixed-out30", "mono-out30"):
        leave, enter = M.transitions(M.run_model(M.scene(name)))
        assert leave > 0 and enter > 0, name                    # edges leave and re-enter across rounds


def test_epilogue_model():
    mp = np.array([3, -1, 9, 0, 2, 1], np.int32)
    out = np.array([1, 1, 1, 0, 0, 1], np.uint8)
    obs = np.array([0, 4, 1, 2], np.int32)
    m2, o2, nmap = M.epilogue(mp, 4, out, obs, True)
    assert m2.tolist() == [-1, -1, 9, 0, 2, -1] and o2.tolist() == [0, 1, 1, 0, 0, 0] and nmap == 1
    m3, o3, nmap3 = M.epilogue(mp, 4, out, None, False)
    assert m3.tolist() == mp.tolist() and o3.tolist() == out.tolist() and nmap3 == 2


def test_pose_optimization_arguments_rejected_without_gpu(orbx_built):
    """orbx_pose_optimization(_batch_device) check their arguments before any device call."""
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: every case fails (or returns) first
    sig = (C.c_float * 8)(*[1.0] * 8)

    def batch(**kw):
        q = L.PoseOptimizationBatch(batch=2, kps=fake, n=fake, cap=16, u_right=None, frame_mp=fake, n_mp=4,
                                    mp_pos=fake, inv_level_sigma2=sig, nlevels=8, fx=500.0, fy=500.0, cx=320.0,
                                    cy=240.0, bf=40.0, Tcw=fake, Tcw_opt=fake, outlier=fake, ninliers=fake,
                                    ninit=fake, trace=None, discard_outliers=0, mp_obs=None, nmatches_map=None)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    dev = lib.orbx_pose_optimization_batch_device
    assert dev(None, None, None) == L.ORBX_ERR_ARG
    assert dev(None, C.byref(batch()), None) == L.ORBX_ERR_ARG
    assert dev(fake, None, None) == L.ORBX_ERR_ARG
    nosig = C.POINTER(C.c_float)()
    for kw in (dict(batch=-1), dict(cap=0), dict(cap=-3), dict(n_mp=-1), dict(nlevels=0), dict(nlevels=33),
               dict(inv_level_sigma2=nosig), dict(kps=None), dict(n=None), dict(frame_mp=None), dict(mp_pos=None),
               dict(Tcw=None), dict(Tcw_opt=None), dict(outlier=None), dict(ninliers=None), dict(ninit=None),
               dict(batch=1 << 20, cap=1 << 12)):
        assert dev(fake, C.byref(batch(**kw)), None) == L.ORBX_ERR_ARG, kw
        assert lib.orbx_last_error()
    assert dev(fake, C.byref(batch(batch=0)), None) == L.ORBX_OK
    host = lib.orbx_pose_optimization
    f12 = (C.c_float * 12)()
    u8 = (C.c_uint8 * 4)()
    i4 = (C.c_int32 * 4)()
    f = (C.c_float * 12)()
    ninl = C.c_int(0)
    FP, IP, UP = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)

    def call(m=fake, keys=fake, n=4, mp=i4, pos=f, n_mp=4, sg=sig, nl=8, tin=f12, tout=f12, out=u8, res=ninl):
        return host(m, keys, n, None, C.cast(mp, IP) if mp is not None else None,
                    C.cast(pos, FP) if pos is not None else None, n_mp, sg, nl, 500.0, 500.0, 320.0, 240.0, 40.0,
                    C.cast(tin, FP) if tin is not None else None, C.cast(tout, FP) if tout is not None else None,
                    C.cast(out, UP) if out is not None else None, None, None,
                    C.byref(res) if res is not None else None)

    for kw in (dict(m=None), dict(keys=None), dict(n=-1), dict(mp=None), dict(pos=None), dict(n_mp=-1),
               dict(sg=nosig), dict(nl=0), dict(nl=40), dict(tin=None), dict(tout=None), dict(out=None),
               dict(res=None)):
        assert call(**kw) == L.ORBX_ERR_ARG, kw
