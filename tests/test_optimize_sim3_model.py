"""tests/optimize_sim3_model.py against closed forms and Optimizer::OptimizeSim3's schedule
(no GPU), and the argument checks of orbx_optimize_sim3(_batch_device) through ctypes."""
from __future__ import annotations

import ctypes as C

import numpy as np

import optimize_sim3_model as M


def _skew(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def _jproj(p, K):
    fx, fy = K[0], K[1]
    x, y, z = p
    return np.array([[fx / z, 0.0, -fx * x / (z * z)], [0.0, fy / z, -fy * y / (z * z)]])


def test_numeric_jacobian_against_the_closed_form():
    """With the update Sim3(x) * S: d(exp(x) p)/dx = [-[p]x | I | p] at x = 0, so the forward
    edge has de/dx = -Jproj(p) [-[p]x | I | p] at p = S.map(X2), and the inverse edge, whose
    point is q = S^-1.map(exp(-x) X1), has de/dx = Jproj(q) A [-[X1]x | I | X1] with A = (1 / s)
    R^T
    (the linear part of S^-1).
    Bound: an error evaluation is about 30 operations on quantities of magnitude up to M (the
    pixel coordinates, obs and fx x / z + cx), each rounding by at most 2^-53 M; the difference
    of two evaluations is divided by 2 delta, so rounding contributes at most 32 x 2^-53 M /
    1e-9 (3.6e-6 M).  Truncation: the central difference's delta^2 f''' / 6 and the probes'
    second-order terms, of order delta^2 |J| x the point's magnitude: below 1e-15 here, taken
    as 1e-12 |J|."""
    for name in ("n65-free", "k1k2-150-free", "n64-fix"):
        sc = M.scene(name)
        E = M.Pairs(sc)
        S = M.sim3_from_rts(sc["R12"], sc["t12"], sc["s12"])
        J = M.numeric_jacobians(E, S, M.probe_increments(sc["fix_scale"]))
        Si = M.sim3_inverse(S)   # the quaternion is not unit: its linear map, column by column
        A = Si[2] * np.stack([M.quat_rotate(Si[0], e) for e in np.eye(3)], axis=1)
        worst = 0.0
        for i in range(E.n):
            p = M.sim3_map(S, E.X2[i:i + 1])[0]
            q = M.sim3_map(M.sim3_inverse(S), E.X1[i:i + 1])[0]
            G12 = np.concatenate([-_skew(p), np.eye(3), p[:, None]], axis=1)
            G21 = np.concatenate([-_skew(E.X1[i]), np.eye(3), E.X1[i][:, None]], axis=1)
            want = np.stack([-_jproj(p, E.K1) @ G12, _jproj(q, E.K2) @ A @ G21])
            if sc["fix_scale"]:
                want[:, :, 6] = 0.0
                assert (J[i, :, :, 6] == 0.0).all()          # the two probes coincide: exactly 0
            mag = max(np.abs(E.obs1[i]).max(), np.abs(E.obs2[i]).max(), 700.0)
            bound = 32 * 2.0 ** -53 * mag / 1e-9 + 1e-12 * np.abs(want)
            diff = np.abs(J[i] - want)
            assert (diff <= bound).all(), (name, i, float(diff.max()), float(bound.min()))
            worst = max(worst, float(diff.max()))
        print(name, "largest |J_num - J_closed|:", worst)


def _clean(seed, fix, **kw):
    return M.make_scene(seed, 80, fix_scale=fix, noise=0.0, **kw)


def test_noiseless_scene_returns_the_true_sim3():
    for fix in (False, True):
        sc = _clean(3, fix)
        r = M.optimize_sim3(sc)
        assert r["ncorr"] == 80 and r["nbad"] == 0 and r["ninliers"] == 80
        R, t, s = r["S64"][:9].reshape(3, 3), r["S64"][9:12], r["S64"][12]
        # the MapPoints are float: 8 m x 2^-24 of position error, seen through a 2-8 m lever
        assert np.abs(R - sc["R_true"]).max() < 1e-5
        assert np.abs(t - sc["t_true"]).max() < 2e-5
        assert abs(s - sc["s_true"]) < 1e-5
        assert np.array_equal(r["matches12"], np.asarray(sc["matches12"][:sc["n1"]], np.int32))
        if fix:
            assert r["s12"] == sc["s12"] == np.float32(1.0) and s == 1.0   # exactly the input's
            for H in r["H0"]:                                              # row 6 holds only lambda
                assert (H[6] == 0.0).all() and (H[:, 6] == 0.0).all()
        else:
            assert all(H[6, 6] > 0 for H in r["H0"])


def test_gross_outliers_are_exactly_the_entries_set_to_minus_one():
    for fix in (False, True):
        sc = M.make_scene(11, 120, fix_scale=fix, noise=0.3, nout=15)
        r = M.optimize_sim3(sc)
        n1 = sc["n1"]
        before = np.asarray(sc["matches12"][:n1], np.int32)
        turned = (r["matches12"] == -1) & (before != -1)
        assert np.array_equal(turned, sc["gross"][:n1])
        assert r["ninliers"] == 120 - 15 and r["nbad"] <= 15
        same = ~turned
        assert np.array_equal(r["matches12"][same], before[same])


def test_fewer_than_ten_pairs_left_returns_zero():
    sc = M.scene("n10-free")                      # 10 clean pairs optimise
    r = M.optimize_sim3(sc)
    assert r["ncorr"] == 10 and r["nbad"] == 0 and r["trace"][1, 0] > 0 and r["ninliers"] == 10
    assert not np.array_equal(r["R12"], sc["R12"])
    for name in ("n10-out1-free", "n10-out1-fix"):   # 10 pairs, one gross: 9 left, return 0
        sc = M.scene(name)
        r = M.optimize_sim3(sc)
        n1 = sc["n1"]
        assert r["ncorr"] == 10 and r["nbad"] == 1 and r["ninliers"] == 0
        assert r["trace"][0, 0] == 5 and (r["trace"][1] == 0).all()
        assert r["R12"].tobytes() == sc["R12"].tobytes() and r["t12"].tobytes() == sc["t12"].tobytes()
        assert r["s12"] == sc["s12"]
        turned = (r["matches12"] == -1) & (np.asarray(sc["matches12"][:n1]) != -1)
        assert np.array_equal(turned, sc["gross"][:n1]) and turned.sum() == 1
    sc = M.scene("n9-free")                       # 9 pairs: optimised once, then 9 < 10
    r = M.optimize_sim3(sc)
    assert r["ncorr"] == 9 and r["trace"][0, 0] > 0 and (r["trace"][1] == 0).all() and r["ninliers"] == 0
    assert r["R12"].tobytes() == sc["R12"].tobytes()


def test_zero_pairs():
    for name in ("n0-free", "n0-fix"):
        sc = M.scene(name)
        assert sc["n1"] > 0                       # slots, every one with a hole
        r = M.optimize_sim3(sc)
        assert r["ncorr"] == 0 and r["nbad"] == 0 and r["ninliers"] == 0 and not r["trace"].any()
        assert np.array_equal(r["matches12"], np.asarray(sc["matches12"][:sc["n1"]], np.int32))
        assert r["R12"].tobytes() == sc["R12"].tobytes() and r["s12"] == sc["s12"]


def test_more_iterations_after_a_rejection(monkeypatch):
    asked = []
    real = M.optimize

    def spy(E, S, active, max_its, *a):
        asked.append((max_its, int(active.sum())))
        return real(E, S, active, max_its, *a)

    monkeypatch.setattr(M, "optimize", spy)
    r = M.optimize_sim3(M.scene("clean-150-free"))
    assert r["nbad"] == 0 and asked == [(5, 150), (5, 150)]
    asked.clear()
    r = M.optimize_sim3(M.scene("out-150-free"))
    assert r["nbad"] > 0 and asked == [(5, 150), (10, 150 - r["nbad"])]


def test_every_variant_passes_the_guard_on_a_test_scene():
    vs = M.scene_variants("n65-free")
    assert len(vs) == 12
    ok, why = M.guard(vs)
    assert ok, why
    assert 0.0 < M.s12_spread(vs) < 1e-6
    # a chi2 at rounding distance from th2 fails it
    a = vs[0]
    bad = [dict(v, chi2=[c.copy() for c in v["chi2"]]) for v in vs]
    for k, v in enumerate(bad):
        v["chi2"][0][0, 0] = float(np.float32(M.TH2)) + 1e-9 * (k + 1)
    assert not M.guard(bad)[0] and a["chi2"][0][0, 0] != bad[0]["chi2"][0][0, 0]


def test_argument_checks_need_no_gpu(orbx_built):
    """orbx_optimize_sim3_batch_device / orbx_optimize_sim3 reject bad arguments before any
    device call; an empty batch is a no-op."""
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)   # never dereferenced: every case fails (or returns) first
    sig = (C.c_float * 8)(*[1.0] * 8)
    K = (C.c_float * 4)(500.0, 500.0, 320.0, 240.0)
    one = (C.c_int32 * 1)(4)

    def batch(**kw):
        q = L.OptimizeSim3Batch(batch=2, cap1=16, n1=fake, kps1=fake, mp1=fake, matches12=fake, idx2=fake, cap2=16,
                                n2=fake, kps2=fake, n_mp=5, mp_pos=fake, Tcw1=fake, Tcw2=fake, inv_level_sigma2_1=sig,
                                inv_level_sigma2_2=sig, nlevels=8, K1=K, K2=K, R12=fake, t12=fake, s12=fake, th2=10.0,
                                fix_scale=0, R12_opt=fake, t12_opt=fake, s12_opt=fake, ninliers=None, ncorr=None,
                                nbad=None, trace=None)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    dev = lib.orbx_optimize_sim3_batch_device
    assert dev(None, C.byref(batch()), None) == L.ORBX_ERR_ARG
    assert dev(fake, None, None) == L.ORBX_ERR_ARG
    nullf = C.POINTER(C.c_float)()
    for kw in (dict(batch=-1), dict(cap1=0), dict(cap2=-3), dict(n_mp=-1), dict(nlevels=0), dict(nlevels=33),
               dict(inv_level_sigma2_1=nullf), dict(inv_level_sigma2_2=nullf), dict(K1=nullf), dict(K2=nullf),
               dict(th2=-1.0), dict(th2=float("nan")), dict(n1=None), dict(kps1=None), dict(mp1=None),
               dict(matches12=None), dict(idx2=None), dict(n2=None), dict(kps2=None), dict(mp_pos=None),
               dict(Tcw1=None), dict(Tcw2=None), dict(R12=None), dict(t12=None), dict(s12=None), dict(R12_opt=None),
               dict(t12_opt=None), dict(s12_opt=None), dict(batch=1 << 20, cap1=1 << 11),
               dict(batch=1 << 20, cap2=1 << 11)):
        assert dev(fake, C.byref(batch(**kw)), None) == L.ORBX_ERR_ARG, kw
    assert dev(fake, C.byref(batch(batch=0)), None) == L.ORBX_OK
    assert dev(fake, C.byref(batch(batch=0, n1=None, kps1=None)), None) == L.ORBX_OK
    host = lib.orbx_optimize_sim3
    assert host(None, C.byref(batch(batch=1)), ) == L.ORBX_ERR_ARG
    assert host(fake, None) == L.ORBX_ERR_ARG
    assert host(fake, C.byref(batch())) == L.ORBX_ERR_ARG                      # batch 2
    assert host(fake, C.byref(batch(batch=0))) == L.ORBX_ERR_ARG
    assert host(fake, C.byref(batch(batch=1, kps1=None))) == L.ORBX_ERR_ARG
    n = C.cast(one, C.c_void_p)
    assert host(fake, C.byref(batch(batch=1, n1=n, n2=n, cap1=3))) == L.ORBX_ERR_ARG   # n1 4 > cap1 3
    assert host(fake, C.byref(batch(batch=1, n1=n, n2=n, cap2=3))) == L.ORBX_ERR_ARG
    one[0] = -1
    assert host(fake, C.byref(batch(batch=1, n1=n, n2=n))) == L.ORBX_ERR_ARG
    assert b"count" in lib.orbx_last_error()
