"""tests/pnp_model.py and the host side of orbx_pnp_* without a GPU: csrc/orbx_epnp.h compiled
for the host is bit-equal to the model's Jacobi variant, the model recovers the ground truth on
clean scenes, the guards hold for every named scene, each quirk of PnPsolver.cc has its known
answer, the header declares the entry points and the library exports them, null arguments fail
before any device call, and orbx_pnp_draws is the reference's RandomInt."""
from __future__ import annotations

import ctypes as C
import re
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pnp_model as M
import pnp_scenes as S

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["orbx_pnp_create", "orbx_pnp_destroy", "orbx_pnp_set_batch_device", "orbx_pnp_iterate_device", "orbx_pnp_set",
         "orbx_pnp_iterate", "orbx_pnp_draws"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/orbx_epnp.h behind tests/cpp/epnp_host.cpp, compiled for the host without contraction."""
    out = tmp_path_factory.mktemp("epnp_host") / "epnp_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                    f"-I{ROOT / 'orbslam2commentedbyxcm_amd' / 'csrc'}", str(ROOT / "tests/cpp/epnp_host.cpp"), "-o",
                    str(out)], check=True)

    def run(mode, data):
        return subprocess.run([str(out), mode], input=data, capture_output=True, check=True, timeout=60).stdout
    return run


def _points(seed, n, noise=0.0, coplanar=False, repeat=False):
    rng = np.random.default_rng(seed)
    K = [float(k) for k in S.K]
    P = rng.uniform(-2, 2, (n, 3)) + [0, 0, 6]
    if coplanar:
        P[:, 2] = 6.0
    if repeat:
        P[1] = P[0]
    R, t = S._rodrigues(rng.normal(size=3) * 0.2), rng.normal(size=3) * 0.3
    P = P.astype(np.float32).astype(np.float64)
    Xc = P @ R.T + t
    u = K[0] * Xc[:, 0] / Xc[:, 2] + K[2] + rng.normal(size=n) * noise
    v = K[1] * Xc[:, 1] / Xc[:, 2] + K[3] + rng.normal(size=n) * noise
    return P, np.stack([u, v], 1).astype(np.float32).astype(np.float64), K, R, t


@pytest.mark.parametrize("seed,n,kw", [(1, 4, {}), (2, 4, {}), (3, 4, dict(noise=0.5)), (4, 4, dict(coplanar=True)),
                                       (5, 4, dict(repeat=True)), (6, 5, {}), (7, 30, dict(noise=0.5)),
                                       (8, 100, dict(noise=0.5)), (9, 12, dict(coplanar=True))])
def test_host_compute_pose_is_bit_equal_to_the_model(host, seed, n, kw):
    """Minimal sets (clean, noisy, coplanar, with a repeated 3D point) and Refine-sized sets."""
    P, U, K, _, _ = _points(seed, n, **kw)
    R, t, err = M.compute_pose(P, U, K)
    got = np.frombuffer(host("pose", struct.pack("<i4d", n, *K) + P.tobytes() + U.tobytes()), np.float64)
    want = np.concatenate([R.reshape(-1), t, [err]])
    assert got.tobytes() == want.tobytes() or (np.array_equal(np.isnan(got), np.isnan(want)) and
                                               np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)]))


@pytest.mark.parametrize("rows,n", [(3, 3), (6, 3), (6, 4), (6, 5), (12, 12)])
def test_host_jacobi_is_bit_equal_to_the_model(host, rows, n):
    rng = np.random.default_rng(rows * 100 + n)
    a = rng.standard_normal((rows, n))
    if rows == n:
        a = a.T @ a                      # symmetric PSD
        if n == 12:
            a = a[:, :8] @ a[:, :8].T    # with a 4-fold null space
    B, V = M.hestenes(a)
    got = np.frombuffer(host("jacobi", struct.pack("<ii", rows, n) + np.ascontiguousarray(a).tobytes()), np.float64)
    assert got[:rows * n].tobytes() == B.tobytes() and got[rows * n:].tobytes() == V.tobytes()
    assert np.abs(V.T @ V - np.eye(n)).max() < 1e-14


def test_host_qr_solve_is_bit_equal_and_returns_early_on_a_zero_pivot_column(host):
    rng = np.random.default_rng(7)
    a, b, x0 = rng.standard_normal((6, 4)), rng.standard_normal(6), rng.standard_normal(4)
    got = np.frombuffer(host("qr", a.tobytes() + b.tobytes() + x0.tobytes()), np.float64)
    want = M.qr_solve(a, b, x0)
    assert got.tobytes() == want.tobytes()
    assert np.abs(want - np.linalg.lstsq(a, b, rcond=None)[0]).max() < 1e-12
    # cc:1242-1247 never looks at the last row: a column that is zero above it is "singular",
    # and X is left as it was (cc:1250-1255)
    a2 = a.copy()
    a2[:5, 1] = 0.0
    a2[0, 0], a2[1:, 0] = 1.0, 0.0       # so that column 1 keeps its zeros after the first reflection
    got = np.frombuffer(host("qr", a2.tobytes() + b.tobytes() + x0.tobytes()), np.float64)
    assert got.tobytes() == x0.tobytes() == M.qr_solve(a2, b, x0).tobytes()


def test_host_check_inliers_is_bit_equal_to_the_model(host):
    """Points spread around the threshold, float products that differ from the fused ones."""
    rng = np.random.default_rng(11)
    P, U, K, R, t = _points(11, 4000, noise=2.5)
    p3, p2 = P.astype(np.float32), U.astype(np.float32)
    max_err = (S.SIGMA2[rng.integers(0, 8, len(P))] * np.float32(5.991)).astype(np.float32)
    want = M.check_inliers(R, t, K, p3, p2, max_err)
    pts = np.concatenate([p3, p2, max_err[:, None]], 1).astype(np.float32)
    data = R.tobytes() + t.tobytes() + struct.pack("<4di", *K, len(P)) + pts.tobytes()
    got = np.frombuffer(host("inlier", data), np.uint8).astype(bool)
    assert np.array_equal(got, want) and 0.1 < want.mean() < 0.9


def test_model_recovers_the_ground_truth_on_clean_scenes():
    for name in ("blind_100", "blind_63", "blind_11"):
        sc, o = S.scene(name), S.guard_for(name)["outs"][-1]
        assert o["found"] and o["refined"]
        T = o["Tcw"].reshape(3, 4)
        assert np.abs(T[:, :3] - sc["R"]).max() < 1e-5 and np.abs(T[:, 3] - sc["t"]).max() < 1e-5
        assert set(np.nonzero(o["inliers"])[0]) == set(sc["inl_slots"])
        assert np.array_equal(o["frame_mp"][o["inliers"] == 1], sc["matches"][o["inliers"] == 1])
        assert (o["frame_mp"][o["inliers"] == 0] == -1).all()
    P, U, K, R, t = _points(21, 50)
    Rm, tm, err = M.compute_pose(P, U, K)
    assert np.abs(Rm - R).max() < 1e-6 and np.abs(tm - t).max() < 1e-5 and err < 1e-3


@pytest.mark.parametrize("name", list(S.SCENES))
def test_guard_holds(name):
    """A scene whose guard fails is a failure, not a skip: seeds are chosen until it holds."""
    g = S.guard_for(name)
    assert len(g["outs"]) >= 1
    if S.scene(name)["blind"]:
        assert len(g["family_b"]) == len(M.CONVENTIONS) >= 6


def test_setransacparameters_quirks():
    # exponent 3, not 4: eps 0.5 -> log(0.01) / log(1 - 0.125) = 34.5 -> 35 (with 4: 72)
    assert M.ransac_parameters(100, 0.99, 10, 300, 4, 0.5) == (50, 35)
    # int(N * eps) is a float product truncated; eps raised to minInliers / N
    assert M.ransac_parameters(11, 0.99, 10, 300, 4, 0.5) == (10, 4)
    assert M.ransac_parameters(63, 0.99, 10, 300, 4, 0.5)[0] == 31
    # minInliers == N: one iteration; minSet bounds it from below
    assert M.ransac_parameters(10, 0.99, 10, 300, 4, 0.5) == (10, 1)
    assert M.ransac_parameters(4, 0.99, 2, 300, 4, 0.5) == (4, 1)
    assert M.ransac_parameters(3, 0.99, 10, 300, 4, 0.5)[0] == 10      # N < minInliers: no iteration
    # the cap clamps
    assert M.ransac_parameters(1000, 0.99, 10, 20, 4, 0.011)[1] == 20


def test_iterate_quirks():
    # the loop is an OR (cc:226): all_10 has a cap of 1, yet the first iterate(5) runs 5 iterations,
    # and Refine's strict > (cc:364) fails with 10 of 10 inliers: found unrefined at the cap
    o = S.guard_for("all_10")["outs"][0]
    assert (o["max_its_used"], o["iterations"], o["found"], o["refined"], o["no_more"]) == (1, 5, 1, 0, 1)
    assert o["n_inliers"] == 10 == o["min_inliers_used"]
    m = S.model_for("all_10")
    m.iterate(5)
    tied = [k for k, c in m.counts.items() if c == 10]
    assert len(tied) >= 2 and m.best_iteration == tied[0]        # a tie keeps the earlier iteration
    assert m.iterate(3)["iterations"] == 8                        # a later call runs n more, beyond the cap
    # Refine runs on the best set, not the current one: after a success the next qualifying
    # iteration returns the same refined pose although its own hypothesis is another
    g = S.guard_for("cont_100")["outs"]
    assert all(o["found"] and o["refined"] for o in g)
    assert all(o["Tcw"].tobytes() == g[0]["Tcw"].tobytes() for o in g)
    assert g[1]["iterations"] > g[0]["iterations"] and g[-1]["best_iteration"] == g[0]["best_iteration"]
    # out of draws, draws out of range
    o = S.guard_for("nodraws_100")["outs"]
    assert [x["status"] for x in o] == [0, 0, M.STATUS_NO_DRAWS] and o[2]["no_more"] and o[2]["iterations"] == 10
    o = S.guard_for("baddraw_64")["outs"][-1]
    assert o["status"] == M.STATUS_BAD_DRAW and o["found"] and o["iterations"] > 3
    # mvMaxError is a float product (cc:189)
    m = S.model_for("blind_11")
    assert m.max_error.dtype == np.float32
    assert np.array_equal(m.max_error, m.sigma2 * np.float32(5.991))


def test_header_declares_and_library_exports(orbx_built):
    text = (ROOT / "include" / "orbx.h").read_text()
    for ref in ["PnPsolver.cc:80-1345", "Tracking.cc:1511-1684", "cc:226", "DUtils/Random.cpp:47-49"]:
        assert ref in text, ref
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lib = C.CDLL(str(orbx_built))
    from orbslam2commentedbyxcm_amd import _lib
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", code), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTED, n
    hpp = (ROOT / "include" / "orbx.hpp").read_text()
    for word in ("class PnPsolver", "SetRansacParameters", "frameMP", "find("):
        assert word in hpp, word


def test_null_arguments_fail_before_any_device_call(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p(0x1234)
    assert lib.orbx_pnp_create(None, 1, 64, 300, C.byref(h)) == L.ORBX_ERR_ARG and not h.value
    assert lib.orbx_pnp_create(None, 1, 64, 300, None) == L.ORBX_ERR_ARG
    q, r = L.PnpBatch(), L.PnpResult()
    assert lib.orbx_pnp_set_batch_device(None, C.byref(q), None) == L.ORBX_ERR_ARG
    assert lib.orbx_pnp_set(None, C.byref(q)) == L.ORBX_ERR_ARG
    assert lib.orbx_pnp_iterate_device(None, 5, C.byref(r), None) == L.ORBX_ERR_ARG
    assert lib.orbx_pnp_iterate(None, 5, C.byref(r)) == L.ORBX_ERR_ARG
    assert lib.orbx_pnp_draws(None, 10, 5) == L.ORBX_ERR_ARG
    lib.orbx_pnp_destroy(None)   # a no-op


def test_without_a_gpu_the_solver_fails_with_err_hip(orbx_built):
    import torch

    from orbslam2commentedbyxcm_amd import OrbxError, PnPsolver, _lib as L
    if torch.cuda.is_available():
        s = PnPsolver(max_batch=1, cap=8, max_draws=4)
        s.close()
        s.close()
        return
    with pytest.raises(OrbxError) as e:
        PnPsolver(max_batch=1, cap=8, max_draws=4)
    assert e.value.code == L.ORBX_ERR_HIP


@pytest.mark.parametrize("n", [4, 5, 25, 1000])
def test_draws_are_the_references_random_int(orbx_built, n):
    from orbslam2commentedbyxcm_amd.pnp import reference_draws
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    RAND_MAX = 2147483647
    libc.srand(4321 + n)
    got = reference_draws(n, 50)
    libc.srand(4321 + n)
    want = np.array([[int((float(libc.rand()) / (float(RAND_MAX) + 1.0)) * (n - j)) for j in range(4)]
                     for _ in range(50)], np.int32)
    assert np.array_equal(got, want)
    assert all(M.select4(d, n) is not None and len(set(M.select4(d, n))) == 4 for d in got)
    assert not reference_draws(0, 3).any() and reference_draws(5, 0).shape == (0, 4)
