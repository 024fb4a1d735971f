"""orbx_initializer_* on the GPU against tests/initializer_model.py.

Scenes (initializer_model.SPECS): TUM1 intrinsics, sigma 1, 0.5 px noise and 20 % outliers
unless the scene says otherwise; N in {8, 9, 63, 64, 65, 100, 255, 256, 257, 1000} matched
slots, each as a general and a planar scene, interleaved with -1, negative and >= n2 entries
in rows of kcap 1024; and the outcome scenes ok_general (F, ok), ok_plane (H, ok),
low_parallax, pure_rotation, few_good, d_ratio (d1/d2 < 1.00001), too_few (N < 8), bad_set,
one_column (zero deviation).  200 iterations, except n8_* (1), n9_* (4 hand-picked sets),
d_ratio (1: without translation every F scores alike) and too_few (8).

Every comparison first asserts its scene's guard (initializer_model.guard_for).  Then every
integer output and flag equals the model's, NaN / 0 stand where the model's stand, and floats
are within max(8 x the scene's own spread between the model's variants, 2 float32 ulps of the
entry); H21 / F21 are compared after scaling to unit Frobenius norm with the largest entry
positive (scale and sign are free in the reference too; a float-rounded matrix normalised in
double is within 2^-23 relative of the normalised double, which is below 2 ulps).

tests/initializer_spread.py over these scenes, largest per field: SH / SF relative 1.63e-10
(pure_rotation), H21 3.83e-13, F21 6.97e-4 (d_ratio: the epipolar geometry of an identity motion
is noise; the next largest is 1.81e-10, pure_rotation), R21 1.29e-12, t21 2.36e-11, p3d 1.64e-9,
parallax 6.26e-10.  Apart from d_ratio's F21 the floor of 2 ulps decides nearly everywhere.  On
an MI355X the largest difference to the model's double result was 0.60 ulp (H21).
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import initializer_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
KCAP = M.KCAP
INT_KEYS = ("ok", "model", "n_matches", "best_it_H", "best_it_F", "n_inliers_H", "n_inliers_F", "best_good",
            "second_good", "n_similar", "status")
FLAG_KEYS = ("inliers_H", "inliers_F", "triangulated")
FILL_U8, FILL_I32, FILL_F32 = 7, -9, -5.0


def guarded(name):
    ok, why = M.guard_for(name)
    assert ok, (name, why)
    return M.scene(name)


@pytest.fixture(scope="module")
def solver(orbx_built):
    from orbslam2commentedbyxcm_amd.initializer import Initializer
    s = Initializer(max_batch=16, kcap=KCAP, max_iterations=200)
    yield s
    s.close()


def pack(scenes, sets=None):
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    B = len(scenes)
    its = len(scenes[0]["sets"] if sets is None else sets[0])
    P = dict(n1=np.zeros(B, np.int32), n2=np.zeros(B, np.int32), keys1=np.zeros((B, KCAP), KEYPOINT_DTYPE),
             keys2=np.zeros((B, KCAP), KEYPOINT_DTYPE), m12=np.full((B, KCAP), 3, np.int32),
             sets=np.zeros((B, its, 8), np.int32))
    P["keys1"]["x"] = P["keys1"]["y"] = P["keys2"]["x"] = P["keys2"]["y"] = 1e9   # never read beyond n1 / n2
    for b, sc in enumerate(scenes):
        n1, n2 = len(sc["keys1"]), len(sc["keys2"])
        P["n1"][b], P["n2"][b] = n1, n2
        P["keys1"][b, :n1] = M.keypoints(sc["keys1"])
        P["keys2"][b, :n2] = M.keypoints(sc["keys2"])
        P["m12"][b, :n1] = sc["matches12"]
        P["sets"][b] = sc["sets"] if sets is None else sets[b]
    return P


def run_batch(solver, scenes, sets=None):
    """initialize_batch_device on the packed scenes: every output as host arrays, prefilled."""
    import torch
    from orbslam2commentedbyxcm_amd.initializer import RESULT_LAYOUT
    P = pack(scenes, sets)
    B = len(scenes)
    dev = torch.device("cuda", solver.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kb = lambda a: t(a.view(np.uint8).reshape(B, KCAP, 28))  # noqa: E731
    stream = torch.cuda.Stream(dev)   # the prefills, the uploads and the library's kernels in one order
    with torch.cuda.stream(stream):
        o = {}
        for k, (dt, shape) in RESULT_LAYOUT.items():
            shp = (B,) + tuple(KCAP if d == "kcap" else d for d in shape)
            tdt, fill = {"i4": (torch.int32, FILL_I32), "f4": (torch.float32, FILL_F32), "u1": (torch.uint8, FILL_U8)}[dt]
            o[k] = torch.full(shp, fill, dtype=tdt, device=dev)
        solver.initialize_batch_device(t(P["n1"]), t(P["n2"]), kb(P["keys1"]), kb(P["keys2"]), t(P["m12"]), M.K4,
                                       t(P["sets"]), stream=stream, **o)
    stream.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


_ALONE = {}


def alone(solver, name):
    """The scene run as a batch of one (cached: the reference bytes of the other tests)."""
    if name not in _ALONE:
        r = run_batch(solver, [M.scene(name)])
        _ALONE[name] = {k: v[0] for k, v in r.items()}
    return _ALONE[name]


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    return np.spacing(np.maximum(x, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def close(got, want, spread, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    fin = ~np.isnan(want)
    tol = np.maximum(8.0 * spread, 2.0 * ulp32(want))
    err = np.abs(got - want)
    assert (err[fin] <= tol[fin]).all(), (what, float(err[fin].max()), got[fin][np.argmax(err[fin])],
                                         want[fin][np.argmax(err[fin])])


def compare(name, got):
    sc = guarded(name)
    vs = M.scene_variants(name)
    want, sp = vs[0], M.spreads(vs)
    n1 = len(sc["keys1"])
    for k in INT_KEYS:
        assert int(got[k]) == int(want[k]), (name, k, int(got[k]), want[k])
    for k in FLAG_KEYS:
        assert np.array_equal(got[k][:n1], want[k]), (name, k)
        assert (got[k][n1:] == FILL_U8).all(), (name, k, "written at or beyond n1")
    assert (got["p3d"][n1:] == np.float32(FILL_F32)).all(), (name, "p3d written at or beyond n1")
    for k in ("SH", "SF"):
        close(got[k], want[k], sp["S"] * abs(want[k]), (name, k))
    close(got["RH"], want["RH"], 2.0 * sp["S"], (name, "RH"))
    for k in ("H21", "F21"):
        close(M.unit(got[k]), M.unit(want[k]), sp[k], (name, k))
    for k in ("R21", "t21", "p3d", "parallax"):
        close(got[k][:n1] if k == "p3d" else got[k], want[k], sp[k], (name, k))
    if not want["ok"]:
        assert not got["R21"].any() and not got["t21"].any() and not got["p3d"][:n1].any()


@pytest.mark.parametrize("name", M.ALL_SCENES)
def test_scene_parity(solver, name):
    compare(name, alone(solver, name))


MIXED = ("n63_gen", "n64_plane", "n65_gen", "n100_plane", "n255_gen", "n256_plane", "n257_gen", "n1000_gen",
         "n1000_plane", "ok_general", "ok_plane", "low_parallax", "pure_rotation", "few_good", "bad_set", "one_column")


def test_a_mixed_batch_gives_each_scenes_bytes(solver):
    assert len(MIXED) == 16
    r = run_batch(solver, [M.scene(n) for n in MIXED])
    for b, n in enumerate(MIXED):
        a = alone(solver, n)
        for k in r:
            assert r[k][b].tobytes() == a[k].tobytes(), (n, k)


@pytest.mark.parametrize("name", ("ok_general", "ok_plane", "n9_gen", "too_few", "bad_set"))
def test_the_host_form_gives_the_batch_forms_bytes(solver, name):
    sc = M.scene(name)
    a = alone(solver, name)
    n1 = len(sc["keys1"])
    o = solver.initialize_host(M.keypoints(sc["keys1"]), M.keypoints(sc["keys2"]), sc["matches12"], M.K4, sc["sets"],
                               max_iterations=len(sc["sets"]))
    for k, v in o.items():
        want = a[k][:n1] if np.ndim(a[k]) and a[k].shape[0] == KCAP else a[k]
        assert np.asarray(v).reshape(-1).tobytes() == np.asarray(want).reshape(-1).tobytes(), (name, k)
    assert solver.last_call_us() > 0.0
    if len(sc["sets"]) == 200:   # the reference's surface on the same arrays
        ok, R, t, p3d, tri = solver.Initialize(sc["keys1"], sc["keys2"], sc["matches12"], M.K4, sc["sets"])
        assert ok == bool(a["ok"]) and (R is None) == (not ok)
        assert np.array_equal(tri, a["triangulated"][:n1].astype(bool)) and p3d.tobytes() == a["p3d"][:n1].tobytes()


def test_two_calls_on_one_solver_give_the_same_bytes(solver):
    first = {k: v.copy() for k, v in alone(solver, "ok_plane").items()}
    run_batch(solver, [M.scene("n1000_gen"), M.scene("one_column")])   # other state in the workspace
    again = run_batch(solver, [M.scene("ok_plane")])
    for k, v in first.items():
        assert again[k][0].tobytes() == v.tobytes(), k


def test_a_tie_keeps_the_earlier_iteration(solver):
    """currentScore > score is strict (cc:235, 303): the winning set given a second time keeps
    the first index, wherever the copy stands."""
    sc = guarded("ok_general")
    a = alone(solver, "ok_general")
    wh, wf = int(a["best_it_H"]), int(a["best_it_F"])
    later = sc["sets"].copy()
    later[199] = sc["sets"][wf]
    later[198] = sc["sets"][wh]
    r = run_batch(solver, [sc], sets=[later])
    assert (int(r["best_it_H"][0]), int(r["best_it_F"][0])) == (wh, wf)
    earlier = sc["sets"].copy()
    earlier[0] = sc["sets"][wf]
    earlier[1] = sc["sets"][wh]
    r = run_batch(solver, [sc], sets=[earlier])
    assert (int(r["best_it_H"][0]), int(r["best_it_F"][0])) == (1, 0)
    for k in ("SH", "SF", "inliers_H", "inliers_F", "R21", "t21", "p3d", "triangulated", "ok"):
        assert r[k][0].tobytes() == a[k].tobytes(), k


def test_a_bad_set_costs_only_its_iteration(solver):
    sc = guarded("bad_set")
    a = alone(solver, "bad_set")
    assert int(a["status"]) == M.STATUS_BAD_SET
    mended = sc["sets"].copy()   # the bad iterations replaced by sets that lose: same outcome, no status bit
    for it in (3, 7, 11):
        mended[it] = sc["sets"][12]
    r = run_batch(solver, [sc], sets=[mended])
    assert int(r["status"][0]) == 0
    for k in a:
        if k != "status":
            assert r[k][0].tobytes() == a[k].tobytes(), k


def test_too_few_matches_set_their_status_bit(solver):
    a = alone(solver, "too_few")
    assert int(a["status"]) == M.STATUS_TOO_FEW and int(a["ok"]) == 0 and int(a["n_matches"]) == 5
    assert int(a["best_it_H"]) == -1 and int(a["best_it_F"]) == -1 and np.isnan(a["RH"])
    assert not a["H21"].any() and not a["F21"].any() and not a["R21"].any()


def test_argument_errors_with_a_live_solver(solver):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    q, r = L.InitializerBatch(), L.InitializerResult()
    k = np.array(M.K4, np.float32)
    q.batch, q.kcap, q.sigma, q.max_iterations = 1, KCAP, 1.0, 200
    q.K = k.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.orbx_initializer_initialize_device(solver._h, C.byref(q), C.byref(r), None) == L.ORBX_ERR_ARG  # null buffers
    assert lib.orbx_initializer_initialize_device(solver._h, None, C.byref(r), None) == L.ORBX_ERR_ARG
    assert lib.orbx_initializer_initialize_device(solver._h, C.byref(q), None, None) == L.ORBX_ERR_ARG
    q.batch = 0
    assert lib.orbx_initializer_initialize_device(solver._h, C.byref(q), C.byref(r), None) == L.ORBX_OK   # nothing to do
    for field, bad in (("batch", 17), ("batch", -1), ("kcap", KCAP + 1), ("kcap", 0), ("max_iterations", 201),
                       ("max_iterations", 0), ("sigma", 0.0)):
        q2 = L.InitializerBatch.from_buffer_copy(q)
        setattr(q2, field, bad)
        assert lib.orbx_initializer_initialize_device(solver._h, C.byref(q2), C.byref(r), None) == L.ORBX_ERR_ARG, field
    q.K = None
    assert lib.orbx_initializer_initialize_device(solver._h, C.byref(q), C.byref(r), None) == L.ORBX_ERR_ARG
    q.batch, q.K = 2, k.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.orbx_initializer_initialize(solver._h, C.byref(q), C.byref(r)) == L.ORBX_ERR_ARG   # one pair only
    h = C.c_void_p()
    assert lib.orbx_initializer_create(solver._m, 1, 8193, 200, C.byref(h)) == L.ORBX_ERR_ARG
    assert lib.orbx_initializer_create(solver._m, 1, 64, L.ORBX_INIT_MAX_ITERATIONS + 1, C.byref(h)) == L.ORBX_ERR_ARG
    assert lib.orbx_initializer_create(solver._m, 0, 64, 200, C.byref(h)) == L.ORBX_ERR_ARG


def test_the_cpp_mirror_prints_the_batch_forms_bytes(solver, tmp_path, orbx_built):
    """tests/cpp/initializer_cli.cpp (orbx::Initializer of include/orbx.hpp) on ok_general: the
    hex of R21, t21, the flags and the points equals the batch form's."""
    sc = M.scene("ok_general")
    a = alone(solver, "ok_general")
    n1, n2 = len(sc["keys1"]), len(sc["keys2"])
    exe = tmp_path / "initializer_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests/cpp/initializer_cli.cpp"), "-o", str(exe), f"-L{lib_dir}", "-lorbx",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    f = tmp_path / "scene.bin"
    with open(f, "wb") as fh:
        fh.write(np.array([n1, n2, len(sc["sets"])], np.int32).tobytes())
        fh.write(np.asarray(M.K4, np.float32).tobytes())
        fh.write(M.keypoints(sc["keys1"]).tobytes())
        fh.write(M.keypoints(sc["keys2"]).tobytes())
        fh.write(np.asarray(sc["matches12"], np.int32).tobytes())
        fh.write(np.asarray(sc["sets"], np.int32).tobytes())
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert int(lines["ok"]) == int(a["ok"]) == 1
    assert lines["R21"].strip() == a["R21"].tobytes().hex()
    assert lines["t21"].strip() == a["t21"].tobytes().hex()
    assert lines["p3d"].strip() == a["p3d"][:n1].tobytes().hex()
    assert lines["triangulated"].strip() == a["triangulated"][:n1].tobytes().hex()


def test_search_for_initialization_feeds_the_initializer(solver):
    """The monocular chain on the device: two synthetic frames of a known motion, matched by
    orbx_search_for_initialization (window 100, as Tracking calls it), its matches12 fed straight
    in with the reference's sets.  ok is 1, R21 is within 1.5 degrees of the truth and t21 within
    5 degrees of its direction: the bounds of tests/test_initializer_model.py, where the model
    measures 0.59 and 1.86 degrees on ok_general (the same geometry and noise)."""
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    from orbslam2commentedbyxcm_amd.matcher import FrameView, ORBmatcher
    sc = M.make_scene(4242, N=400, outliers=0.0)
    rng = np.random.default_rng(4242)
    n1 = len(sc["keys1"])
    desc1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    truth12 = np.where((sc["matches12"] >= 0) & (sc["matches12"] < n1), sc["matches12"], -1)
    desc2 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)     # unmatched keypoints of frame 2: unrelated
    seen = truth12 >= 0
    bits = np.unpackbits(desc1[seen], axis=1)
    bits ^= (rng.random(bits.shape) < 0.02).astype(np.uint8)
    desc2[truth12[seen]] = np.packbits(bits, axis=1)
    sf = (1.2 ** np.arange(8)).astype(np.float32)

    def view(xy, desc):
        keys = np.zeros(len(xy), KEYPOINT_DTYPE)
        keys["x"], keys["y"], keys["size"], keys["angle"], keys["class_id"] = xy[:, 0], xy[:, 1], 31, 45.0, -1
        return FrameView(keys=keys, desc=desc, fx=float(M.FX), fy=float(M.FY), cx=float(M.CX), cy=float(M.CY),
                         max_x=640.0, max_y=480.0, scale_factors=sf, level_sigma2=sf * sf,
                         Tcw=np.eye(4, dtype=np.float32))

    A, B = view(sc["keys1"], desc1), view(sc["keys2"], desc2)
    m = ORBmatcher(0.9, True)
    prev = np.ascontiguousarray(sc["keys1"], np.float32).copy()
    nm, m12 = m.SearchForInitialization(A, B, prev, 100)
    assert nm >= 100 and (m12[seen] == truth12[seen]).mean() > 0.9
    o = solver.initialize_host(A.keys, B.keys, m12, M.K4)     # the reference's sets for N = nm
    assert int(o["ok"][0]) == 1 and int(o["n_matches"][0]) == nm
    R = o["R21"].reshape(3, 3).astype(np.float64)
    ang = np.degrees(np.arccos(np.clip((np.trace(R @ sc["truth"]["R"].T) - 1.0) / 2.0, -1.0, 1.0)))
    assert ang < 1.5, ang
    t = o["t21"].astype(np.float64)
    assert np.degrees(np.arccos(np.clip(t @ sc["truth"]["t"], -1.0, 1.0))) < 5.0
