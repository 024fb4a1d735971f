"""orbx_sim3_* on the GPU against tests/sim3_model.py.

Scenes (sim3_model.SEEDS): TUM1 intrinsics (one with K1 != K2), points 1-8 m away, pixel noise
1 px x 1.2^octave, 30 % outliers unless the scene says otherwise, octaves 0-7, true rotation
0.3 rad, scale 1.3 or fixed; N in {0, 2, 3, 4, 5, 19, 20, 21, 63, 64, 65, 255, 256, 257, 1000}
valid pairs in rows of cap 1024 with skipped slots interleaved (-1, negative and outside the
table, in either id array); min_inliers 20 (3 for N <= 19), 300 iterations unless the scene
says otherwise.

Every comparison first asserts its scene's guard (sim3_model.guard_for): over every iteration
the test walks, the model's variants -- numpy's eigh, the model's Jacobi, the eigenvector
negated, reversed sums, ang and Rodrigues moved by one ulp -- agree on every flag and count,
and every err / threshold is further from 1 than 1000 x the largest relative difference
between them.  Then flags, counts, found, no_more, iterations, best_iteration, n_pairs and
status are equal to the model's, NaN stands where the model's NaN stands, and T12, R, t, s are
within TOL.

Tolerance of T12 / R / t / s: tests/sim3_spread.py measures the largest entry difference
between the variants over these scenes: 1.95e-13.  8 x that, 1.56e-12, is far below float
resolution, so the floor decides: 2 float32 ulps of the entry's magnitude.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SPREAD = 1.95e-13           # python tests/sim3_spread.py
TOL = 8 * SPREAD            # floor: 2 float32 ulps of the entry
INT_KEYS = ("found", "no_more", "n_inliers", "best_inliers", "best_iteration", "iterations", "n_pairs", "status")
F32_KEYS = (("T12", 16), ("best_R", 9), ("best_t", 3), ("best_s", 1))
FILL = 7                    # prefill of the flag rows: entries beyond n1 keep it


def guarded(name):
    ok, why, _ = M.guard_for(name)
    assert ok, (name, why)
    return M.scene(name)


@pytest.fixture(scope="module")
def solver(orbx_built):
    from orbslam2commentedbyxcm_amd.sim3 import Sim3Solver
    s = Sim3Solver(max_batch=16, cap=1024, max_iterations=300)
    yield s
    s.close()


def run_batch(solver, scenes, schedule):
    """set_batch_device on the packed scenes, then the schedule's calls (ints, or "find");
    returns one dict of host arrays per call."""
    import torch
    P = M.pack(scenes)
    B, cap = len(scenes), P["cap"]
    dev = torch.device("cuda", solver.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sc = scenes[0]
    stream = torch.cuda.Stream(dev)   # the prefills, the uploads and the library's kernels in one order
    calls = []
    with torch.cuda.stream(stream):
        solver.set_batch_device(t(P["n1"]), t(P["mp1"]), t(P["mp2"]), t(P["oct1"]), t(P["oct2"]), t(P["pos"]),
                                t(P["Tcw1"]), t(P["Tcw2"]), sc["level_sigma2"], sc["K1"], sc["K2"], t(P["draws"]),
                                fix_scale=sc["fix_scale"], probability=sc["probability"],
                                min_inliers=sc["min_inliers"], max_iterations=sc["max_iterations"], stream=stream)
        for c in schedule:
            o = {k: torch.full((B,), -9, dtype=torch.int32, device=dev) for k in INT_KEYS}
            o["inliers"] = torch.full((B, cap), FILL, dtype=torch.uint8, device=dev)
            for k, n in F32_KEYS:
                o[k] = torch.full((B, n) if k != "best_s" else (B,), -5.0, dtype=torch.float32, device=dev)
            solver.iterate_batch_device(sc["max_iterations"] if c == "find" else int(c), stream=stream, **o)
            calls.append(o)
    stream.synchronize()
    return [{k: v.cpu().numpy() for k, v in o.items()} for o in calls]


def one(res, b):
    """Candidate b's outputs of one call."""
    return {k: v[b] for k, v in res.items()}


def assert_close(got, want64, what):
    """NaN where the model has NaN; else within 8 x the variants' spread, floor 2 float32 ulps."""
    got = np.asarray(got, np.float32).reshape(-1)
    want64 = np.asarray(want64, np.float64).reshape(-1)
    want32 = want64.astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), (what, got.tolist(), want64.tolist())
    fin = ~np.isnan(want64)
    tol = np.maximum(TOL, 2 * np.spacing(np.abs(want32[fin])).astype(np.float64))
    diff = np.abs(got[fin].astype(np.float64) - want32[fin].astype(np.float64))
    assert (diff <= tol).all(), (what, float(diff.max()), got.tolist(), want32.tolist())
    return float(diff.max()) if fin.any() else 0.0


def assert_call(got, sc, r, what):
    """One candidate's outputs of one call against the model's result r."""
    n1 = int(sc["n1"])
    for k in INT_KEYS:
        assert int(got[k]) == int(r[k]), (what, k, int(got[k]), int(r[k]))
    assert np.array_equal(got["inliers"][:n1], r["inliers"]), what
    assert (got["inliers"][n1:] == FILL).all(), (what, "flags beyond n1 were written")
    d = assert_close(got["T12"], r["T12"], what + " T12")
    d = max(d, assert_close(got["best_R"], r["best_R"], what + " R"))
    d = max(d, assert_close(got["best_t"], r["best_t"], what + " t"))
    d = max(d, assert_close(got["best_s"], [r["best_s"]], what + " s"))
    print(f"{what}: found {int(got['found'])} no_more {int(got['no_more'])} inliers {int(got['n_inliers'])} best "
          f"{int(got['best_inliers'])} at {int(got['best_iteration'])} iterations {int(got['iterations'])} "
          f"max |d| {d:.3g}")


def same_bytes(a, b, what, n1):
    for k in a:
        x, y = a[k], b[k]
        if k == "inliers":
            x, y = x[:n1], y[:n1]
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, k)


def rounds(solver, sc, step):
    """LoopClosing::ComputeSim3's schedule on the device: as many iterate(step) as the model
    needs until the candidate returns or has no more, in one stream, read back at the end."""
    want = M.rounds_of(sc, step)
    return run_batch(solver, [sc], [step] * len(want)), want


@pytest.mark.parametrize("name", M.PARITY_SCENES)
def test_scene_parity(solver, name):
    sc = guarded(name)
    got, want = rounds(solver, sc, 5)
    for i, (g, r) in enumerate(zip(got, want)):
        assert_call(one(g, 0), sc, r, f"{name} round {i}")
    assert want[-1]["found"] or want[-1]["no_more"]


@pytest.mark.parametrize("name", M.CHUNK_SCENES)
def test_chunking_gives_equal_bytes(solver, name):
    """iterate(5) rounds, iterate(1) rounds and find(): the same bytes wherever they can be
    compared -- after every fifth single iteration, and at the end."""
    sc = guarded(name)
    n1 = int(sc["n1"])
    five, want5 = rounds(solver, sc, 5)
    ones, _ = rounds(solver, sc, 1)
    whole = run_batch(solver, [sc], ["find"])[0]
    for i, r in enumerate(want5):
        assert_call(one(five[i], 0), sc, r, f"{name} iterate(5) round {i}")
    for i in range(len(five) - 1):                      # neither has returned: 5 (i + 1) iterations walked
        same_bytes(one(five[i], 0), one(ones[5 * (i + 1) - 1], 0), f"{name} after {5 * (i + 1)} iterations", n1)
    same_bytes(one(five[-1], 0), one(ones[-1], 0), f"{name} iterate(5) against iterate(1) at the end", n1)
    same_bytes(one(five[-1], 0), one(whole, 0), f"{name} iterate(5) against find()", n1)


def test_batch_of_16_equals_each_alone(solver):
    scenes = [guarded(n) for n in M.BATCH_SCENES]
    assert len(scenes) == 16
    schedule = [5, 5, 40]
    batch = run_batch(solver, scenes, schedule)
    models = [M.run(sc, schedule)[0] for sc in scenes]
    for b, sc in enumerate(scenes):
        alone = run_batch(solver, [sc], schedule)
        for c in range(len(schedule)):
            same_bytes(one(batch[c], b), one(alone[c], 0), f"{M.BATCH_SCENES[b]} call {c}: batch against alone",
                       int(sc["n1"]))
            if models[b][c]["iterations"] <= M.guard_for(M.BATCH_SCENES[b])[2]["upto"]:
                assert_call(one(batch[c], b), sc, models[b][c], f"{M.BATCH_SCENES[b]} call {c}")


def test_continuing_after_a_return(solver):
    """mnBestInliers persists: the next returning iteration needs inl >= the best so far."""
    sc = guarded("continue-300")
    schedule = M.SCHEDULES["continue-300"]
    got = run_batch(solver, [sc], schedule)
    want = M.run(sc, schedule)[0]
    for i, (g, r) in enumerate(zip(got, want)):
        assert_call(one(g, 0), sc, r, f"continue-300 call {i}")
    assert want[0]["found"] and any(r["found"] for r in want[1:])
    for a, b in zip(got, got[1:]):
        if int(b["found"][0]):
            assert int(b["n_inliers"][0]) >= int(a["best_inliers"][0])


def test_tie_goes_to_the_later_iteration(solver):
    sc = guarded("tie-64")
    got = run_batch(solver, [sc], [1] * 8)
    want = M.run(sc, [1] * 8)[0]
    for i, (g, r) in enumerate(zip(got, want)):
        assert_call(one(g, 0), sc, r, f"tie-64 iteration {i}")
    best = [int(g["best_iteration"][0]) for g in got]
    assert best[4] < 5 and best[5] == 5 and best[6] == 6 and best[7] == 6
    assert int(got[4]["best_inliers"][0]) == int(got[6]["best_inliers"][0]) > 0


def test_identical_point_sets_are_nan(solver):
    sc = guarded("nan-50")
    got, want = rounds(solver, sc, 5)
    for i, (g, r) in enumerate(zip(got, want)):
        assert_call(one(g, 0), sc, r, f"nan-50 round {i}")
    last = one(got[-1], 0)
    assert int(last["no_more"]) == 1 and int(last["found"]) == 0 and int(last["best_inliers"]) == 0
    assert int(last["iterations"]) == sc["max_iterations"] and int(last["best_iteration"]) == sc["max_iterations"] - 1
    assert np.isnan(last["best_R"]).all() and np.isnan(last["best_t"]).all() and np.isnan(last["best_s"])


def test_a_bad_draw_costs_its_iteration_only(solver):
    sc = guarded("bad-64")
    got = run_batch(solver, [sc], [1] * 8)
    want = M.run(sc, [1] * 8)[0]
    for i, (g, r) in enumerate(zip(got, want)):
        assert_call(one(g, 0), sc, r, f"bad-64 iteration {i}")
    status = [int(g["status"][0]) for g in got]
    assert status == [0] + [M.STATUS_BAD_DRAW] * 7
    whole = run_batch(solver, [sc], ["find"])[0]
    same_bytes(one(got[-1], 0), one(whole, 0), "bad-64 iterate(1) against find()", int(sc["n1"]))


def test_set_resets_the_state(solver):
    sc = guarded("first-64")
    a = run_batch(solver, [sc], ["find"])[0]
    b = run_batch(solver, [sc], ["find"])[0]
    same_bytes(one(a, 0), one(b, 0), "first-64 set twice", int(sc["n1"]))
    assert int(a["iterations"][0]) == 1 and int(a["found"][0]) == 1


def test_argument_errors_with_a_live_solver(solver):
    import ctypes as C

    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)   # never dereferenced: every case fails first
    sig = (C.c_float * 8)(*[float(s) for s in M.LEVEL_SIGMA2])
    K = (C.c_float * 4)(*M.TUM1)

    def batch(**kw):
        q = L.Sim3Batch(batch=1, cap=64, n1=fake, mp1=fake, mp2=fake, oct1=fake, oct2=fake, n_mp=10, mp_pos=fake,
                        Tcw1=fake, Tcw2=fake, level_sigma2=sig, nlevels=8, K1=K, K2=K, fix_scale=0, probability=0.99,
                        min_inliers=20, max_iterations=300, draws=fake)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for kw in (dict(batch=17), dict(batch=-1), dict(cap=0), dict(cap=1025), dict(n_mp=-1), dict(nlevels=0),
               dict(nlevels=33), dict(min_inliers=-1), dict(max_iterations=0), dict(max_iterations=301),
               dict(probability=0.0), dict(probability=1.0), dict(n1=None), dict(mp1=None), dict(mp2=None),
               dict(oct1=None), dict(oct2=None), dict(mp_pos=None), dict(Tcw1=None), dict(Tcw2=None), dict(draws=None),
               dict(level_sigma2=None), dict(K1=None), dict(K2=None)):
        q = batch(**kw)
        assert lib.orbx_sim3_set_batch_device(solver._h, C.byref(q), None) == L.ORBX_ERR_ARG, kw
        assert lib.orbx_sim3_set(solver._h, C.byref(q)) == L.ORBX_ERR_ARG, kw
    assert lib.orbx_sim3_set(solver._h, C.byref(batch(batch=2))) == L.ORBX_ERR_ARG
    r = L.Sim3Result()
    assert lib.orbx_sim3_iterate_device(solver._h, -1, C.byref(r), None) == L.ORBX_ERR_ARG
    assert lib.orbx_sim3_iterate_device(solver._h, 5, None, None) == L.ORBX_ERR_ARG
    h = C.c_void_p()
    assert lib.orbx_sim3_create(solver._m, 1, 64, L.ORBX_SIM3_MAX_ITERATIONS + 1, C.byref(h)) == L.ORBX_ERR_ARG
    assert lib.orbx_sim3_create(solver._m, 0, 64, 300, C.byref(h)) == L.ORBX_ERR_ARG and not h.value


# ---- the mirrors ---------------------------------------------------------------------------------
MIRROR = "n257-free"
MIRROR_SCHEDULE = (3, 5, "find")


def host_calls(sc, schedule):
    from orbslam2commentedbyxcm_amd.sim3 import Sim3Solver
    s = Sim3Solver(sc["mp1"][:sc["n1"]], sc["mp2"][:sc["n1"]], sc["oct1"][:sc["n1"]], sc["oct2"][:sc["n1"]],
                   sc["mp_pos"], sc["Tcw1"], sc["Tcw2"], sc["level_sigma2"], sc["K1"], sc["K2"], sc["fix_scale"],
                   draws=sc["draws"], max_iterations=sc["max_iterations"])
    s.SetRansacParameters(sc["probability"], sc["min_inliers"], sc["max_iterations"])
    out = []
    for c in schedule:
        out.append(s.iterate_host(sc["max_iterations"] if c == "find" else c))
    # the reference's surface on the same object
    s.SetRansacParameters(sc["probability"], sc["min_inliers"], sc["max_iterations"])
    T, inl, n = s.find()
    R, t, scale = s.GetEstimatedRotation(), s.GetEstimatedTranslation(), s.GetEstimatedScale()
    us = s.last_call_us()
    s.close()
    s.close()
    return out, (T, inl, n, R, t, scale, us)


def test_the_single_host_call_gives_the_batch_forms_bytes(solver):
    sc = guarded(MIRROR)
    n1 = int(sc["n1"])
    batch = run_batch(solver, [sc], MIRROR_SCHEDULE)
    host, (T, inl, n, R, t, scale, us) = host_calls(sc, MIRROR_SCHEDULE)
    for c, (b, h) in enumerate(zip(batch, host)):
        b0 = one(b, 0)
        for k in INT_KEYS:
            assert int(b0[k]) == int(h[k][0]), (c, k)
        for k, _ in F32_KEYS:
            assert np.asarray(b0[k], np.float32).tobytes() == np.asarray(h[k], np.float32).tobytes(), (c, k)
        assert np.array_equal(b0["inliers"][:n1], h["inliers"]), c
    whole = one(run_batch(solver, [sc], ["find"])[0], 0)
    assert T is not None and T.astype(np.float32).tobytes() == whole["T12"].tobytes()
    assert n == int(whole["n_inliers"]) and np.array_equal(inl, whole["inliers"][:n1].astype(bool))
    assert R.tobytes() == whole["best_R"].tobytes() and t.tobytes() == whole["best_t"].tobytes()
    assert np.float32(scale).tobytes() == np.float32(whole["best_s"]).tobytes()
    assert us > 0.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory, orbx_built):
    out = tmp_path_factory.mktemp("sim3_cli") / "sim3_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/sim3_cli.cpp"),
                    "-o", str(out), f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"], check=True)
    return out


def test_the_cpp_mirror_prints_the_batch_forms_bytes(solver, exe, tmp_path):
    sc = guarded(MIRROR)
    n1 = int(sc["n1"])
    batch = run_batch(solver, [sc], MIRROR_SCHEDULE)
    path = tmp_path / "candidate.txt"
    path.write_text(M.cli_text(sc))
    r = subprocess.run([str(exe), str(path), *[str(c) for c in MIRROR_SCHEDULE]], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    want = []
    for c, b in zip(MIRROR_SCHEDULE, batch):
        b0 = one(b, 0)
        b0["inliers"] = b0["inliers"][:n1]
        lines = M.cli_lines(c, b0)
        if c == "find":     # find() has no bNoMore: the mirror prints 0
            lines[0] = lines[0].replace(f"no_more {int(b0['no_more'])}", "no_more 0")
        want += lines
    assert r.stdout.split("\n")[:-1] == want
