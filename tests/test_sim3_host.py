"""The host side of orbx_sim3_* (include/orbx.h), without a GPU: the header declares the entry
points and the library exports them, null arguments fail with ORBX_ERR_ARG before any device
call, a machine without a GPU answers ORBX_ERR_HIP, orbx_sim3_draws is the reference's
RandomInt over the C library's rand(), the C++ mirror builds, and a Sim3Solver left alive is
closed from the exit hook."""
from __future__ import annotations

import ctypes as C
import json
import re
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["orbx_sim3_create", "orbx_sim3_destroy", "orbx_sim3_set_batch_device", "orbx_sim3_iterate_device",
         "orbx_sim3_set", "orbx_sim3_iterate", "orbx_sim3_draws"]


def test_header_declares_and_library_exports(orbx_built):
    text = (ROOT / "include" / "orbx.h").read_text()
    for ref in ["Sim3Solver.cc:37-534", "LoopClosing.cc:243-377", "Sim3Solver.h:143-144", "DUtils/Random.cpp:47-49"]:
        assert ref in text, ref
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lib = C.CDLL(str(orbx_built))
    from orbslam2commentedbyxcm_amd import _lib
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", code), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTED, n
    for field in ("draws", "fix_scale", "probability", "min_inliers", "level_sigma2", "best_iteration", "n_pairs"):
        assert re.search(rf"\b{field}\b", code), field
    hpp = (ROOT / "include" / "orbx.hpp").read_text()
    for word in ("class Sim3Solver", "SetRansacParameters", "GetEstimatedRotation", "GetEstimatedTranslation",
                 "GetEstimatedScale", "find("):
        assert word in hpp, word


def test_null_arguments_fail_before_any_device_call(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p(0x1234)
    assert lib.orbx_sim3_create(None, 1, 64, 300, C.byref(h)) == L.ORBX_ERR_ARG and not h.value
    assert lib.orbx_sim3_create(None, 1, 64, 300, None) == L.ORBX_ERR_ARG
    q, r = L.Sim3Batch(), L.Sim3Result()
    assert lib.orbx_sim3_set_batch_device(None, C.byref(q), None) == L.ORBX_ERR_ARG
    assert lib.orbx_sim3_set(None, C.byref(q)) == L.ORBX_ERR_ARG
    assert lib.orbx_sim3_iterate_device(None, 5, C.byref(r), None) == L.ORBX_ERR_ARG
    assert lib.orbx_sim3_iterate(None, 5, C.byref(r)) == L.ORBX_ERR_ARG
    assert lib.orbx_sim3_draws(None, 10, 5) == L.ORBX_ERR_ARG
    d = np.zeros((2, 3), np.int32)
    assert lib.orbx_sim3_draws(d.ctypes.data_as(C.POINTER(C.c_int32)), -1, 2) == L.ORBX_ERR_ARG
    assert lib.orbx_sim3_draws(d.ctypes.data_as(C.POINTER(C.c_int32)), 5, -1) == L.ORBX_ERR_ARG
    lib.orbx_sim3_destroy(None)   # a no-op


def test_without_a_gpu_the_solver_fails_with_err_hip(orbx_built):
    """A machine without a GPU: ORBX_ERR_HIP, as everywhere else; with one, the solver opens."""
    import torch

    from orbslam2commentedbyxcm_amd import OrbxError, _lib as L
    from orbslam2commentedbyxcm_amd.sim3 import Sim3Solver
    if torch.cuda.is_available():
        s = Sim3Solver(max_batch=1, cap=8, max_iterations=4)
        s.close()
        s.close()
        return
    with pytest.raises(OrbxError) as e:
        Sim3Solver(max_batch=1, cap=8, max_iterations=4)
    assert e.value.code == L.ORBX_ERR_HIP


@pytest.mark.parametrize("n", [3, 4, 25, 1000])
def test_draws_are_the_references_random_int(orbx_built, n):
    """int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) (DUtils/Random.cpp:47-49) on a seeded
    rand(), three per iteration with d = n, n - 1, n - 2, all iterations up front."""
    from orbslam2commentedbyxcm_amd.sim3 import reference_draws
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    RAND_MAX = 2147483647
    libc.srand(1234 + n)
    got = reference_draws(n, 50)
    libc.srand(1234 + n)
    want = np.array([[int((float(libc.rand()) / (float(RAND_MAX) + 1.0)) * (n - j)) for j in range(3)]
                     for _ in range(50)], np.int32)
    assert np.array_equal(got, want)
    assert (got >= 0).all() and all((got[:, j] < n - j).all() for j in range(3))


def test_draws_for_fewer_than_three_pairs_are_zero(orbx_built):
    from orbslam2commentedbyxcm_amd.sim3 import reference_draws
    assert not reference_draws(0, 4).any() and reference_draws(2, 4)[:, 2].tolist() == [0, 0, 0, 0]
    assert reference_draws(5, 0).shape == (0, 3)


def test_cpp_mirror_builds_and_exits_2_without_arguments(tmp_path, orbx_built):
    out = tmp_path / "sim3_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests/cpp/sim3_cli.cpp"), "-o", str(out), f"-L{lib_dir}", "-lorbx",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


FAKE = textwrap.dedent(r'''
    import ctypes as C, json, sys
    sys.path.insert(0, {root!r})
    from orbslam2commentedbyxcm_amd import _lib as L
    LOG = open({log!r}, "w")
    def rec(*ev):
        LOG.write(json.dumps([*ev, sys.is_finalizing()]) + "\n"); LOG.flush()
    class Fake:
        n = 0
        def _new(self, kind, out):
            Fake.n += 1
            out._obj.value = 0x1000 + Fake.n
            rec("create", kind, 0x1000 + Fake.n)
            return 0
        def orbx_matcher_create(self, dev, r, o, out): return self._new("matcher", out)
        def orbx_sim3_create(self, m, b, cap, its, out): return self._new("sim3", out)
        def orbx_matcher_destroy(self, h): rec("destroy", "matcher", h.value)
        def orbx_sim3_destroy(self, h): rec("destroy", "sim3", h.value)
    L._lib = Fake()
    from orbslam2commentedbyxcm_amd.matcher import ORBmatcher
    from orbslam2commentedbyxcm_amd.sim3 import Sim3Solver

    class Cycle:
        pass
    c = Cycle()
    c.me = c
    m = ORBmatcher(0.75, True)
    c.objs = [Sim3Solver(max_batch=4, cap=64, max_iterations=300), m, Sim3Solver(matcher=m, max_batch=2, cap=8)]
    freed = Sim3Solver(max_batch=1, cap=8)   # freed normally: destroyed at once, not again at exit
    del freed
    {extra}
    rec("main_done", "-", 0)
    del c, m
''')


def _run(tmp_path, extra=""):
    log = tmp_path / "log.jsonl"
    r = subprocess.run([sys.executable, "-c", FAKE.format(root=str(ROOT), log=str(log), extra=extra)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [json.loads(x) for x in log.read_text().splitlines()]


def test_a_live_solver_is_closed_at_exit(tmp_path):
    """DESIGN.md §1 "Teardown": solvers held in a cycle are closed from the exit hook, newest
    first, each handle once, the solver before the matcher it borrows, never during
    finalisation."""
    ev = _run(tmp_path)
    created = [(e[1], e[2]) for e in ev if e[0] == "create"]
    destroyed = [(e[1], e[2]) for e in ev if e[0] == "destroy"]
    assert sorted(created) == sorted(destroyed) and len(set(destroyed)) == len(destroyed)
    assert not any(e[3] for e in ev), "a handle was released during interpreter finalisation"
    done = [i for i, e in enumerate(ev) if e[0] == "main_done"][0]
    assert [e[1] for e in ev[:done] if e[0] == "destroy"] == ["sim3", "matcher"]   # `freed`: its solver, then its matcher
    tail = [e[1] for e in ev[done + 1:]]
    # the borrowing solver, then the first solver and its own matcher, then the shared matcher
    # (registered first): it outlives the solver that borrows it
    assert tail == ["sim3", "sim3", "matcher", "matcher"]
    assert ev[-1][2] == [h for k, h in created if k == "matcher"][0]


def test_close_is_idempotent(tmp_path):
    ev = _run(tmp_path, extra="c.objs[0].close(); c.objs[0].close(); c.objs[2].close(); c.objs[2].close()")
    destroyed = [e[2] for e in ev if e[0] == "destroy"]
    assert len(set(destroyed)) == len(destroyed) == sum(e[0] == "create" for e in ev)
