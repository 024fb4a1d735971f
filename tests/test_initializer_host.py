"""The host side of orbx_initializer_* (include/orbx.h), without a GPU: the header declares the
entry points and the library exports them, the ctypes layouts match the header, null arguments
fail with ORBX_ERR_ARG before any device call, a machine without a GPU answers ORBX_ERR_HIP,
orbx_initializer_sets is Initializer.cc:103-123 over the C library's rand(), the C++ mirror
builds, and an Initializer left alive is closed from the exit hook."""
from __future__ import annotations

import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import initializer_model as M

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["orbx_initializer_create", "orbx_initializer_destroy", "orbx_initializer_initialize_device",
         "orbx_initializer_initialize", "orbx_initializer_sets"]


def _code():
    return re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "orbx.h").read_text(), flags=re.S)


def test_header_declares_and_library_exports(orbx_built):
    text = (ROOT / "include" / "orbx.h").read_text()
    for ref in ["Initializer.cc:64-165", "cc:1215-1379", "cc:103-123", "DUtils/Random.cpp:47-49", "DESIGN.md §4.19"]:
        assert ref in text, ref
    code = _code()
    lib = C.CDLL(str(orbx_built))
    from orbslam2commentedbyxcm_amd import _lib
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", code), n
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTED, n
    for word in ("ORBX_INIT_MAX_ITERATIONS", "ORBX_INIT_STATUS_BAD_SET", "ORBX_INIT_STATUS_TOO_FEW"):
        assert re.search(rf"#define {word}\b", code), word
    hpp = (ROOT / "include" / "orbx.hpp").read_text()
    for word in ("class Initializer", "bool Initialize(", "vbTriangulated", "orbx_initializer_sets"):
        assert word in hpp, word
    import orbslam2commentedbyxcm_amd as P
    assert "Initializer" in P.__all__ and P.Initializer.__name__ == "Initializer"


def _struct_fields(name):
    """The member names of `typedef struct { ... } name;` in declaration order."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", _code(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"[\s\*]", "", d).split("[")[0].split(" ")[-1] for d in
                    re.sub(r"^(const\s+)?\w+\s*\**\s*", "", decl, count=1).split(",")]
    return out


def test_ctypes_layouts_match_the_header(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    assert [f[0] for f in L.InitializerBatch._fields_] == _struct_fields("orbx_initializer_batch")
    assert [f[0] for f in L.InitializerResult._fields_] == _struct_fields("orbx_initializer_result")
    assert list(L.INITIALIZER_RESULT_FIELDS) == _struct_fields("orbx_initializer_result")
    # sizes as a C compiler lays them out
    src = '#include <stdio.h>\n#include "orbx.h"\nint main(void) { printf("%zu %zu %zu\\n", ' \
          "sizeof(orbx_initializer_batch), sizeof(orbx_initializer_result), " \
          "__builtin_offsetof(orbx_initializer_batch, sets)); return 0; }\n"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.c").write_text(src)
        subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(Path(d) / "s.c"), "-o", str(Path(d) / "s")], check=True)
        sizes = subprocess.run([str(Path(d) / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in sizes] == [C.sizeof(L.InitializerBatch), C.sizeof(L.InitializerResult),
                                       L.InitializerBatch.sets.offset]
    code = _code()
    assert int(re.search(r"#define ORBX_INIT_MAX_ITERATIONS (\d+)", code).group(1)) == L.ORBX_INIT_MAX_ITERATIONS
    assert int(re.search(r"#define ORBX_INIT_STATUS_BAD_SET (\d+)", code).group(1)) == L.ORBX_INIT_STATUS_BAD_SET == \
        M.STATUS_BAD_SET
    assert int(re.search(r"#define ORBX_INIT_STATUS_TOO_FEW (\d+)", code).group(1)) == L.ORBX_INIT_STATUS_TOO_FEW == \
        M.STATUS_TOO_FEW


def test_null_arguments_fail_before_any_device_call(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p(0x1234)
    assert lib.orbx_initializer_create(None, 1, 64, 200, C.byref(h)) == L.ORBX_ERR_ARG and not h.value
    assert lib.orbx_initializer_create(None, 1, 64, 200, None) == L.ORBX_ERR_ARG
    q, r = L.InitializerBatch(), L.InitializerResult()
    assert lib.orbx_initializer_initialize_device(None, C.byref(q), C.byref(r), None) == L.ORBX_ERR_ARG
    assert lib.orbx_initializer_initialize(None, C.byref(q), C.byref(r)) == L.ORBX_ERR_ARG
    assert lib.orbx_initializer_sets(None, 10, 5) == L.ORBX_ERR_ARG
    d = np.zeros((2, 8), np.int32)
    assert lib.orbx_initializer_sets(d.ctypes.data_as(C.POINTER(C.c_int32)), -1, 2) == L.ORBX_ERR_ARG
    assert lib.orbx_initializer_sets(d.ctypes.data_as(C.POINTER(C.c_int32)), 50, -1) == L.ORBX_ERR_ARG
    lib.orbx_initializer_destroy(None)   # a no-op


def test_without_a_gpu_the_solver_fails_with_err_hip(orbx_built):
    """A machine without a GPU: ORBX_ERR_HIP, as everywhere else; with one, the solver opens."""
    import torch

    from orbslam2commentedbyxcm_amd import Initializer, OrbxError, _lib as L
    if torch.cuda.is_available():
        s = Initializer(max_batch=1, kcap=8, max_iterations=4)
        s.close()
        s.close()
        return
    with pytest.raises(OrbxError) as e:
        Initializer(max_batch=1, kcap=8, max_iterations=4)
    assert e.value.code == L.ORBX_ERR_HIP


@pytest.mark.parametrize("n", [8, 9, 100, 1000])
def test_sets_are_the_references(orbx_built, n):
    """cc:103-123 restated over ctypes' srand / rand: srand(0), then per iteration eight
    RandomInt(0, size - 1) draws, each removed by a swap with the back and a pop."""
    from orbslam2commentedbyxcm_amd.initializer import reference_sets
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand(99)                       # whatever state the process is in: the call seeds itself
    got = reference_sets(n, 40)
    want = M.sets_restated(n, 40, libc)
    assert np.array_equal(got, want)
    assert (got >= 0).all() and (got < n).all()
    assert all(len(set(row.tolist())) == 8 for row in got)
    assert np.array_equal(reference_sets(n, 40), got)   # srand(0) on every call


def test_sets_for_fewer_than_eight_matches_are_zero(orbx_built):
    from orbslam2commentedbyxcm_amd.initializer import reference_sets
    assert not reference_sets(7, 4).any() and not reference_sets(0, 4).any()
    assert reference_sets(50, 0).shape == (0, 8)


def test_cpp_mirror_builds_and_exits_2_without_arguments(tmp_path, orbx_built):
    out = tmp_path / "initializer_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests/cpp/initializer_cli.cpp"), "-o", str(out), f"-L{lib_dir}", "-lorbx",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


FAKE = r'''
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
    def orbx_initializer_create(self, m, b, kcap, its, out): return self._new("initializer", out)
    def orbx_matcher_destroy(self, h): rec("destroy", "matcher", h.value)
    def orbx_initializer_destroy(self, h): rec("destroy", "initializer", h.value)
L._lib = Fake()
from orbslam2commentedbyxcm_amd.matcher import ORBmatcher
from orbslam2commentedbyxcm_amd.initializer import Initializer

class Cycle:
    pass
c = Cycle()
c.me = c
m = ORBmatcher(0.9, True)
c.objs = [Initializer(max_batch=4, kcap=64), m, Initializer(max_batch=2, kcap=8, matcher=m)]
freed = Initializer(max_batch=1, kcap=8)   # freed normally: destroyed at once, not again at exit
freed.close(); freed.close()
del freed
rec("main_done", "-", 0)
del c, m
'''


def test_a_live_initializer_is_closed_at_exit(tmp_path):
    """DESIGN.md §1 "Teardown": initializers held in a cycle are closed from the exit hook, newest
    first, each handle once, the one that borrows a matcher before that matcher, never during
    finalisation; close() is idempotent."""
    import json
    import sys
    log = tmp_path / "log.jsonl"
    r = subprocess.run([sys.executable, "-c", FAKE.format(root=str(ROOT), log=str(log))], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    ev = [json.loads(x) for x in log.read_text().splitlines()]
    created = [(e[1], e[2]) for e in ev if e[0] == "create"]
    destroyed = [(e[1], e[2]) for e in ev if e[0] == "destroy"]
    assert sorted(created) == sorted(destroyed) and len(set(destroyed)) == len(destroyed)
    assert not any(e[3] for e in ev), "a handle was released during interpreter finalisation"
    done = [i for i, e in enumerate(ev) if e[0] == "main_done"][0]
    assert [e[1] for e in ev[:done] if e[0] == "destroy"] == ["initializer", "matcher"]   # `freed`
    assert [e[1] for e in ev[done + 1:]] == ["initializer", "initializer", "matcher", "matcher"]
    assert ev[-1][2] == [h for k, h in created if k == "matcher"][0]
