"""The C++ mirror orbx::Optimizer::OptimizeEssentialGraph (include/orbx.hpp) through
tests/cpp/essgraph_cli.cpp: it builds with g++ against liborbx.so and, on ring-9, prints the
same bytes as the Python single call."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import essential_graph_model as M

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "essgraph_cli.cpp"
NAME = "ring-9"


@pytest.fixture(scope="module")
def exe(tmp_path_factory, orbx_built):
    out = tmp_path_factory.mktemp("essgraph_cli") / "essgraph_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                    f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"], check=True)
    return out


def _hex(a) -> str:
    return " ".join("%08x" % int(v) for v in np.asarray(a, np.float32).reshape(-1).view(np.uint32))


def _hex64(a) -> str:
    return " ".join("%016x" % int(v) for v in np.asarray(a, np.float64).reshape(-1).view(np.uint64))


def test_cpp_mirror_builds_without_gpu(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


@pytest.mark.gpu
def test_cpp_essential_graph_prints_the_python_calls_bytes(exe, tmp_path):
    from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer
    sc = M.scene(NAME)
    K, E, P = len(sc["Tcw"]), len(sc["edge_v"]), len(sc["pos"])
    lines = [f"{K} {len(sc['corr_S'])} {E} {P} {sc['loop']} {sc['fix_scale']}"]
    lines += [f"{int(sc['corr'][k])} {_hex(sc['Tcw'][k])}" for k in range(K)]
    lines += [_hex64(s) for s in sc["corr_S"]]
    lines += [f"{int(i)} {int(j)} {int(k)}" for (i, j), k in zip(sc["edge_v"], sc["edge_kind"])]
    lines += [f"{int(sc['pt_ref'][p])} {_hex(sc['pos'][p])}" for p in range(P)]
    path = tmp_path / "graph.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr

    opt = EssentialGraphOptimizer()
    h = opt.OptimizeEssentialGraph(sc["Tcw"], sc["corr"], sc["corr_S"], sc["loop"], sc["edge_v"], sc["edge_kind"],
                                   sc["pos"], sc["pt_ref"], sc["fix_scale"])
    opt.close()
    want = [f"status {h['status']} trace {int(h['trace'][0])} {int(h['trace'][1])}", "Tcw " + _hex(h["Tcw"]),
            "pos " + _hex(h["pos"]), "Scw " + _hex64(h["Scw"]), "chi2 " + _hex64(h["chi2"])]
    assert r.stdout.split("\n")[:-1] == want
    assert h["status"] == 0 and h["trace"][0] > 0
