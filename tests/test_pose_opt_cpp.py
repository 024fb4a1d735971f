"""The C++ mirror orbx::Optimizer::PoseOptimization (include/orbx.hpp) through
tests/cpp/poseopt_cli.cpp: it builds with g++ against liborbx.so and, on one mixed frame,
prints the same bytes as the Python single call (and the model's flags, counts and trace)."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import pose_opt_model as M

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "poseopt_cli.cpp"
NAME = "mixed-257"


@pytest.fixture(scope="module")
def exe(tmp_path_factory, orbx_built):
    out = tmp_path_factory.mktemp("poseopt_cli") / "poseopt_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                    f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"], check=True)
    return out


def _hex(a) -> str:
    return " ".join("%08x" % int(v) for v in np.asarray(a, np.float32).reshape(-1).view(np.uint32))


def test_cpp_mirror_builds_without_gpu(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


@pytest.mark.gpu
def test_cpp_pose_optimization_prints_the_python_calls_bytes(exe, tmp_path):
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    from orbslam2commentedbyxcm_amd.optimizer import PoseOptimizer
    sc = M.scene(NAME)
    vs = M.variants(sc)
    ok, why = M.guard(vs)
    assert ok, why
    n = sc["n"]
    lines = [f"{n} {len(sc['pos'])} 8 1", _hex(sc["cam"]), _hex(sc["tcw"]), _hex(M.INV_SIGMA2)]
    for i in range(n):
        lines.append(f"{_hex(sc['keys_xy'][i])} {int(sc['octave'][i])} {_hex(sc['u_right'][i])} {int(sc['mp'][i])}")
    lines += [_hex(p) for p in sc["pos"]]
    path = tmp_path / "frame.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    keys = np.zeros(n, KEYPOINT_DTYPE)
    keys["x"], keys["y"], keys["octave"] = sc["keys_xy"][:n, 0], sc["keys_xy"][:n, 1], sc["octave"][:n]
    opt = PoseOptimizer()
    h = opt.PoseOptimization(keys, sc["u_right"][:n], sc["mp"][:n], sc["pos"], M.INV_SIGMA2, *sc["cam"], sc["tcw"])
    opt.close()
    want = [f"inliers {h['ninliers']} ninit {h['ninit']}", "tcw " + _hex(h["Tcw"]),
            "trace " + " ".join(str(int(t)) for t in h["trace"].reshape(-1)),
            "outlier " + "".join("1" if o else "0" for o in h["outlier"])]
    assert r.stdout.split("\n")[:-1] == want
    m = vs[0]
    assert h["ninliers"] == m["ninliers"] and np.array_equal(h["outlier"], m["outlier"])
    assert np.array_equal(h["trace"], m["trace"])
