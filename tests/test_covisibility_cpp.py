"""The C++ mirror orbx::Covisibility (include/orbx.hpp) through tests/cpp/covis_cli.cpp: it
builds with g++ against liborbx.so and, on one scene, prints the model's lists."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import covisibility_model as M

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "covis_cli.cpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory, orbx_built):
    out = tmp_path_factory.mktemp("covis_cli") / "covis_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                    f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"], check=True)
    return out


def test_cpp_mirror_builds_without_gpu(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


@pytest.mark.gpu
def test_cpp_covisibility_prints_the_models_lists(exe, tmp_path):
    kf_mp, kf_n, kf_bad, mp_bad = M.scene(**M.GPU_SCENES["band24"])
    K, cap = kf_mp.shape
    lines = [f"{K} {cap} {len(mp_bad)} 64"]
    lines += [f"{int(kf_n[k])} {int(kf_bad[k])} " + " ".join(str(int(p)) for p in kf_mp[k]) for k in range(K)]
    lines.append(" ".join(str(int(b)) for b in mp_bad))
    g = M.Graph(K, 64)
    g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
    for k in (3, 4):
        g.update_connections(k)
        lines.append(f"u 1 {k}")
    rest = [k for k in range(K) if k not in (3, 4)]
    for k in rest:
        g.update_connections(k)
    lines.append(f"u {len(rest)} " + " ".join(map(str, rest)))
    g.erase_keyframe(7)
    kf_bad = kf_bad.copy()
    kf_bad[7] = 1
    g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
    g.update_connections(8)
    lines += ["e 7", "b 7", "r", "u 1 8", "p"]
    path = tmp_path / "map.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = []
    for k in range(K):
        want.append(f"{k}:" + "".join(f" {kf}:{w}" for kf, w in zip(g.ordered[k], g.weights[k])))
        want.append(f"best10 {k}:" + "".join(f" {kf}" for kf in g.best_covisibles(k, 10)))
        want.append(f"w15 {k}:" + "".join(f" {kf}" for kf in g.covisibles_by_weight(k, 15)))
    want.append("parent " + " ".join(str(p) for p in g.parent))
    want.append("first " + " ".join(str(int(b)) for b in g.first))
    assert r.stdout.splitlines() == want
    assert any(len(o) > 1 for o in g.ordered) and np.sum(np.array(g.parent) >= 0) > K // 2
