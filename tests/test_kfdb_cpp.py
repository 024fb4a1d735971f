"""The C++ mirror of ORBVocabulary::score / KeyFrameDatabase (include/orbx.hpp) through
tests/cpp/kfdb_cli.cpp: it builds with g++ against liborbx.so, scores on the host like the
model without a GPU and, on the GPU, returns the model's candidates for the relocalisation
and loop scenes of tests/test_gpu_kfdb.py."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import kfdb_model as M
import vocab_scenes as VS
from test_kfdb_host import LOOP_SEED, RELOC_SEED

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "kfdb_cli.cpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory, orbx_built):
    out = tmp_path_factory.mktemp("kfdb_cli") / "kfdb_cli"
    lib_dir = Path(orbx_built).parent
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out),
                    f"-L{lib_dir}", "-lorbx", f"-Wl,-rpath,{lib_dir}"], check=True)
    return out


def _bow(b: dict) -> str:
    return " ".join([str(len(b))] + [f"{w} {b[w]:.17g}" for w in sorted(b)])


def _run(exe, tmp_path, voc, lines, max_kf=8, max_words=8):
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(voc), str(script), str(max_kf), str(max_words)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.split("\n")[:-1]


def test_cpp_bow_score_matches_model_without_gpu(exe, tmp_path):
    rng = np.random.default_rng(9)
    pairs = [(M.random_bow(rng, int(rng.integers(0, 80)), 120), M.random_bow(rng, int(rng.integers(0, 80)), 120))
             for _ in range(40)] + [({1: 0.5, 2: 0.5}, {3: 1.0}), ({}, {})]
    out = _run(exe, tmp_path, "-", [f"score {_bow(a)} {_bow(b)}" for a, b in pairs])
    want = ["score %016x" % int(np.float64(M.l1_score(a, b)).view(np.uint64)) for a, b in pairs]
    assert out == want
    assert out[-1] == "score 8000000000000000"  # -0.0


@pytest.mark.gpu
def test_cpp_database_matches_model(exe, tmp_path):
    voc = tmp_path / "voc.txt"
    voc.write_text(VS.make_vocab(71, k=10, L=3).text())
    ops, queries = M.reloc_scene(RELOC_SEED)
    _, loops = M.loop_scene(LOOP_SEED)  # over the first 120 ids' scene; here on the 300-id one
    lines = []
    for op in ops:
        if op[0] == "add":
            lines.append(f"add {op[1]} {_bow(op[2])}")
        elif op[0] == "erase":
            lines.append(f"erase {op[1]}")
        else:
            lines.append(f"covis {op[1]} {len(op[2])} " + " ".join(map(str, op[2])))
    model = M.replay(ops)
    want = []
    for q in queries:
        lines.append(f"reloc {_bow(q)}")
        want.append(model.detect_relocalization_candidates(q))
    for bow, conn, ms in loops:
        conn = [c for c in conn if c in model.live]
        lines.append(f"loop {float(ms):.9g} {len(conn)} " + " ".join(map(str, conn)) + f" {_bow(bow)}")
        want.append(model.detect_loop_candidates(bow, conn, ms))
    lines += ["clear", f"reloc {_bow(queries[0])}"]
    want.append([])
    out = _run(exe, tmp_path, voc, lines, 300, 128)
    assert out == [" ".join(["cand"] + [str(i) for i in w]) for w in want]
    assert any(len(w) >= 2 for w in want)
