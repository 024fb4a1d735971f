"""The C++ mirror orbx::LoopClosing (include/orbx.hpp) through tests/cpp/correctloop_cli.cpp: it
builds with g++ against liborbx.so and, on one scene, writes the bytes of the Python path."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import correct_loop_model as M

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "correctloop_cli.cpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory, orbx_built):
    out = tmp_path_factory.mktemp("correctloop_cli") / "correctloop_cli"
    lib_dir = Path(orbx_built).parent
    hip_dir = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "lib"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(SRC), "-o", str(out), f"-L{lib_dir}",
                    "-lorbx", f"-L{hip_dir}", "-lamdhip64", f"-Wl,-rpath,{lib_dir}", f"-Wl,-rpath,{hip_dir}"], check=True)
    return out


def test_cpp_mirror_builds_without_gpu(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2


@pytest.mark.gpu
def test_cpp_chain_writes_the_python_paths_bytes(exe, tmp_path):
    import torch

    from test_gpu_correct_loop import Dev
    name = "band24"
    d = Dev(name)
    sc, st = d.sc, d.st0
    K, cap = sc["kf_mp"].shape
    n, mc = len(sc["mp_bad"]), sc["max_conn"]
    loop_ids = d.loop_ids.cpu().numpy()
    max_edges, max_lc = 400, 200
    head = np.array([K, cap, n, mc, sc["cur"], sc["loop"], sc["min_feat"], len(st["scale"]), len(loop_ids), max_edges, max_lc],
                    np.int32)
    parts = [head, sc["kf_mp"], sc["kf_mp_fused"], sc["kf_n"], sc["kf_bad"], sc["mp_bad"], st["poses"], st["mp_pos"],
             st["mp_corrected_by_kf"], st["mp_corrected_ref"], st["mp_ref_kf"], st["octave"], st["scale"],
             np.asarray(sc["Scw"], np.float64), d.loop_off.cpu().numpy(), loop_ids]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in parts))
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    blob = dst.read_bytes()
    # the same chain through the Python path
    p = d.propagate()
    d.fuse()
    a = d.assemble(max_edges=max_edges, max_lc=max_lc)
    status = d.lc.update_normal_and_depth()
    torch.cuda.synchronize()
    tail = {k: d.d[k].cpu().numpy() for k in ("normal", "max_distance", "min_distance")}
    want = [p[k] for k in ("n_conn", "conn", "corr_S", "kf_corr", "kf_Tcw_nc", "status", "kf_Tcw", "mp_pos", "mp_corrected_by_kf",
                           "mp_corrected_ref", "normal", "max_distance", "min_distance")]
    want += [a[k] for k in ("lc_off", "lc_member", "lc_kf", "lc_w", "kf_ids", "kf_row", "n_rows", "kf_off", "loop_row",
                            "kf_corr_rows", "kf_Tcw_rows", "edge_v", "edge_kind", "n_edges", "edge_off", "pt_ref", "pt_off",
                            "env_blocks", "status")]
    want += [tail["normal"], tail["max_distance"], tail["min_distance"], status.cpu().numpy()]
    at = 0
    for i, w in enumerate(want):
        got = blob[at:at + w.nbytes]
        assert got == w.tobytes(), i
        at += w.nbytes
    assert at == len(blob)
    assert int(a["n_edges"][0]) > 20 and int(p["n_conn"][0]) >= 4
