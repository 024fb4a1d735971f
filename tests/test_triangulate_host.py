"""CPU-side checks of the device CreateNewMapPoints (orbx_triangulate_pairs*): the model's
variants and scenes (tests/triangulate_model.py), the nullable-depth rule against the oracle's
mvDepth, the C ABI's argument errors without a GPU, the ctypes layouts against the header, and
the C++ mirror's CLI building against it."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import triangulate_model as M

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("name", M.ALL_SCENES)
def test_variants_pass_the_guard(name):
    vs = M.scene_variants(name)
    assert len(vs) == len(M.VARIANTS) >= 6
    ok, why = M.guard(vs)
    assert ok, (name, why)
    sc = M.scene(name)
    for row, m in zip(vs[0], sc["matched"]):
        assert np.array_equal(row["new_idx"], np.flatnonzero(row["reason"] == 0)) and row["nnew"] == len(row["new_idx"])
        assert len(row["reason"]) == len(m) <= sc["cap"]
        assert (row["out"][row["reason"] != 0] == 0).all()


def test_guard_notices_a_pair_on_a_threshold():
    """A z1 one rounding error from 0 fails the guard (it does reject what it is there to reject)."""
    vs = [[dict(r) for r in v] for v in M.scene_variants("n1")]
    for i, v in enumerate(vs):
        v[0]["tested"] = [[(n, (1e-15 + 1e-17 * i) if n == "z1" else x) for n, x in v[0]["tested"][0]]]
    ok, why = M.guard(vs)
    assert not ok and "z1" in why


def test_every_reason_and_method_occurs():
    reasons, methods = M.histogram()
    print("reasons", reasons.tolist(), "methods", methods.tolist())
    assert all(reasons[r] > 0 for r in M.REACHABLE_REASONS), reasons.tolist()
    assert all(methods[m] > 0 for m in (0, 1, 2, 3)), methods.tolist()
    assert M.scene_extra()


def test_scene_shapes():
    counts = sorted(len(m) for name in M.ALL_SCENES for m in M.scene(name)["matched"])
    for want in (0, 1, 63, 64, 65, 255, 256, 257):
        assert want in counts
    full = M.scene("full")
    assert len(full["matched"][0]) == full["cap"]
    assert sorted({len(M.scene(n)["pairs"]) for n in M.ALL_SCENES}) == [1, 3, 17]
    for name in ("p3", "p17"):
        sc = M.scene(name)
        assert 2 <= sc["nkf"] <= 6
        assert set(sc["pairs"][:, 0]) & set(sc["pairs"][:, 1])   # a keyframe that is KF1 here and KF2 there
    p17 = M.scene("p17")
    assert any(k["raw"] is not None for k in p17["kfs"]) and any(k["depth"] is None and k["u_right"] is not None
                                                                   for k in p17["kfs"])
    assert p17["kfs"][5]["u_right"] is None


def test_derived_depth_is_the_oracles_mvdepth(oracle):
    """depth NULL means the float mbf / (keys.x - u_right): on the keyframe pipeline's synthetic
    stereo frames that is ComputeStereoMatches' mvDepth bit for bit wherever mvuRight >= 0."""
    from orbslam2commentedbyxcm_amd import synth
    from orbslam2commentedbyxcm_amd.keyframes import EUROC as s
    from orbslam2commentedbyxcm_amd.matcher import FrameView
    O = oracle
    p = O.params(s["nfeatures"], s["scale"], s["nlevels"], s["ini_th"], s["min_th"])
    seq = synth.StereoSequence(3, 2, s["width"], s["height"], step=16, margin=256, disp=13)
    sf = M.SCALE
    nstereo = 0
    for g in range(2):
        left, right = seq.views([g])
        kl, dl, _ = O.extract(left[0], p)
        kr, dr, _ = O.extract(right[0], p)
        v = FrameView(keys=kl, desc=dl, fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], bf=s["bf"], b=s["bf"] / s["fx"],
                      max_x=float(s["width"]), max_y=float(s["height"]), scale_factors=sf, level_sigma2=sf * sf)
        ur, dp = O.compute_stereo_matches(v, kr, dr, O.pyramid(left[0], p), O.pyramid(right[0], p), s["fx"])
        st = ur >= 0
        nstereo += int(st.sum())
        got = M.derived_depth(kl["x"], ur)
        assert np.float32(s["bf"]) == M.BF
        assert got[st].tobytes() == dp[st].tobytes()
    assert nstereo > 200


# ---- the C ABI without a GPU ----
def _valid_batch():
    from orbslam2commentedbyxcm_amd import _lib as L
    cam = M.cam()
    cv = cam.c()
    kfs = (L.KeyFrameGeomDevice * 2)()
    for k in kfs:
        k.keys_un, k.n = 256, 512      # never dereferenced: the checks only look at them
    pairs = np.array([[0, 1]], np.int32)
    out = L.NewMapPoints()
    return cam, cv, kfs, pairs, out


def test_argument_errors_need_no_gpu(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    cam, cv, kfs, pairs, out = _valid_batch()
    fake = C.c_void_p(4096)        # stands for d_pairs / d_npairs: never dereferenced
    pp = pairs.ctypes.data_as(C.POINTER(C.c_int32))

    def call(nkf=2, kfs=kfs, cam=C.addressof(cv), npairs=1, pairs=pp, cap=64, d_pairs=fake, d_npairs=fake,
             out=C.byref(out)):
        rc = lib.orbx_triangulate_pairs_batch_device(None, nkf, None if kfs is None else C.addressof(kfs), cam, npairs,
                                                     pairs, cap, d_pairs, d_npairs, 0.11, 47.9, out, None)
        return rc, lib.orbx_last_error().decode()

    assert call() == (L.ORBX_ERR_ARG, "null matcher")      # every argument is fine: only the handle is missing
    for kw, why in ((dict(kfs=None), "null buffer"), (dict(cam=None), "null argument"), (dict(pairs=None), "null buffer"),
                    (dict(d_pairs=None), "null buffer"), (dict(d_npairs=None), "null buffer"),
                    (dict(out=None), "null argument"), (dict(cap=8193), "cap above 8192"), (dict(cap=0), "bad cap"),
                    (dict(npairs=-1), "negative count"), (dict(nkf=-1), "negative count"),
                    (dict(nkf=1), "keyframe index out of range")):
        assert call(**kw) == (L.ORBX_ERR_ARG, why), kw
    bad = np.array([[0, -1]], np.int32)
    assert call(pairs=bad.ctypes.data_as(C.POINTER(C.c_int32))) == (L.ORBX_ERR_ARG, "keyframe index out of range")
    nokeys = (L.KeyFrameGeomDevice * 2)()
    assert call(kfs=nokeys) == (L.ORBX_ERR_ARG, "null keyframe array")
    assert call(cap=8192) == (L.ORBX_ERR_ARG, "null matcher")

    # the single host form
    n = np.array([1], np.int32)
    kp = np.zeros(1, L.KEYPOINT_DTYPE)
    k1 = L.KeyFrameGeomDevice()
    k1.keys_un, k1.n = kp.ctypes.data, n.ctypes.data
    mt = np.zeros((1, 2), np.int32)
    mp = mt.ctypes.data_as(C.POINTER(C.c_int32))

    def one(kf1=C.byref(k1), kf2=C.byref(k1), cam=C.addressof(cv), k=1, matched=mp, out=C.byref(out)):
        rc = lib.orbx_triangulate_pairs(None, kf1, kf2, cam, k, matched, 0.11, 47.9, out)
        return rc, lib.orbx_last_error().decode()

    assert one() == (L.ORBX_ERR_ARG, "null matcher")
    assert one(kf1=None) == (L.ORBX_ERR_ARG, "null keyframe")
    assert one(kf2=None) == (L.ORBX_ERR_ARG, "null keyframe")
    assert one(k=-1) == (L.ORBX_ERR_ARG, "negative count")
    assert one(k=8193) == (L.ORBX_ERR_ARG, "more than 8192 matched pairs")
    assert one(matched=None) == (L.ORBX_ERR_ARG, "null buffer")
    assert one(cam=None) == (L.ORBX_ERR_ARG, "null argument")
    assert one(out=None) == (L.ORBX_ERR_ARG, "null argument")
    neg = np.array([-1], np.int32)
    k2 = L.KeyFrameGeomDevice()
    k2.keys_un, k2.n = kp.ctypes.data, neg.ctypes.data
    assert one(kf2=C.byref(k2)) == (L.ORBX_ERR_ARG, "negative count")


def test_symbols_and_header_text(orbx_built):
    lib = C.CDLL(str(orbx_built))
    for name in ("orbx_triangulate_pairs_batch_device", "orbx_triangulate_pairs"):
        assert hasattr(lib, name)
    text = (ROOT / "include" / "orbx.h").read_text()
    for ref in ("LocalMapping.cc:307-501", "KeyFrame.cc:666-679", "MapPoint.cc:386-439", "neighbour i+1"):
        assert ref in text


def test_struct_layouts_equal_the_headers(tmp_path):
    from orbslam2commentedbyxcm_amd import _lib as L
    structs = {"orbx_keyframe_geom_device": L.KeyFrameGeomDevice, "orbx_new_mappoints": L.NewMapPoints}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf(" %zu", offsetof({cname}, {f}));')
        lines.append('printf("\\n");')
    src = tmp_path / "offsets.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "orbx.h"\nint main() {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = tmp_path / "offsets"
    subprocess.run(["g++", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    want = [" ".join([cname, str(C.sizeof(cls))] + [str(getattr(cls, f).offset) for f, _ in cls._fields_])
            for cname, cls in structs.items()]
    assert got == want


def test_cli_compiles_with_wall(tmp_path, orbx_built):
    lib_dir = Path(orbx_built).parent
    out = tmp_path / "triangulate_cli"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "cpp" / "triangulate_cli.cpp"), "-o", str(out), f"-L{lib_dir}", "-lorbx",
                        f"-Wl,-rpath,{lib_dir}"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    assert subprocess.run([str(out)], capture_output=True, timeout=60).returncode == 2
