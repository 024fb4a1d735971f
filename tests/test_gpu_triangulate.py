"""orbx_triangulate_pairs(_batch_device) on the GPU against tests/triangulate_model.py.

Scenes (triangulate_model.SPECS): the EuRoC calibration, octaves 0-7, pixel noise 1 px x scale,
six keyframes (lateral, forward, below-mb and coincident-centre baselines, one monocular, two with
mvKeys != mvKeysUn, two without a depth array); matched-pair counts 0, 1, 63 / 64 / 65 (wave),
255 / 256 / 257 (the workgroup's stride) and one full cap row; 1, 3 and 17 keyframe pairs.

Every comparison first asserts the model's guard on its scene (all six variants agree on reason
and method, every compared quantity is further from its threshold than 1000 x the variants'
largest difference) and scene_extra.  Then reason, method, nnew and new_idx are equal to the
model's and pos / normal / max_distance / min_distance are within tolerance.

Tolerance: tests/triangulate_spread.py measures the largest output difference between the
variants over these scenes: 2.24e-10 (X3D_SPREAD).  The tolerance is 8 x that, 1.79e-9, floor 2
float32 ulps of the entry (the outputs are floats: the floor is what binds).  On the MI355X the
largest difference to the model's double result rounded to float was 0 (MAX_SEEN_ON_MI355X): every
pos / normal / distance entry of every scene, and of the pipeline's 3,585 new points, is the float
the model's double rounds to.
"""
from __future__ import annotations

import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import triangulate_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
X3D_SPREAD = 2.24e-10            # python tests/triangulate_spread.py
X3D_TOL = 8 * X3D_SPREAD         # floor: 2 float32 ulps of the entry
MAX_SEEN_ON_MI355X = 0.0         # largest |GPU - float32(model)| over all scenes and the pipeline test
FLOATS = ("pos", "normal", "max_distance", "min_distance")
NAMES = ("reason", "method") + FLOATS + ("nnew", "new_idx")


@functools.lru_cache(maxsize=None)
def assert_guard(name):
    vs = M.scene_variants(name)
    ok, why = M.guard(vs)
    assert ok, (name, why)
    assert M.scene_extra()
    return M.scene(name), vs[0]


@pytest.fixture(scope="module")
def tri(orbx_built):
    from orbslam2commentedbyxcm_amd.mapping import Triangulator
    t = Triangulator()
    yield t
    t.close()


SENT_U8, SENT_F32, SENT_I32 = 0xA5, -12345.5, -77


def sentinel_outputs(P, cap, dev, skip=(), full=None):
    import torch
    full = full or (lambda shape, v, dtype: torch.full(shape, v, dtype=dtype, device=dev))
    f = lambda *s: full(s, SENT_F32, torch.float32)  # noqa: E731
    u = lambda *s: full(s, SENT_U8, torch.uint8)  # noqa: E731
    i = lambda *s: full(s, SENT_I32, torch.int32)  # noqa: E731
    out = {"reason": u(P, cap), "method": u(P, cap), "pos": f(P, cap, 3), "normal": f(P, cap, 3),
           "max_distance": f(P, cap), "min_distance": f(P, cap), "nnew": i(P), "new_idx": i(P, cap)}
    return {k: v for k, v in out.items() if k not in skip}


def decoy_pack(Pk):
    """The packed scene with every keyframe's keypoints, right coordinates and depths moved; the
    pair tables, counts and octaves are the real ones."""
    Q = dict(Pk)
    Q["kfs"] = []
    for K in Pk["kfs"]:
        D = dict(K)
        for k in ("keys_un", "keys"):
            if K[k] is not None:
                D[k] = K[k].copy()
                D[k]["x"] += np.float32(1.5)
                D[k]["y"] -= np.float32(0.75)
        for k, d in (("u_right", 0.5), ("depth", 0.125)):
            if K[k] is not None:
                D[k] = np.where(K[k] > 0, K[k] + np.float32(d), K[k]).astype(np.float32)
        Q["kfs"].append(D)
    return Q


def run_batch(tri, sc, rows=None, skip=(), io=None, decoy=False, packed=None):
    """The batch call on the scene's rows; returns host arrays of the outputs (+ the packed inputs).
    io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    call); decoy: fill the inputs with decoy_pack's arrays before an ordered run's real uploads;
    packed: the packed inputs to run instead of the scene's."""
    import torch

    import stream_order as SO
    from orbslam2commentedbyxcm_amd.mapping import keyframe_geom_device
    Pk = M.pack(sc, rows) if packed is None else packed
    Qk = decoy_pack(Pk) if decoy else Pk
    dev = torch.device("cuda", tri.device)
    io = io or SO.SyncIO(dev)
    raw = lambda K, k: K[k].view(np.uint8) if k in ("keys_un", "keys") and K[k] is not None else K[k]  # noqa: E731
    keep, recs = [], []
    for K, D in zip(Pk["kfs"], Qk["kfs"]):
        d = {k: None if K[k] is None else io.up(raw(K, k), raw(D, k)) for k in ("keys_un", "keys", "u_right", "depth", "n")}
        keep.append(d)
        recs.append(keyframe_geom_device(d["keys_un"], d["n"], K["Tcw"].reshape(3, 4), d["u_right"], d["depth"], d["keys"]))
    P, cap = len(Pk["pairs"]), Pk["cap"]
    out = sentinel_outputs(max(P, 1), cap, dev, skip, io.full)
    d_pairs = io.up(Pk["d_pairs"] if P else np.zeros((1, cap, 2), np.int32))
    d_np = io.up(Pk["npairs"] if P else np.zeros(1, np.int32))
    pairs = np.ascontiguousarray(Pk["pairs"], np.int32).reshape(-1, 2)
    h_pairs = io.host(pairs, pairs[:, ::-1])
    cam = M.cam()                                     # its level tables are the caller's host arrays too
    for name in ("scale_factors", "level_sigma2"):
        a = np.ascontiguousarray(getattr(cam, name), np.float32)
        setattr(cam, name, io.host(a, a[::-1].copy()))
    io.begin()
    tri.triangulate_pairs_batch_device(recs, cam, h_pairs, cap, d_pairs, d_np, out, stream=io.stream)
    io.end()
    got = {k: io.down(v) for k, v in out.items()}
    got["packed"] = Pk
    return got


def assert_floats_close(got, want64, what):
    """8 x the measured spread between the variants, floor 2 float32 ulps of the entry."""
    want32 = want64.astype(np.float32)
    tol = np.maximum(X3D_TOL, 2 * np.spacing(np.abs(want32)).astype(np.float64))
    diff = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    assert np.isfinite(got).all(), what
    assert (diff <= tol).all(), (what, float(diff.max()))
    return float(diff.max()) if diff.size else 0.0


def assert_row(got, j, ref, cap, what):
    """Row j of the batch outputs against a model row; slots past the row's count keep the sentinels."""
    k = len(ref["reason"])
    assert np.array_equal(got["reason"][j, :k], ref["reason"]), (what, got["reason"][j, :k].tolist(), ref["reason"].tolist())
    assert np.array_equal(got["method"][j, :k], ref["method"]), what
    assert got["nnew"][j] == ref["nnew"], what
    assert np.array_equal(got["new_idx"][j, :ref["nnew"]], ref["new_idx"]), what
    worst = 0.0
    for name, cols in (("pos", slice(0, 3)), ("normal", slice(3, 6)), ("max_distance", 6), ("min_distance", 7)):
        worst = max(worst, assert_floats_close(got[name][j, :k], ref["out"][:, cols], (what, name)))
    rej = ref["reason"] != 0
    for name in FLOATS:
        assert (got[name][j, :k][rej] == 0).all(), (what, name)      # rejected slots: 0
    # output hygiene: nothing past npairs[p], nothing past nnew[p]
    assert (got["reason"][j, k:] == SENT_U8).all() and (got["method"][j, k:] == SENT_U8).all(), what
    for name in FLOATS:
        assert (got[name][j, k:] == np.float32(SENT_F32)).all(), (what, name)
    assert (got["new_idx"][j, ref["nnew"]:] == SENT_I32).all(), what
    print(f"{what}: {k} pairs, {ref['nnew']} new, max |d| {worst:.3g}")
    return worst


@pytest.mark.parametrize("name", M.ALL_SCENES)
def test_batch_equals_model(tri, name):
    sc, ref = assert_guard(name)
    got = run_batch(tri, sc)
    for j, r in enumerate(ref):
        assert_row(got, j, r, sc["cap"], f"{name}[{j}]")


def test_a_pair_alone_and_inside_each_batch_gives_equal_bytes(tri):
    sc, ref = assert_guard("p17")
    whole = run_batch(tri, sc)
    three = [4, 7, 15]
    sub = run_batch(tri, sc, three)
    for j, r in enumerate(three):
        k = len(ref[r]["reason"])
        assert_row(sub, j, ref[r], sc["cap"], f"p17 rows {three}[{j}]")
        for name in NAMES[:-2]:
            assert sub[name][j, :k].tobytes() == whole[name][r, :k].tobytes(), (r, name)
    for r in (1, 4, 7, 8, 15, 16):
        k = len(ref[r]["reason"])
        one = run_batch(tri, sc, [r])
        for name in NAMES[:-2]:
            assert one[name][0, :k].tobytes() == whole[name][r, :k].tobytes(), (r, name)
        assert one["nnew"][0] == whole["nnew"][r]
        assert one["new_idx"][0].tobytes() == whole["new_idx"][r].tobytes()
    again = run_batch(tri, sc)
    for name in NAMES:
        assert again[name].tobytes() == whole[name].tobytes(), name


@pytest.mark.parametrize("name", ["n0", "n1", "n65", "n257", "full", "coincident"])
def test_single_host_call_equals_batch_bytes(tri, name):
    sc, ref = assert_guard(name)
    got = run_batch(tri, sc)
    a, b = sc["pairs"][0]

    def host(K):
        return dict(keys_un=M.keypoints(K["un"], K["oct"]), Tcw=np.asarray(K["Tcw"]).reshape(3, 4), u_right=K["u_right"],
                    depth=K["depth"], keys=None if K["raw"] is None else M.keypoints(K["raw"], K["oct"]))
    h = tri.triangulate_pairs(host(sc["kfs"][a]), host(sc["kfs"][b]), M.cam(), sc["matched"][0])
    k = len(sc["matched"][0])
    for nm in NAMES[:-2]:
        assert h[nm].tobytes() == got[nm][0, :k].tobytes(), nm
    assert h["nnew"] == got["nnew"][0] == ref[0]["nnew"]
    assert np.array_equal(h["new_idx"], ref[0]["new_idx"])
    assert tri.last_call_us() > 0


def test_every_output_may_be_null(tri):
    sc, ref = assert_guard("p3")
    full = run_batch(tri, sc)
    for skip in (("reason", "method"), ("pos", "normal", "max_distance", "min_distance"), ("nnew",), ("new_idx",),
                 NAMES[:-1]):
        lean = run_batch(tri, sc, skip=skip)
        for name in NAMES:
            if name not in skip:
                assert lean[name].tobytes() == full[name].tobytes(), (skip, name)


def test_pipeline_triangulates_the_searchs_own_pairs(orbx_built):
    """StereoKeyFramePipeline(B=6, triangulate=True), 3 steps: the new arrays equal the model fed
    with the host copies of the same step, and every existing array of results() is byte-equal to
    a triangulate=False run."""
    import torch

    from orbslam2commentedbyxcm_amd.keyframes import StereoKeyFramePipeline
    res = {}
    for flag in (False, True):
        pl = StereoKeyFramePipeline(6, triangulate=flag)
        pl.run(3)
        torch.cuda.synchronize()
        res[flag] = pl.host_results()
        P, cap, plan, poses, mb = len(pl.plan.pairs), pl.cap, pl.plan, pl._rec_poses, pl.mb
        pl.close()
    off, on = res[False], res[True]
    assert set(on) - set(off) == {"new_" + k for k in NAMES}
    # rows the pipeline allocates uninitialised are defined up to their count only
    counted = {"kr": "nr", "dr": "nr", "tri_pairs": "tri_n"}
    for k in off:
        if k in counted:
            for row, (a, b) in enumerate(zip(off[k], on[k])):
                n = int(off[counted[k]][row])
                assert a[:n].tobytes() == b[:n].tobytes(), (k, row)
        else:
            assert np.asarray(off[k]).tobytes() == np.asarray(on[k]).tobytes(), k
    assert P > 0 and int(on["tri_n"].sum()) > 100
    # the model on the host copies: KF1 is a local keyframe (its own depth array), KF2 a
    # gathered neighbour (depth NULL: derived from u_right)
    kfs = {}

    def kf(rec, with_depth):
        n = int(on["nl"][rec])
        ur = on["ur"][rec, :n]
        un = np.stack([on["kl"][rec, :n]["x"], on["kl"][rec, :n]["y"]], 1)
        eff = on["depth"][rec, :n] if with_depth else M.derived_depth(un[:, 0], ur)
        return dict(n=n, un=un, raw=None, oct=on["kl"][rec, :n]["octave"], u_right=ur, depth_eff=eff,
                    Tcw=np.asarray(poses[rec], np.float32)[:3, :4].reshape(-1), Ow=M.centre(np.asarray(poses[rec])[:3, :4]))
    assert np.float32(mb) == M.MB
    worst, total, seen = 0.0, 0, np.zeros(10, np.int64)
    for p, (a, b) in enumerate(plan.pairs):
        k1 = kfs.setdefault((a, True), kf(a, True))
        k2 = kfs.setdefault((b, False), kf(b, False))
        m = on["tri_pairs"][p, :on["tri_n"][p]]
        vs = [M.triangulate_row(k1, k2, m, s, c) for s, c in M.VARIANTS]
        ok, why = M.guard([[v] for v in vs])
        assert ok, (p, why)
        got = {k: on["new_" + k][p:p + 1] for k in NAMES}
        r = vs[0]
        k = len(m)
        assert np.array_equal(got["reason"][0, :k], r["reason"]) and np.array_equal(got["method"][0, :k], r["method"]), p
        assert got["nnew"][0] == r["nnew"] and np.array_equal(got["new_idx"][0, :r["nnew"]], r["new_idx"]), p
        for name, cols in (("pos", slice(0, 3)), ("normal", slice(3, 6)), ("max_distance", 6), ("min_distance", 7)):
            worst = max(worst, assert_floats_close(got[name][0, :k], r["out"][:, cols], (p, name)))
        total += r["nnew"]
        seen += np.bincount(r["reason"], minlength=10)
    print(f"pipeline: {P} keyframe pairs, {total} new points, reasons {seen.tolist()}, max |d| {worst:.3g}")
    assert total > 50


def _hex(a) -> str:
    return " ".join("%08x" % int(v) for v in np.asarray(a, np.float32).reshape(-1).view(np.uint32))


def test_cpp_mirror_prints_the_models_line(tri, tmp_path, orbx_built):
    """tests/cpp/triangulate_cli.cpp (orbx::LocalMapping::TriangulatePairs) on one pair per method."""
    lib_dir = Path(orbx_built).parent
    exe = tmp_path / "triangulate_cli"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "cpp" / "triangulate_cli.cpp"), "-o", str(exe), f"-L{lib_dir}", "-lorbx",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    sc, ref = assert_guard("p17")
    got = run_batch(tri, sc)
    done = set()
    for r, ((a, b), m) in enumerate(zip(sc["pairs"], sc["matched"])):
        for s, (i1, i2) in enumerate(m):
            key = (int(ref[r]["reason"][s]), int(ref[r]["method"][s]))
            if key not in ((0, 1), (0, 2), (0, 3), (8, 1)) or key in done:
                continue
            done.add(key)
            lines = [f"{_hex([M.FX, M.FY, M.CX, M.CY, M.MB, M.BF])}", str(M.NLEVELS), _hex(M.SCALE), _hex(M.SIGMA2)]
            for K, i in ((sc["kfs"][a], i1), (sc["kfs"][b], i2)):
                raw, ur, dp = K["raw"], K["u_right"], K["depth"]
                lines += [_hex(K["Tcw"]), f"{_hex(K['un'][i])} {int(K['oct'][i])}",
                          f"{int(raw is not None)} {_hex(raw[i] if raw is not None else [0, 0])}",
                          f"{int(ur is not None)} {_hex([ur[i] if ur is not None else 0])}",
                          f"{int(dp is not None)} {_hex([dp[i] if dp is not None else 0])}"]
            path = tmp_path / f"pair_{key[0]}_{key[1]}.txt"
            path.write_text("\n".join(lines) + "\n")
            out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            o32 = ref[r]["out"][s].astype(np.float32)
            # the batch form's bytes for this slot: equal to the CLI's, and within tolerance of the model's line
            want = (f"reason {key[0]} method {key[1]} pos {_hex(got['pos'][r, s])} normal {_hex(got['normal'][r, s])} "
                    f"max {_hex(got['max_distance'][r, s])} min {_hex(got['min_distance'][r, s])} nnew {int(key[0] == 0)}")
            assert out.stdout == want + "\n", (key, out.stdout, want)
            model = (f"reason {key[0]} method {key[1]} pos {_hex(o32[0:3])} normal {_hex(o32[3:6])} max {_hex(o32[6])} "
                     f"min {_hex(o32[7])} nnew {int(key[0] == 0)}")
            print(key, "cli == model line:", out.stdout.strip() == model)
    assert done == {(0, 1), (0, 2), (0, 3), (8, 1)}
