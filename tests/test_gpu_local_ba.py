"""orbx_local_bundle_adjustment(_batch_device) on the GPU against tests/local_ba_model.py.

Scenes (local_ba_model.SPECS): TUM1 intrinsics, points 3-8 m away, 1 px x scale noise, keyframe
slots and keypoint rows dealt out of storage order.  The smallest at which each piece can go
wrong: 1 free + 1 fixed keyframe with 6 points; 2 keyframes of which the first is flagged
fixed; all monocular / all stereo / mixed; a point with a single observation (Hll invertible
only through lambda), one with none and a fixed keyframe without an edge; 10 % gross outliers
(50 px) with a point behind a camera, leaving a point, and in another scene a free keyframe,
without a level-0 edge in the second optimisation; 63 / 64 / 65 and 255 / 256 / 257 edges; 1 and
257 points; ORBX_LOCAL_BA_MAX_FREE_KF free keyframes, one more (the capacity bit), none.

Every comparison first asserts the conditions on its scene (local_ba_model.guard): all
variants of the model agree on the LM trace, the flags and the active sets, every LDL^T pivot
is positive, and every chi2 / depth that is tested is further from its threshold than 1000 x
its spread between the variants.  Then the flags, n_erase, the trace and the status must
equal the model's, and poses and positions lie within 8 x the measured spread between the
variants (python tests/local_ba_spread.py: 8.77e-9 for a pose entry, 5.0e-8 for a position
entry), floor 2 float32 ulps of the entry.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import local_ba_model as M

pytestmark = pytest.mark.gpu

POSE_SPREAD = 8.77e-9             # python tests/local_ba_spread.py
POS_SPREAD = 5.0e-8
POSE_TOL = 8 * POSE_SPREAD        # floor: 2 float32 ulps of the entry
POS_TOL = 8 * POS_SPREAD


@functools.lru_cache(maxsize=None)
def assert_guard(name):
    sc = M.scene(name)
    vs = M.variants(sc)
    ok, why = M.guard(vs)
    assert ok, (name, why)
    assert M.scene_extra(name, vs[0]), name
    return sc, vs[0]


@pytest.fixture(scope="module")
def opt(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import LocalBundleAdjuster
    o = LocalBundleAdjuster()
    yield o
    o.close()


def keypoints(xy, octv):
    from orbslam2commentedbyxcm_amd import _lib as L
    k = np.zeros(xy.shape[:-1], L.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = xy[..., 0], xy[..., 1], octv
    return k


def upload_arrays(scenes):
    """The arrays of a batch as they are uploaded (kps: the 28-byte keypoint records)."""
    A = M.batch_arrays(scenes)
    A["kps"] = keypoints(A["kps_xy"], A["kps_oct"]).view(np.uint8).reshape(A["n_slots"], A["cap"], 28)
    return A


def run_batch(opt, scenes, level1=True, trace=True, max_free_kf=0, io=None, decoy=None):
    """io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    call); decoy: the scenes whose arrays fill the inputs before an ordered run's real uploads."""
    import torch

    import stream_order as SO
    A = upload_arrays(scenes)
    Q = A if decoy is None else upload_arrays(decoy)
    B = len(scenes)
    dev = torch.device("cuda", opt.device)
    io = io or SO.SyncIO(dev)
    t = lambda k: io.up(A[k], Q[k])  # noqa: E731
    n_kf, n_pt, n_obs = len(A["fixed"]), len(A["pos"]), len(A["obs_kf"])
    d_T = io.full((n_kf, 12), float("nan"), torch.float32)
    d_X = io.full((n_pt, 3), float("nan"), torch.float32)
    d_er = io.full((n_obs,), 9, torch.uint8)
    d_l1 = io.full((n_obs,), 9, torch.uint8) if level1 else None
    d_ne = io.full((B,), -9, torch.int32)
    d_st = io.full((B,), -9, torch.int32)
    d_tr = io.full((B, 2, 2), -9, torch.int32) if trace else None
    s0 = scenes[0]
    fx, fy, cx, cy, bf = s0["cam"]
    ins = [t(k) for k in ("kf_off", "Tcw", "fixed", "slot", "pt_off", "pos", "obs_off", "obs_kf", "obs_kp", "kps",
                          "u_right")]
    sig = io.host(np.asarray(s0["inv_sigma2"], np.float32), np.asarray(s0["inv_sigma2"], np.float32)[::-1])
    io.begin()
    opt.local_ba_batch_device(
        *ins, sig, fx, fy, cx, cy, bf, d_T, d_X, d_er, d_ne, d_st, d_level1=d_l1, d_trace=d_tr,
        max_free_kf=max_free_kf, stream=io.stream)
    io.end()
    return dict(Tcw=io.down(d_T), pos=io.down(d_X), erase=io.down(d_er), level1=io.down(d_l1), n_erase=io.down(d_ne),
                status=io.down(d_st), trace=io.down(d_tr), arrays=A)


def part(got, b):
    """Problem b's rows of a batch result."""
    A = got["arrays"]
    k0, k1 = A["kf_off"][b:b + 2]
    p0, p1 = A["pt_off"][b:b + 2]
    o0, o1 = A["obs_off"][p0], A["obs_off"][p1]
    return dict(Tcw=got["Tcw"][k0:k1], pos=got["pos"][p0:p1], erase=got["erase"][o0:o1],
                level1=None if got["level1"] is None else got["level1"][o0:o1], n_erase=int(got["n_erase"][b]),
                status=int(got["status"][b]), trace=None if got["trace"] is None else got["trace"][b])


def assert_close(got, want32, tol, what):
    """8 x the measured spread between the variants, floor 2 float32 ulps of the entry."""
    lim = np.maximum(tol, 2 * np.spacing(np.abs(want32)).astype(np.float64))
    diff = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    assert np.isfinite(got).all(), what
    assert (diff <= lim).all(), (what, float(diff.max()), float((diff / lim).max()))


def assert_problem(g, sc, r, what):
    dT = np.abs(g["Tcw"].astype(np.float64) - r["Tcw"]).max() if g["Tcw"].size else 0.0
    dX = np.abs(g["pos"].astype(np.float64) - r["pos"]).max() if g["pos"].size else 0.0
    print(f"{what}: trace {None if g['trace'] is None else g['trace'].reshape(-1).tolist()} model "
          f"{r['trace'].reshape(-1).tolist()} n_erase {g['n_erase']} model {r['n_erase']} status {g['status']} "
          f"max |dT| {dT:.3g} max |dX| {dX:.3g}")
    assert g["status"] == r["status"], what
    if g["trace"] is not None:
        assert np.array_equal(g["trace"], r["trace"]), (what, g["trace"].tolist(), r["trace"].tolist())
    if g["level1"] is not None:
        assert np.array_equal(g["level1"], r["level1"]), what
    assert np.array_equal(g["erase"], r["erase"]), what
    assert g["n_erase"] == r["n_erase"], what
    assert_close(g["Tcw"], r["Tcw"], POSE_TOL, what + " poses")
    assert_close(g["pos"], r["pos"], POS_TOL, what + " positions")
    fixed = np.asarray(sc["fixed"]).astype(bool)
    assert g["Tcw"][fixed].tobytes() == np.asarray(sc["Tcw"], np.float32)[fixed].tobytes(), what


@pytest.mark.parametrize("name", list(M.SPECS))
def test_single_problem_batch_equals_model(opt, name):
    sc, r = assert_guard(name)
    got = run_batch(opt, [sc])
    assert_problem(part(got, 0), sc, r, name)


def test_scenes_are_what_their_names_say():
    for n in (63, 64, 65, 255, 256, 257):
        assert len(M.scene(f"edges-{n}")["obs_kf"]) == n
    sc, r = assert_guard("single-obs")
    cnt = np.diff(sc["obs_off"])
    assert (cnt == 1).any() and (cnt == 0).any()
    assert not np.isin(len(sc["fixed"]) - 1, sc["obs_kf"])              # the fixed keyframe without an edge
    assert r["pos"][cnt == 0].tobytes() == sc["pos"][cnt == 0].tobytes()
    for kind, name in (("mono", "mono"), ("stereo", "stereo")):
        assert assert_guard(name)[1]["stereo"].all() == (kind == "stereo")
        assert assert_guard(name)[1]["stereo"].any() == (kind == "stereo")
    st = assert_guard("mixed")[1]["stereo"]
    assert st.any() and not st.all()
    sc, r = assert_guard("out10-starve-pt")
    assert r["level1"].sum() >= 0.1 * len(r["level1"]) and (r["depth"][0] < 0).any()
    assert int((~np.asarray(assert_guard("kf-cap")[0]["fixed"]).astype(bool)).sum()) == M.MAX_FREE_KF
    assert len(assert_guard("pts-1")[0]["pos"]) == 1 and len(assert_guard("pts-257")[0]["pos"]) == 257
    sc = M.scene("mixed")
    assert not np.array_equal(np.sort(sc["slot"]), sc["slot"])          # slots out of storage order
    assert (np.diff(sc["obs_kp"]) < 0).any()


def test_capacity_and_no_free_keyframe_return_the_inputs(opt):
    over = M.make_scene(0, n_free=M.MAX_FREE_KF + 1, n_fixed=1, n_pts=12, max_obs=6)
    none = M.make_scene(0, n_free=0, n_fixed=3, n_pts=12)
    small = M.scene("mixed")                                            # 3 free keyframes, sized for 2
    for sc, status, kw in ((over, M.STATUS_CAPACITY, {}), (none, M.STATUS_NO_FREE_KF, {}),
                           (small, M.STATUS_CAPACITY, dict(max_free_kf=2))):
        r = M.local_ba(sc, **({"max_free": 2} if kw else {}))
        assert r["status"] == status
        g = part(run_batch(opt, [sc], **kw), 0)
        assert g["status"] == status and g["n_erase"] == 0 and not g["trace"].any()
        assert not g["erase"].any() and not g["level1"].any()
        assert g["Tcw"].tobytes() == sc["Tcw"].tobytes() and g["pos"].tobytes() == sc["pos"].tobytes()


def test_bad_indices_are_no_edges(opt):
    sc = dict(M.scene("mixed"))
    kf, kp = sc["obs_kf"].copy(), sc["obs_kp"].copy()
    kf[3], kp[7], kf[11] = len(sc["fixed"]), sc["kps_xy"].shape[1], -1
    o0 = sc["obs_off"][5]
    kf[o0 + 1] = kf[o0]                                                 # a keyframe twice in one point
    sc["obs_kf"], sc["obs_kp"] = kf, kp
    vs = M.variants(sc)
    ok, why = M.guard(vs)
    assert ok, why
    r = vs[0]
    assert r["status"] == M.STATUS_BAD_INDEX
    g = part(run_batch(opt, [sc]), 0)
    assert_problem(g, sc, r, "bad indices")
    assert not g["erase"][[3, 7, 11, o0 + 1]].any()


BATCH8 = ("mixed", "1+1-6pts", "edges-65", "out10-starve-pt", "single-obs", "edges-257", "stereo", "out10-starve-kf")


def test_batch_of_8_equals_model_alone_and_twice(opt):
    scenes = [assert_guard(n) for n in BATCH8]
    got = run_batch(opt, [s for s, _ in scenes])
    again = run_batch(opt, [s for s, _ in scenes])
    for k in ("Tcw", "pos", "erase", "level1", "n_erase", "status", "trace"):
        assert got[k].tobytes() == again[k].tobytes(), k
    for b, (name, (sc, r)) in enumerate(zip(BATCH8, scenes)):
        g = part(got, b)
        assert_problem(g, sc, r, f"batch8[{b}] {name}")
        alone = part(run_batch(opt, [sc]), 0)
        for k in ("Tcw", "pos", "erase", "level1", "trace"):
            assert g[k].tobytes() == alone[k].tobytes(), (name, k)
        assert (g["n_erase"], g["status"]) == (alone["n_erase"], alone["status"]), name


def test_optional_outputs_may_be_null(opt):
    sc, r = assert_guard("mixed")
    g = part(run_batch(opt, [sc], level1=False, trace=False), 0)
    assert_problem(g, sc, r, "no level1, no trace")


def host_call(opt, sc, **kw):
    fx, fy, cx, cy, bf = sc["cam"]
    return opt.LocalBundleAdjustment(sc["Tcw"], sc["fixed"], sc["slot"], sc["pos"], sc["obs_off"], sc["obs_kf"],
                                     sc["obs_kp"], keypoints(sc["kps_xy"], sc["kps_oct"]), sc["u_right"],
                                     sc["inv_sigma2"], fx, fy, cx, cy, bf, **kw)


@pytest.mark.parametrize("name", ["1+1-6pts", "mono", "single-obs", "out10-starve-kf", "edges-257", "pts-1"])
def test_single_host_call_equals_batch_bytes(opt, name):
    sc, r = assert_guard(name)
    g = part(run_batch(opt, [sc]), 0)
    h = host_call(opt, sc)
    for k in ("Tcw", "pos", "erase", "level1", "trace"):
        assert h[k].tobytes() == g[k].tobytes(), (name, k)
    assert (h["n_erase"], h["status"]) == (g["n_erase"], g["status"])
    assert opt.last_call_us() > 0


def test_host_call_without_a_free_keyframe(opt):
    sc = M.make_scene(0, n_free=0, n_fixed=3, n_pts=12)
    h = host_call(opt, sc)
    assert h["status"] == M.STATUS_NO_FREE_KF and h["Tcw"].tobytes() == sc["Tcw"].tobytes()
    assert h["pos"].tobytes() == sc["pos"].tobytes() and not h["erase"].any()
