"""orbx_pose_optimization(_batch_device) on the GPU against tests/pose_opt_model.py.

Scenes: points 1-8 m away, TUM1 / KITTI intrinsics, octaves 0-7 with invSigma2 =
1.2^(-2 octave), pixel noise 1 px x scale, fixed seeds (pose_opt_model.SEEDS).  Edge counts
0, 2, 3, 9, 10 (the two early exits), 63-65 (wave), 255-257 (workgroup stride), 1983 / 1985
(either side of the kernel's LDS staging capacity, 1984), cap 5000 with 2000 edges; all
monocular, all stereo and mixed; MapPoint ids of -1, negative and outside the table
interleaved with the valid ones.

Every comparison first asserts the conditions on its scene (pose_opt_model.guard): the model's
summation orders -- forward, reversed, pairwise and the kernel's own tree shape -- agree on
the whole LM trace, and every chi2 at every classification is further from its threshold
than 1000 x the largest chi2 difference between them.  Then mvbOutlier, the return value,
nInitialCorrespondences and the trace are equal to the model's and Tcw is within TCW_TOL.

Tolerance of Tcw: tests/pose_opt_spread.py measures the largest pose-entry difference between
the summation orders over these scenes: 9.88e-15.  8 x that, 7.9e-14, is far below float
resolution, so the floor decides: 2 float32 ulps of the entry's magnitude.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import pose_opt_model as M

pytestmark = pytest.mark.gpu

POSE_SPREAD = 9.88e-15          # python tests/pose_opt_spread.py
TCW_TOL = 8 * POSE_SPREAD       # floor: 2 float32 ulps of the entry


@functools.lru_cache(maxsize=None)
def ref(name):
    sc = M.scene(name)
    vs = M.variants(sc)
    return sc, vs


def assert_guard(name):
    sc, vs = ref(name)
    ok, why = M.guard(vs)
    assert ok, (name, why)
    assert M.scene_extra(name, vs[0]), name
    return sc, vs[0]


@pytest.fixture(scope="module")
def opt(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import PoseOptimizer
    o = PoseOptimizer()
    yield o
    o.close()


def pack(scenes):
    """Frames of one camera into batch arrays: a shared MapPoint table, ids offset per frame
    (-1 / negative ids stay, ids outside a frame's table go outside the shared one)."""
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    B = len(scenes)
    cap = max(s["cap"] for s in scenes)
    total = sum(len(s["pos"]) for s in scenes)
    kps = np.zeros((B, cap), KEYPOINT_DTYPE)
    ur = np.full((B, cap), -1.0, np.float32)
    mp = np.full((B, cap), -1, np.int32)
    n = np.zeros(B, np.int32)
    tcw = np.zeros((B, 12), np.float32)
    pos = np.concatenate([s["pos"] for s in scenes]).astype(np.float32)
    off = 0
    for b, s in enumerate(scenes):
        c = s["cap"]
        kps["x"][b, :c], kps["y"][b, :c], kps["octave"][b, :c] = s["keys_xy"][:, 0], s["keys_xy"][:, 1], s["octave"]
        if s["u_right"] is not None:
            ur[b, :c] = s["u_right"]
        ids = s["mp"].astype(np.int64)
        mp[b, :c] = np.where(ids < 0, ids, np.where(ids < len(s["pos"]), ids + off, total + 7 + ids))
        n[b] = s["n"]
        tcw[b] = s["tcw"]
        off += len(s["pos"])
    stereo = any(s["u_right"] is not None for s in scenes)
    assert len({s["cam"] for s in scenes}) == 1
    return dict(kps=kps, ur=ur if stereo else None, mp=mp, n=n, tcw=tcw, pos=pos, cap=cap, cam=scenes[0]["cam"])


def run_batch(opt, scenes, discard=False, mp_obs=None, want_map=False, trace=True, outlier_init=0, io=None, decoy=None):
    """io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    call); decoy: the scenes whose arrays fill the inputs before an ordered run's real uploads."""
    import torch

    import stream_order as SO
    P = pack(scenes)
    Q = P if decoy is None else pack(decoy)
    B, cap = len(scenes), P["cap"]
    dev = torch.device("cuda", opt.device)
    io = io or SO.SyncIO(dev)
    t = lambda k: io.up(P[k], Q[k])  # noqa: E731
    d_kps = io.up(P["kps"].view(np.uint8).reshape(B, cap * 28), Q["kps"].view(np.uint8).reshape(B, cap * 28))
    d_mp = t("mp")
    d_out = io.full((B, cap), outlier_init, torch.uint8)
    d_tout = io.full((B, 12), float("nan"), torch.float32)
    d_ninl = io.full((B,), -9, torch.int32)
    d_nini = io.full((B,), -9, torch.int32)
    d_tr = io.full((B, 4, 2), -9, torch.int32) if trace else None
    d_map = io.full((B,), -9, torch.int32) if want_map else None
    fx, fy, cx, cy, bf = P["cam"]
    d_n, d_pos, d_tcw = t("n"), t("pos"), t("tcw")
    d_ur = None if P["ur"] is None else t("ur")
    d_obs = None if mp_obs is None else io.up(mp_obs)
    sig = io.host(np.asarray(M.INV_SIGMA2, np.float32), np.asarray(M.INV_SIGMA2, np.float32)[::-1])
    io.begin()
    opt.pose_optimization_batch_device(
        d_kps, d_n, d_mp, d_pos, sig, fx, fy, cx, cy, bf, d_tcw, d_tout, d_out, d_ninl,
        d_nini, d_u_right=d_ur, d_trace=d_tr, discard_outliers=discard,
        d_mp_obs=d_obs, d_nmatches_map=d_map, stream=io.stream)
    io.end()
    return dict(Tcw=io.down(d_tout), outlier=io.down(d_out), ninliers=io.down(d_ninl),
                ninit=io.down(d_nini), trace=io.down(d_tr),
                mp=io.down(d_mp), nmap=io.down(d_map), packed=P)


def assert_pose_close(got, want32, want64, what):
    """8 x the measured spread between summation orders, floor 2 float32 ulps of the entry."""
    got = np.asarray(got, np.float32)
    tol = np.maximum(TCW_TOL, 2 * np.spacing(np.abs(want32).astype(np.float32)).astype(np.float64))
    diff = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    assert np.isfinite(got).all(), what
    assert (diff <= tol).all(), (what, float(diff.max()), got.tolist(), want32.tolist(), want64.tolist())


def assert_frame(got, b, sc, r, what):
    n = sc["n"]
    print(f"{what}: trace {got['trace'][b].tolist()} model {r['trace'].tolist()} ninliers {got['ninliers'][b]} "
          f"model {r['ninliers']} max |dTcw| {np.abs(got['Tcw'][b].astype(np.float64) - r['Tcw']).max():.3g}")
    assert got["ninit"][b] == r["ninit"], what
    assert np.array_equal(got["trace"][b], r["trace"]), (what, got["trace"][b].tolist(), r["trace"].tolist())
    assert np.array_equal(got["outlier"][b, :n], r["outlier"]), what
    assert not got["outlier"][b, n:].any(), what
    assert got["ninliers"][b] == r["ninliers"], what
    assert_pose_close(got["Tcw"][b], r["Tcw"], r["Tcw64"], what)


ALL = sorted(M.scene_specs())


@pytest.mark.parametrize("name", ALL)
def test_single_frame_batch_equals_model(opt, name):
    sc, r = assert_guard(name)
    got = run_batch(opt, [sc])
    assert_frame(got, 0, sc, r, name)
    if r["ninit"] < 3:  # cc:428: the pose bytes untouched
        assert got["Tcw"][0].tobytes() == sc["tcw"].tobytes()
    assert np.array_equal(got["mp"], got["packed"]["mp"])  # frame_mp is written only by the epilogue


def test_edge_kinds_and_table_ids_are_what_the_names_say():
    for name in ("mono-257", "stereo-257", "mixed-257"):
        sc, r = assert_guard(name)
        kind = name.split("-")[0]
        frac = r["stereo"].mean()
        assert (frac == 0.0) if kind == "mono" else (frac == 1.0) if kind == "stereo" else (0.5 < frac < 0.8)
        ids = sc["mp"][:sc["n"]]
        assert (ids == -1).any() and (ids < -1).any() and (ids >= len(sc["pos"])).any()
        assert r["ninit"] == 257 < sc["n"]


def test_batch_of_16_equals_model_and_is_deterministic(opt):
    scenes, refs = [], []
    for name in M.BATCH16:
        sc, r = assert_guard(name)
        scenes.append(sc)
        refs.append(r)
    assert len(scenes) == 16 and len({r["ninit"] for r in refs}) == 16
    assert 0 in {r["ninit"] for r in refs} and 2 in {r["ninit"] for r in refs}
    a = run_batch(opt, scenes)
    for b, (sc, r) in enumerate(zip(scenes, refs)):
        assert_frame(a, b, sc, r, M.BATCH16[b])
    again = run_batch(opt, scenes)
    for k in ("Tcw", "outlier", "ninliers", "ninit", "trace"):
        assert a[k].tobytes() == again[k].tobytes(), k
    # a frame alone gives the bytes it gives inside the batch
    for b in (3, 8, 10, 12, 14, 15):
        one = run_batch(opt, [scenes[b]])
        c = scenes[b]["cap"]
        assert one["Tcw"][0].tobytes() == a["Tcw"][b].tobytes(), M.BATCH16[b]
        assert one["trace"][0].tobytes() == a["trace"][b].tobytes()
        assert one["outlier"][0].tobytes() == a["outlier"][b, :c].tobytes()
        assert one["ninliers"][0] == a["ninliers"][b] and one["ninit"][0] == a["ninit"][b]


@pytest.mark.parametrize("name", ["mixed-2", "mono-9", "mixed-257", "stereo-1985", "mixed-out30"])
def test_single_host_call_equals_batch_bytes(opt, name):
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    sc, r = assert_guard(name)
    got = run_batch(opt, [sc])
    n = sc["n"]
    keys = np.zeros(n, KEYPOINT_DTYPE)
    keys["x"], keys["y"], keys["octave"] = sc["keys_xy"][:n, 0], sc["keys_xy"][:n, 1], sc["octave"][:n]
    fx, fy, cx, cy, bf = sc["cam"]
    ur = None if sc["u_right"] is None else sc["u_right"][:n]
    h = opt.PoseOptimization(keys, ur, sc["mp"][:n], sc["pos"], M.INV_SIGMA2, fx, fy, cx, cy, bf, sc["tcw"])
    assert h["Tcw"].tobytes() == got["Tcw"][0].tobytes()
    assert h["outlier"].tobytes() == got["outlier"][0, :n].tobytes()
    assert h["trace"].tobytes() == got["trace"][0].tobytes()
    assert h["ninliers"] == got["ninliers"][0] == r["ninliers"] and h["ninit"] == got["ninit"][0]
    assert opt.last_call_us() > 0


def test_epilogue_discards_outliers_and_counts_map_matches(opt):
    """Tracking.cc:1004-1017 applied to the model's flags; flags of keypoints without a
    MapPoint are left as they were."""
    names = ["mixed-out30", "mixed-2", "mixed-257", "mixed-0"]
    scenes, refs = zip(*[assert_guard(nm) for nm in names])
    P = pack(scenes)
    rng = np.random.default_rng(5)
    obs = rng.integers(0, 3, len(P["pos"])).astype(np.int32)      # a third with Observations() == 0
    for discard, with_obs in ((True, True), (False, True), (True, False)):
        got = run_batch(opt, scenes, discard=discard, mp_obs=obs if with_obs else None, want_map=True, trace=False,
                        outlier_init=1)
        for b, (sc, r) in enumerate(zip(scenes, refs)):
            n = sc["n"]
            flags = np.ones(P["cap"], np.uint8)
            has = (P["mp"][b] >= 0) & (P["mp"][b] < len(P["pos"]))
            has[n:] = False
            flags[has] = 0
            flags[:n][r["outlier"].astype(bool)] = 1
            mp_in = np.where(has, P["mp"][b], -1)
            want_mp, want_flags, want_map = M.epilogue(mp_in, len(P["pos"]), np.where(has, flags, 0),
                                                       obs if with_obs else None, discard)
            assert np.array_equal(got["mp"][b][has], want_mp[has]), (names[b], discard)
            assert np.array_equal(got["mp"][b][~has], P["mp"][b][~has])
            assert np.array_equal(got["outlier"][b][has], want_flags[has]), (names[b], discard)
            assert (got["outlier"][b][~has] == 1).all()
            assert got["nmap"][b] == want_map, (names[b], discard, with_obs)
            assert got["ninliers"][b] == r["ninliers"]
        assert got["nmap"][0] > 0 and refs[0]["outlier"].any()


def test_rejected_trials_show_in_the_trace(opt):
    sc, r = assert_guard("mixed-off3")
    got = run_batch(opt, [sc])
    assert (got["trace"][0][:, 1] > got["trace"][0][:, 0]).any()  # more solves than iterations: rejections
    assert np.array_equal(got["trace"][0], r["trace"])


# ---- the RGB-D pipeline ------------------------------------------------------------------------
PIPE_SEED = 4160   # the first scene seed (of 4100..4269) whose 8 frames all satisfy guard()
PIPE_B = 8
PIPE_PARAMS = (1000, 1.2, 8, 20, 7)


def _run_pipeline(pose_opt):
    import torch

    import tum_rgbd_scenes as S
    from orbslam2commentedbyxcm_amd.extractor import device_frames
    from orbslam2commentedbyxcm_amd.rgbd import RGBDSequencePipeline
    gray, depth, T = S.sequence(PIPE_SEED, PIPE_B, workers=8)
    pl = RGBDSequencePipeline(PIPE_B, S.W, S.H, S.FX, S.FY, S.CX, S.CY, S.DIST, S.BF, params=PIPE_PARAMS,
                              pose_opt=pose_opt)
    d_gray, d_depth, d_T = device_frames(gray, pl.dev), torch.from_numpy(depth).to(pl.dev), torch.from_numpy(T).to(pl.dev)
    pl.set_tracked(None, None)
    pl.run(d_gray, d_T, 1, d_depth)
    torch.cuda.synchronize(pl.dev)
    pl.set_tracked(*pl.tracked_from(S.tracked_mask(PIPE_SEED, PIPE_B, pl.cap)))
    pl.run(d_gray, d_T, 2, d_depth)
    torch.cuda.synchronize(pl.dev)
    keys = set(pl.results())
    h = pl.host_results()
    sig = pl.exs[0].GetInverseScaleSigmaSquares()
    pl.close()
    return h, keys, T, sig


def test_rgbd_pipeline_pose_opt(orbx_built):
    """RGBDSequencePipeline(pose_opt=True) at 640x480 x 1000 x 8, B = 8: every frame's Tcw_opt,
    flags and counts against the model fed the pipeline's own mvKeysUn, mvuRight, cur_mp and
    LastFrame MapPoints; with the flag off the results are the same bytes and hold no new key."""
    import tum_rgbd_scenes as S
    on, keys_on, T, sig = _run_pipeline(True)
    off, keys_off, _, _ = _run_pipeline(False)
    new = {"Tcw_opt", "outlier", "ninliers", "ninit", "nmatches_map"}
    assert keys_on - keys_off == new and not (keys_off & new)
    assert off["n"].tobytes() == on["n"].tobytes()
    for k in off:  # slots past a frame's keypoint count are never written
        if off[k].ndim == 1:
            assert off[k].tobytes() == on[k].tobytes(), k
        else:
            for b in range(PIPE_B):
                assert off[k][b][:off["n"][b]].tobytes() == on[k][b][:on["n"][b]].tobytes(), (k, b)
    pos = on["mp_pos"].reshape(-1, 3)
    obs = on["mp_obs"].reshape(-1)
    assert on["nm"][1:].min() >= 20 and on["nmatches_map"][1:].min() > 0
    for b in range(PIPE_B):
        n = int(on["n"][b])
        kp = on["kpu"][b][:n]
        xy = np.stack([kp["x"], kp["y"]], axis=1)
        vs = [M.pose_optimization(xy, kp["octave"], on["ur"][b][:n], on["mp"][b][:n], pos, sig, S.FX, S.FY, S.CX, S.CY,
                                  S.BF, T[b], o) for o in M.ORDERS]
        ok, why = M.guard(vs)
        assert ok, (b, why)
        r = vs[0]
        assert on["ninit"][b] == r["ninit"] == int((on["mp"][b][:n] >= 0).sum()), b
        assert np.array_equal(on["outlier"][b][:n], r["outlier"]) and not on["outlier"][b][n:].any(), b
        assert on["ninliers"][b] == r["ninliers"], b
        assert_pose_close(on["Tcw_opt"][b], r["Tcw"], r["Tcw64"], f"frame {b}")
        _, _, nmap = M.epilogue(on["mp"][b][:n], len(pos), r["outlier"], obs, False)
        assert on["nmatches_map"][b] == nmap, b
        if r["ninit"] < 3:
            assert on["Tcw_opt"][b].tobytes() == T[b].tobytes()
