"""orbx_optimize_sim3(_batch_device) on the GPU against tests/optimize_sim3_model.py.

Scenes (optimize_sim3_model.SPECS): points 1.5-8 m away, TUM1 intrinsics (KITTI's for pKF2 in
k1k2-150), octaves 0-7 with invSigma2 = 1.2^(-2 octave), pixel noise 1 px x scale, a start 2 deg /
5 cm / 3 % off, th2 = 10, fixed seeds.  Pair counts 0, 9, 10 and 11 with one gross outlier
(the early exits), 63 / 64 / 65 (wave), 255 / 256 / 257 (the workgroup's stride), one sparse row
(cap1 2000, 300 pairs among 1900 slots); fix_scale 0 and 1; slots with mp1 -1, matches12 -1 /
negative / outside the table, idx2 -1 and >= n2 interleaved with the kept ones; one scene with
no rejection (clean-150) and several with many.

Every comparison first asserts the conditions on its scene (optimize_sim3_model.guard): the
model's twelve variants -- four summation orders x three roundings of the probes' exp() --
agree on the whole LM trace, on both classifications and on the counts, and every chi2 at
both classifications is further from th2 than 1000 x the largest chi2 difference between
them.  Then matches12, ninliers, ncorr, nbad and the trace are equal to the model's and S12 is
within S12_TOL.

Tolerance of S12: tests/optimize_sim3_spread.py measures the largest R12 / t12 / s12 entry
difference between the variants over these scenes: 6.22e-8 (S12_SPREAD; the numeric Jacobian's
1e-9 step leaves H and b with a relative rounding error near 1e-7, far above the analytic
Jacobian's 1e-14 of PoseOptimization).  The tolerance is 8 x that, 4.98e-7, floor 2 float32 ulps
of the entry.  On the MI355X the largest difference to the model's double result was 5.8e-8.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import optimize_sim3_model as M

pytestmark = pytest.mark.gpu

S12_SPREAD = 6.22e-8              # python tests/optimize_sim3_spread.py
S12_TOL = 8 * S12_SPREAD        # floor: 2 float32 ulps of the entry


@functools.lru_cache(maxsize=None)
def assert_guard(name):
    sc = M.scene(name)
    vs = M.scene_variants(name)
    ok, why = M.guard(vs)
    assert ok, (name, why)
    assert M.scene_extra(name, vs[0]), name
    return sc, vs[0]


@pytest.fixture(scope="module")
def opt(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import Sim3Optimizer
    o = Sim3Optimizer()
    yield o
    o.close()


keypoints, pack = M.keypoints, M.pack


def run_batch(opt, scenes, trace=True, counts=True, io=None, decoy=None):
    """io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    call); decoy: the scenes whose arrays fill the inputs before an ordered run's real uploads."""
    import torch

    import stream_order as SO
    P = pack(scenes)
    Q = P if decoy is None else pack(decoy)
    B, cap1, cap2 = len(scenes), P["cap1"], P["cap2"]
    dev = torch.device("cuda", opt.device)
    io = io or SO.SyncIO(dev)
    t = lambda k: io.up(P[k], Q[k])  # noqa: E731
    kp = lambda k, cap: io.up(P[k].view(np.uint8).reshape(B, cap * 28), Q[k].view(np.uint8).reshape(B, cap * 28))  # noqa: E731
    d_m12 = t("m12")
    d_R = io.full((B, 9), float("nan"), torch.float32)
    d_t = io.full((B, 3), float("nan"), torch.float32)
    d_s = io.full((B,), float("nan"), torch.float32)
    i32 = lambda *shape: io.full(shape, -9, torch.int32)  # noqa: E731
    d_nin, d_nc, d_nb = (i32(B), i32(B), i32(B)) if counts else (None, None, None)
    d_tr = i32(B, 2, 2) if trace else None
    s0 = scenes[0]
    ins = [kp("kps1", cap1), t("n1"), t("mp1"), d_m12, t("idx2"), kp("kps2", cap2), t("n2"), t("pos"), t("Tcw1"), t("Tcw2")]
    start = [t("R12"), t("t12"), t("s12")]
    sig1 = io.host(np.asarray(s0["inv_sigma2_1"], np.float32), np.asarray(s0["inv_sigma2_1"], np.float32)[::-1])
    sig2 = io.host(np.asarray(s0["inv_sigma2_2"], np.float32), np.asarray(s0["inv_sigma2_2"], np.float32)[::-1])
    K1, K2 = (io.host(np.asarray(s0[k], np.float32), np.asarray(s0[k], np.float32) * np.float32(1.02)) for k in ("K1", "K2"))
    io.begin()
    opt.optimize_sim3_batch_device(
        *ins, sig1, sig2, K1, K2, *start,
        float(s0["th2"]), s0["fix_scale"], d_R, d_t, d_s, d_ninliers=d_nin, d_ncorr=d_nc, d_nbad=d_nb, d_trace=d_tr,
        stream=io.stream)
    io.end()
    return dict(R12=io.down(d_R), t12=io.down(d_t), s12=io.down(d_s), m12=io.down(d_m12), ninliers=io.down(d_nin),
                ncorr=io.down(d_nc), nbad=io.down(d_nb), trace=io.down(d_tr), packed=P)


def s12_of(got, b):
    return np.concatenate([got["R12"][b], got["t12"][b], [got["s12"][b]]]).astype(np.float32)


def assert_s12_close(got13, r, what):
    """8 x the measured spread between the variants, floor 2 float32 ulps of the entry."""
    want32 = np.concatenate([r["R12"], r["t12"], [r["s12"]]]).astype(np.float32)
    tol = np.maximum(S12_TOL, 2 * np.spacing(np.abs(want32)).astype(np.float64))
    diff = np.abs(got13.astype(np.float64) - want32.astype(np.float64))
    assert np.isfinite(got13).all(), what
    assert (diff <= tol).all(), (what, float(diff.max()), got13.tolist(), want32.tolist(), r["S64"].tolist())


def want_matches(P, b, sc, r):
    """The packed matches12 row with the model's rejections applied."""
    want = P["m12"][b].copy()
    n1 = sc["n1"]
    want[:n1][r["matches12"] != np.asarray(sc["matches12"][:n1], np.int32)] = -1
    return want


def assert_candidate(got, b, sc, r, what):
    print(f"{what}: trace {got['trace'][b].reshape(-1).tolist()} model {r['trace'].reshape(-1).tolist()} ninliers "
          f"{got['ninliers'][b]} model {r['ninliers']} nbad {got['nbad'][b]} model {r['nbad']} max |dS12| "
          f"{np.abs(s12_of(got, b).astype(np.float64) - r['S64']).max():.3g}")
    assert got["ncorr"][b] == r["ncorr"] == sc["npairs"], what
    assert np.array_equal(got["trace"][b], r["trace"]), (what, got["trace"][b].tolist(), r["trace"].tolist())
    assert got["nbad"][b] == r["nbad"], what
    assert np.array_equal(got["m12"][b], want_matches(got["packed"], b, sc, r)), what
    assert got["ninliers"][b] == r["ninliers"], what
    assert_s12_close(s12_of(got, b), r, what)


@pytest.mark.parametrize("name", M.ALL_SCENES)
def test_single_candidate_batch_equals_model(opt, name):
    sc, r = assert_guard(name)
    got = run_batch(opt, [sc])
    assert_candidate(got, 0, sc, r, name)
    if r["ncorr"] - r["nbad"] < 10:  # cc:1331: return 0, S12's bytes untouched
        assert got["ninliers"][0] == 0
        assert s12_of(got, 0).tobytes() == np.concatenate([sc["R12"], sc["t12"], [sc["s12"]]]).astype(
            np.float32).tobytes()


def test_scenes_are_what_their_names_say():
    sc, r = assert_guard("sparse-300-free")
    n1 = sc["n1"]
    assert sc["cap1"] == 2000 and n1 == 1900 and r["ncorr"] == 300
    hole = np.ones(n1, bool)
    hole[sc["slots"]] = False
    n_mp = len(sc["mp_pos"])
    assert (sc["mp1"][:n1][hole] == -1).any() and (sc["matches12"][:n1][hole] == -1).any()
    assert (sc["matches12"][:n1][hole] < -1).any() and (sc["matches12"][:n1][hole] >= n_mp).any()
    assert (sc["idx2"][:n1][hole] == -1).any() and (sc["idx2"][:n1][hole] >= sc["n2"]).any()
    _, clean = assert_guard("clean-150-free")
    assert clean["nbad"] == 0 and clean["ninliers"] == 150 and clean["trace"][1, 0] > 0
    _, many = assert_guard("out-150-fix")
    assert many["nbad"] >= 5
    sc, _ = assert_guard("k1k2-150-free")
    assert not np.array_equal(sc["K1"], sc["K2"])
    # gross outliers are among the rejected entries
    sc, r = assert_guard("out-150-free")
    n1 = sc["n1"]
    assert (r["matches12"][sc["gross"][:n1]] == -1).all()


@pytest.mark.parametrize("fix", ["free", "fix"])
def test_batch_of_16_equals_model_and_is_deterministic(opt, fix):
    names = [f"{k}-{fix}" for k in M.BATCH16 if f"{k}-{fix}" in M.SEEDS]
    names = (names + names)[:16]
    scenes, refs = zip(*[assert_guard(nm) for nm in names])
    assert len(scenes) == 16
    a = run_batch(opt, scenes)
    for b, (sc, r) in enumerate(zip(scenes, refs)):
        assert_candidate(a, b, sc, r, names[b])
    again = run_batch(opt, scenes)
    for k in ("R12", "t12", "s12", "m12", "ninliers", "ncorr", "nbad", "trace"):
        assert a[k].tobytes() == again[k].tobytes(), k
    # a candidate alone gives the bytes it gives inside the batch
    for b in (1, 4, 6, 9, 11):
        one = run_batch(opt, [scenes[b]])
        c = scenes[b]["cap1"]
        assert s12_of(one, 0).tobytes() == s12_of(a, b).tobytes(), names[b]
        assert one["trace"][0].tobytes() == a["trace"][b].tobytes()
        want = want_matches(one["packed"], 0, scenes[b], refs[b])
        assert np.array_equal(one["m12"][0], want) and np.array_equal(a["m12"][b][:c] == -1, want == -1)
        assert (one["ninliers"][0], one["ncorr"][0], one["nbad"][0]) == (a["ninliers"][b], a["ncorr"][b], a["nbad"][b])


def test_optional_outputs_may_be_null(opt):
    sc, r = assert_guard("n65-free")
    full = run_batch(opt, [sc])
    lean = run_batch(opt, [sc], trace=False, counts=False)
    assert s12_of(lean, 0).tobytes() == s12_of(full, 0).tobytes()
    assert lean["m12"].tobytes() == full["m12"].tobytes()


@pytest.mark.parametrize("name", ["n0-free", "n9-fix", "n10-out1-free", "n65-fix", "n257-free", "sparse-300-free"])
def test_single_host_call_equals_batch_bytes(opt, name):
    sc, r = assert_guard(name)
    got = run_batch(opt, [sc])
    n1, n2 = sc["n1"], sc["n2"]
    h = opt.OptimizeSim3(keypoints(sc["k1_xy"][:n1], sc["k1_oct"][:n1]), sc["mp1"][:n1], sc["matches12"][:n1],
                         sc["idx2"][:n1], keypoints(sc["k2_xy"][:n2], sc["k2_oct"][:n2]), sc["mp_pos"], sc["Tcw1"],
                         sc["Tcw2"], sc["inv_sigma2_1"], sc["inv_sigma2_2"], sc["K1"], sc["K2"], sc["R12"], sc["t12"],
                         sc["s12"], sc["th2"], sc["fix_scale"])
    assert np.concatenate([h["R12"], h["t12"], [h["s12"]]]).astype(np.float32).tobytes() == s12_of(got, 0).tobytes()
    assert np.array_equal(h["matches12"], r["matches12"])
    assert np.array_equal(h["matches12"] == -1, got["m12"][0, :n1] == -1)
    assert h["trace"].tobytes() == got["trace"][0].tobytes()
    assert (h["ninliers"], h["ncorr"], h["nbad"]) == (got["ninliers"][0], got["ncorr"][0], got["nbad"][0])
    assert h["ninliers"] == r["ninliers"]
    assert opt.last_call_us() > 0


def test_chain_from_sim3_solver_device_buffers(opt):
    """orbx_sim3_iterate_device's best_R / best_t / best_s device buffers go straight in as R12 /
    t12 / s12: Sim3Solver on the candidate's own pairs, then the refinement from its result.
    Both models' guards hold for this candidate and these draws (chosen on the CPU)."""
    import torch

    import sim3_model as S
    from orbslam2commentedbyxcm_amd.sim3 import Sim3Solver
    name, draws_seed = M.CHAIN
    sc, _ = assert_guard(name)
    s3 = M.sim3_solver_scene(sc, draws_seed)
    ok, why, _ = S.guard(s3)
    assert ok, why
    dev = torch.device("cuda", opt.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    Pk = S.pack([s3])
    solver = Sim3Solver(max_batch=1, cap=Pk["cap"], max_iterations=s3["max_iterations"])
    stream = torch.cuda.current_stream(dev)
    solver.set_batch_device(t(Pk["n1"]), t(Pk["mp1"]), t(Pk["mp2"]), t(Pk["oct1"]), t(Pk["oct2"]), t(Pk["pos"]),
                            t(Pk["Tcw1"]), t(Pk["Tcw2"]), s3["level_sigma2"], s3["K1"], s3["K2"], t(Pk["draws"]),
                            fix_scale=s3["fix_scale"], probability=s3["probability"], min_inliers=s3["min_inliers"],
                            max_iterations=s3["max_iterations"], stream=stream)
    d_R = torch.zeros((1, 9), dtype=torch.float32, device=dev)
    d_t = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    d_s = torch.zeros((1,), dtype=torch.float32, device=dev)
    d_found = torch.zeros((1,), dtype=torch.int32, device=dev)
    solver.iterate_batch_device(s3["max_iterations"], stream=stream, best_R=d_R, best_t=d_t, best_s=d_s, found=d_found)
    P = pack([sc])
    d_m12 = t(P["m12"])
    d_Ro, d_to, d_so = torch.zeros_like(d_R), torch.zeros_like(d_t), torch.zeros_like(d_s)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    d_nin, d_nc, d_nb, d_tr = i32(1), i32(1), i32(1), i32(1, 2, 2)
    opt.optimize_sim3_batch_device(
        t(P["kps1"].view(np.uint8).reshape(1, -1)), t(P["n1"]), t(P["mp1"]), d_m12, t(P["idx2"]),
        t(P["kps2"].view(np.uint8).reshape(1, -1)), t(P["n2"]), t(P["pos"]), t(P["Tcw1"]), t(P["Tcw2"]),
        sc["inv_sigma2_1"], sc["inv_sigma2_2"], sc["K1"], sc["K2"], d_R, d_t, d_s, float(sc["th2"]), sc["fix_scale"],
        d_Ro, d_to, d_so, d_ninliers=d_nin, d_ncorr=d_nc, d_nbad=d_nb, d_trace=d_tr, stream=stream)
    torch.cuda.synchronize(dev)
    solver.close()
    assert int(d_found.cpu()[0]) == 1
    start = dict(best_R=d_R.cpu().numpy()[0], best_t=d_t.cpu().numpy()[0], best_s=d_s.cpu().numpy()[0])
    want = S.run(s3, ["find"])[0][0]
    for k in ("best_R", "best_t", "best_s"):   # test_gpu_sim3.py's tolerance: 2 float32 ulps
        w = np.asarray(want[k], np.float64).reshape(-1).astype(np.float32)
        assert (np.abs(start[k].reshape(-1) - w) <= 2 * np.spacing(np.abs(w))).all(), k
    fed = M.chain_start(sc, start)
    vs = M.variants(fed)
    ok, why = M.guard(vs)
    assert ok, why
    r = vs[0]
    got = dict(R12=d_Ro.cpu().numpy(), t12=d_to.cpu().numpy(), s12=d_so.cpu().numpy(), m12=d_m12.cpu().numpy(),
               ninliers=d_nin.cpu().numpy(), ncorr=d_nc.cpu().numpy(), nbad=d_nb.cpu().numpy(),
               trace=d_tr.cpu().numpy(), packed=P)
    assert r["ninliers"] >= 20 and r["trace"][1, 0] > 0
    assert_candidate(got, 0, fed, r, "chain")
