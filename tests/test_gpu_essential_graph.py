"""orbx_optimize_essential_graph(_batch_device) on the GPU against tests/essential_graph_model.py.

Scenes (essential_graph_model.SPECS): closed trajectories with keyframes 0.3 m apart whose
estimates drifted, the last keyframes corrected as CorrectLoop leaves them, kind-0 edges from the
corrected keyframes to the loop's side, kind-1 spanning-tree, loop and covisibility edges, 3
points per keyframe that refer to corrected, uncorrected and the fixed keyframe.  2 and 3
keyframes; 9 with a free and with a fixed scale; 63 / 64 / 65 vertices that may move (wave) and
257 (the workgroup's stride; a covisibility band of 3 and three loop edges: short and long
envelope columns); the fixed keyframe in the middle with repeated and reversed pairs; a keyframe
without an edge; bad edges and point references interleaved with good ones; tiny and large start
errors.  The drift of the scenes that are compared over 4 iterations is far larger than a real
loop's (60 degrees, 60 % of a step per keyframe): with a real loop's few degrees the
optimisation has converged to rounding noise by the third iteration and nothing after it can be
compared (essential_graph_model.guard fails).

Every comparison first asserts essential_graph_model.guard at its iteration count k: the
model's twelve variants take the same accept / reject decisions and every trial's
|currentChi - tempChi| is at least 1000 x its largest difference between the variants.  Then
the trace and the status at k equal the model's.  The full 20 iterations decide on rounding noise
once converged, so their trace is not compared.

Estimates: at k and at 20 iterations Tcw_opt and pt_pos_opt are within 8 x the spread between the
variants that tests/essential_graph_spread.py measures at that count (SPREAD below), floor 2
float32 ulps of the entry; the final chi2 within 8 x the variants' relative chi2 spread.  Where the
model's final chi2 is below ZERO_CHI2 x the initial one (pair, whose single edge is met exactly: the
variants' chi2 are rounding noise there and their relative spread is near 1) the device's must be
below it too.
Measured spread (per scene, SPREAD below): pose entries 2e-9 to 4e-7 for the scenes of up to 9
keyframes, 1.5e-6 to 4.7e-6 for the rings of 63-65, 1.8e-4 for ring-257 (258 keyframes, 60 degrees
of drift); positions up to 3.9e-4 (ring-257), 1.2e-5 next; the final chi2 relatively up to 6.3e-7.
On the MI355X every trace and status equal the model's; the largest difference of a device float
to the model's double was 1.7e-4 for a pose entry and 2.8e-4 for a position (ring-257), 7.4e-6 /
1.9e-5 for the rings of 63-65, at most 3.3e-7 / 2.0e-6 elsewhere; the final chi2 differed
relatively by 6.0e-7 (ring-257) and 1e-7 (tiny) at most.  DESIGN.md §4.22.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import essential_graph_model as M

pytestmark = pytest.mark.gpu

# python tests/essential_graph_spread.py, per scene at its k and at 20 iterations: the largest
# difference between the variants of (a pose entry, a position entry, the final chi2 relatively)
SPREAD = {
    "pair": {"k": (1.3e-09, 1.55e-09, 0.381), 20: (1.11e-15, 5.33e-15, 0.956)},
    "chain-3": {"k": (1.36e-08, 2.88e-08, 1.25e-10), 20: (3.37e-08, 1.81e-07, 7.57e-14)},
    "ring-9": {"k": (2.06e-09, 1.45e-08, 2.31e-10), 20: (2.06e-09, 1.45e-08, 2.31e-10)},
    "ring-9-fixed-scale": {"k": (4.29e-07, 1.84e-06, 5.81e-10), 20: (2.8e-07, 1.36e-06, 1.37e-10)},
    "ring-63": {"k": (2.45e-06, 5.31e-06, 8e-10), 20: (4.67e-06, 9.29e-06, 5.05e-10)},
    "ring-64": {"k": (3.68e-06, 9.28e-06, 6.4e-09), 20: (4.58e-06, 1.17e-05, 2.11e-09)},
    "ring-65": {"k": (2.05e-06, 5.74e-06, 1.89e-11), 20: (1.47e-06, 5.24e-06, 3.11e-12)},
    "ring-257": {"k": (0.000143, 0.000389, 6.28e-07), 20: (0.000182, 0.000224, 3.5e-07)},
    "fixed-mid": {"k": (2.13e-07, 5.52e-07, 8.34e-11), 20: (1.72e-07, 1.07e-06, 2.27e-11)},
    "isolated": {"k": (3.08e-08, 1.52e-07, 2.37e-09), 20: (4.9e-08, 2.74e-07, 9.73e-12)},
    "bad-edges": {"k": (4.29e-07, 1.84e-06, 5.81e-10), 20: (2.8e-07, 1.36e-06, 1.37e-10)},
    "tiny": {"k": (2.09e-08, 2.18e-08, 6.16e-07), 20: (2.09e-08, 2.18e-08, 6.16e-07)},
    "large": {"k": (3.57e-07, 1.49e-06, 1.33e-10), 20: (4.14e-07, 1.69e-06, 9.74e-11)},
}
SCENES = tuple(M.SPECS)
# A final chi2 below this fraction of the initial one is zero up to rounding: chi2 is a sum of
# squares, so the residual is below 1e-6 of the start's, under the float32 resolution of the outputs.
ZERO_CHI2 = 1e-12


@functools.lru_cache(maxsize=None)
def model(name, iterations):
    k = M.exact_iterations(name)
    ok, why = M.guard(name, k)
    assert ok, (name, why)
    return M.essential_graph(M.scene(name), iterations=iterations)


@pytest.fixture(scope="module")
def opt(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import EssentialGraphOptimizer
    o = EssentialGraphOptimizer()
    yield o
    o.close()


def blocks_of(sc, dense=False):
    return M.envelope(len(sc["Tcw"]), sc["loop"], sc["edge_v"], dense)[2]


def run_batch(opt, scenes, iterations=0, dense=False, max_env_blocks=None, optional=True, io=None, decoy=None):
    """io: a stream_order I/O object (default: blocking uploads, a device synchronise around the
    call); decoy: the scenes whose arrays fill the inputs before an ordered run's real uploads.
    The per-problem rows are views that an ordered run fills when its stream is synchronised."""
    import torch

    import stream_order as SO
    P = M.pack(scenes)
    Q = P if decoy is None else M.pack(decoy)
    B = len(scenes)
    dev = torch.device("cuda", opt.device)
    io = io or SO.SyncIO(dev)
    nk, npt = len(P["Tcw"]), len(P["pos"])
    d_T = io.full((nk, 12), float("nan"), torch.float32)
    d_X = io.full((npt, 3), float("nan"), torch.float32)
    d_st = io.full((B,), -9, torch.int32)
    d_S = io.full((nk, 8), float("nan"), torch.float64) if optional else None
    d_tr = io.full((B, 2), -9, torch.int32) if optional else None
    d_chi = io.full((B, 2), float("nan"), torch.float64) if optional else None
    if max_env_blocks is None:
        max_env_blocks = max(blocks_of(sc, dense) for sc in scenes)
    ins = [io.up(P[k], Q[k]) for k in ("kf_off", "Tcw", "corr", "corr_S", "loop", "edge_off", "edge_v", "edge_kind",
                                       "pt_off", "pos", "pt_ref")]
    io.begin()
    opt.essential_graph_batch_device(
        *ins, bool(scenes[0]["fix_scale"]), max_env_blocks,
        d_T, d_X, d_st, d_Scw_opt=d_S, d_trace=d_tr, d_chi2=d_chi, iterations=iterations, dense=dense,
        stream=io.stream)
    io.end()
    T, X, S, st, tr, chi = (io.down(x) for x in (d_T, d_X, d_S, d_st, d_tr, d_chi))
    out = []
    for b in range(B):
        k0, k1, p0, p1 = P["kf_off"][b], P["kf_off"][b + 1], P["pt_off"][b], P["pt_off"][b + 1]
        out.append(dict(Tcw=T[k0:k1], pos=X[p0:p1], Scw=None if S is None else S[k0:k1], status=st[b:b + 1],
                        trace=None if tr is None else tr[b], chi2=None if chi is None else chi[b]))
    if not io.ordered:
        for o in out:
            o["status"] = int(o["status"][0])
    return out


def run_host(opt, sc, **kw):
    return opt.OptimizeEssentialGraph(sc["Tcw"], sc["corr"], sc["corr_S"], sc["loop"], sc["edge_v"], sc["edge_kind"],
                                      sc["pos"], sc["pt_ref"], sc["fix_scale"], **kw)


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("Tcw", "pos", "Scw", "trace", "chi2")) \
        and a["status"] == b["status"]


def assert_close(got, r, which, what):
    """8 x the scene's measured spread between the variants, floor 2 float32 ulps of the entry."""
    sT, sX, sC = SPREAD[what][which]
    for key, k64, s in (("Tcw", "T64", sT), ("pos", "pos64", sX)):
        want = r[key].astype(np.float64)
        tol = np.maximum(8 * s, 2 * np.spacing(np.abs(r[key])).astype(np.float64))
        diff = np.abs(got[key].astype(np.float64) - want)
        print(f"{what} {key}: max |device - model| {np.abs(got[key].astype(np.float64) - r[k64]).max() if diff.size else 0:.3g}")
        assert np.isfinite(got[key]).all(), (what, key)
        assert (diff <= tol).all(), (what, key, float(diff.max()), float(tol.min()))
    rel = abs(got["chi2"][1] - r["chi2"][1]) / max(abs(r["chi2"][1]), np.finfo(float).tiny)
    print(f"{what} chi2: device {got['chi2'].tolist()} model {r['chi2'].tolist()} relative {rel:.3g}")
    if r["chi2"][1] < ZERO_CHI2 * r["chi2"][0]:
        assert got["chi2"][1] < ZERO_CHI2 * r["chi2"][0], (what, got["chi2"].tolist())
    else:
        assert rel <= max(8 * sC, 2 * np.finfo(float).eps), (what, rel)


@pytest.mark.parametrize("name", SCENES)
def test_trace_and_estimates_at_k(opt, name):
    k = M.exact_iterations(name)
    r = model(name, k)
    got = run_batch(opt, [M.scene(name)], iterations=k)[0]
    print(f"{name}: trace {got['trace'].tolist()} model {r['trace'].tolist()} status {got['status']} hist {r['hist'].tolist()}")
    assert np.array_equal(got["trace"], r["trace"]), (name, got["trace"].tolist(), r["trace"].tolist())
    assert got["status"] == r["status"], name
    assert_close(got, r, "k", name)


@pytest.mark.parametrize("name", SCENES)
def test_estimates_at_20_iterations(opt, name):
    r = model(name, 0)
    got = run_batch(opt, [M.scene(name)])[0]
    print(f"{name}: trace {got['trace'].tolist()} model {r['trace'].tolist()}")
    assert got["status"] == r["status"], name
    assert_close(got, r, 20, name)


@pytest.mark.parametrize("name,iterations", [("ring-9", 0), ("fixed-mid", 0), ("ring-65", 0), ("ring-257", 2)])
def test_envelope_equals_forced_dense(opt, name, iterations):
    sc = M.scene(name)
    env = run_batch(opt, [sc], iterations=iterations)[0]
    dense = run_batch(opt, [sc], iterations=iterations, dense=True)[0]
    assert blocks_of(sc) < blocks_of(sc, True)
    assert env["trace"][0] > 0 and same_bytes(env, dense), name


def test_batch_equals_single_launches_and_host_form(opt):
    names = ["ring-9", "pair", "ring-65", "ring-9"]
    scenes = [dict(M.scene(n), fix_scale=0) for n in names]      # fix_scale is one value per launch
    both = run_batch(opt, scenes)
    for b, sc in enumerate(scenes):
        one = run_batch(opt, [sc])[0]
        assert same_bytes(both[b], one), names[b]
        host = run_host(opt, sc)
        assert same_bytes(both[b], host), names[b]
    assert same_bytes(both[0], both[3])


def test_capacity_no_fixed_kf_and_bad_indices_return_inputs(opt):
    sc = M.scene("ring-9")
    need = blocks_of(sc)
    G = M.Graph(sc)
    for got in (run_batch(opt, [sc], max_env_blocks=need - 1)[0], run_host(opt, sc, max_env_blocks=need - 1)):
        assert got["status"] == M.STATUS_CAPACITY
        assert got["Tcw"].tobytes() == sc["Tcw"].tobytes() and got["pos"].tobytes() == sc["pos"].tobytes()
        assert got["Scw"].tobytes() == G.S0.T.copy().tobytes()
        assert not got["trace"].any() and not got["chi2"].any()
    assert run_batch(opt, [sc], max_env_blocks=need)[0]["status"] == 0
    for loop in (-1, len(sc["Tcw"])):
        got = run_batch(opt, [dict(sc, loop=loop)])[0]
        assert got["status"] == M.STATUS_NO_FIXED_KF
        assert got["Tcw"].tobytes() == sc["Tcw"].tobytes() and got["pos"].tobytes() == sc["pos"].tobytes()
        assert not got["trace"].any()
    bad = M.scene("bad-edges")
    got = run_batch(opt, [bad])[0]
    assert got["status"] == M.STATUS_BAD_INDEX
    out = (bad["pt_ref"] < 0) | (bad["pt_ref"] >= len(bad["Tcw"]))
    assert out.sum() == 2 and got["pos"][out].tobytes() == bad["pos"][out].tobytes()
    # the bad edges are no edges: the same bytes as the scene without them
    G = M.Graph(bad)
    clean = dict(bad, edge_v=bad["edge_v"][G.index], edge_kind=bad["edge_kind"][G.index])
    ref = run_batch(opt, [clean])[0]
    assert got["Tcw"].tobytes() == ref["Tcw"].tobytes() and np.array_equal(got["trace"], ref["trace"])
    # a neighbour in the batch that returns its inputs does not change a problem's bytes
    three = run_batch(opt, [dict(bad, loop=-1), bad, clean])
    assert three[0]["status"] == M.STATUS_NO_FIXED_KF and same_bytes(three[1], got) and same_bytes(three[2], ref)


def test_isolated_keyframe_keeps_its_estimate(opt):
    sc = M.scene("isolated")
    got = run_batch(opt, [sc])[0]
    G = M.Graph(sc)
    assert got["Scw"][-1].tobytes() == G.S0[:, -1].copy().tobytes()


def test_null_optional_outputs(opt):
    sc = M.scene("ring-9")
    full = run_batch(opt, [sc])[0]
    bare = run_batch(opt, [sc], optional=False)[0]
    assert bare["Tcw"].tobytes() == full["Tcw"].tobytes() and bare["pos"].tobytes() == full["pos"].tobytes()
    assert bare["status"] == full["status"] == 0
