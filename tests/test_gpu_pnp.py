"""orbx_pnp_* on the GPU against tests/pnp_model.py.

Scenes (pnp_scenes.SCENES): TUM1 intrinsics, 8 levels at scale 1.2, matched slots interleaved
with -1, negative and out-of-table ids in rows of cap 512; N (valid correspondences) in {3, 4,
9, 10, 11, 63, 64, 65, 100, 257}; Tracking::Relocalization's parameters unless the scene says
otherwise.  By outcome: success at iteration 1 (first_100), success after misses (the blind_*
and noisy_* scenes), Refine fails on a decoy pose with exactly minInliers points, a tie keeps
the earlier iteration and reuses the stored failure, then the best state is replaced and Refine
succeeds (staged_100), never found with no_more by the cap (none_100, behind_64: every point
behind the camera), found unrefined at the cap with Refine failing on every qualifying
iteration and minInliers == N (all_10), N == minInliers == 4 (all_4), no iteration at all
(few_3, few_4, few_9), going on after a return (cont_100), out of draws (nodraws_100), draws out
of range (baddraw_64), a coplanar minimal set and one that holds the same correspondence twice
at iteration 0 with regular draws after (coplanar_64, repeat_64).  What a degenerate set's
hypothesis is hangs on how a singular matrix is decomposed, so the guard leaves that iteration's
own values out of its margins and requires instead that it qualifies in no variant of the model;
nothing the calls return then depends on it, and the device must agree on all of it: were its
degenerate hypothesis to qualify, best_iteration, iterations or the refined result would differ.

Every comparison first asserts its scene's guard (pnp_scenes.guard_for): over every iteration
the test walks, the family-A variants of the model agree on every count, flag and field, and
every error2 / mvMaxError and every rep_errors comparison between different poses is farther
from its threshold than 1000 x the largest relative difference between the variants.  Then
every integer, flag, iterations, best_iteration, refined and status equals the model's, and
Tcw / best_Tcw are within 8 x the scene's own family-A spread, with a floor of 2 float32 ulps
of the entry (the measured spread is 0: the variants give the same floats; python
tests/pnp_spread.py).

Convention-blind scenes are also compared with every family-B variant of the model (PCA axes
and null vectors negated, the minimal sets' null basis rotated): found, inliers and n_inliers
equal, Tcw within 8 x the family-B spread measured over the convention-blind scenes (no
floor), after the guard's part (B): every refined error2 / mvMaxError reached by any variant is
farther from 1 than 1000 x the largest difference of the returned Refine's between the variants.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import pnp_scenes as S

pytestmark = pytest.mark.gpu

INT_KEYS = ("found", "no_more", "n_inliers", "refined", "best_inliers", "best_iteration", "iterations", "n_corr",
            "min_inliers_used", "max_its_used", "status")
FILL = 7          # prefill of the flag rows: entries beyond n keep it
FILL_MP = -77     # prefill of frame_mp
REF_SCENES = [k for k, v in S.SCENES.items() if "params" not in v and "n_draws" not in v]


@pytest.fixture(scope="module")
def solver(orbx_built):
    from orbslam2commentedbyxcm_amd.pnp import PnPsolver
    s = PnPsolver(max_batch=16, cap=S.CAP, max_draws=S.N_DRAWS)
    yield s
    s.close()


def run_batch(solver, names, schedule):
    """set_batch_device on the packed scenes, then the schedule's calls; one dict of host arrays
    per call."""
    import torch
    P = S.pack(names)
    B = len(names)
    dev = torch.device("cuda", solver.device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    stream = torch.cuda.Stream(dev)   # the prefills, the uploads and the library's kernels in one order
    calls = []
    p = P["params"]
    with torch.cuda.stream(stream):
        solver.set_batch_device(t(P["kps"].view(np.uint8).reshape(B, S.CAP, 28)), t(P["n"]), t(P["matches"]),
                                t(P["pos"]), S.SIGMA2, S.K, t(P["draws"]), probability=p["probability"],
                                min_inliers=p["min_inliers"], max_iterations=p["max_iterations"],
                                min_set=p["min_set"], epsilon=p["epsilon"], th2=p["th2"], stream=stream)
        for c in schedule:
            o = {k: torch.full((B,), -9, dtype=torch.int32, device=dev) for k in INT_KEYS}
            o["inliers"] = torch.full((B, S.CAP), FILL, dtype=torch.uint8, device=dev)
            o["frame_mp"] = torch.full((B, S.CAP), FILL_MP, dtype=torch.int32, device=dev)
            o["Tcw"] = torch.full((B, 12), -5.0, dtype=torch.float32, device=dev)
            o["best_Tcw"] = torch.full((B, 12), -5.0, dtype=torch.float32, device=dev)
            solver.iterate_batch_device(int(c), stream=stream, **o)
            calls.append(o)
    stream.synchronize()
    res = [{k: v.cpu().numpy() for k, v in o.items()} for o in calls]
    for r in res:
        r["_offsets"] = P["offsets"]
    return res


def one(res, b):
    return {k: v[b] for k, v in res.items()}


def assert_close(got, want, tol, what, floor=True):
    """NaN where the model has NaN; else within tol, with a floor of 2 float32 ulps of the entry
    where `floor`."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    f = ~np.isnan(want)
    bound = np.full(int(f.sum()), float(tol))
    if floor:
        bound = np.maximum(bound, 2 * np.spacing(np.abs(want[f]).astype(np.float32)).astype(np.float64))
    d = np.abs(got[f].astype(np.float64) - want[f].astype(np.float64))
    assert (d <= bound).all(), (what, d.max(), got, want)


def assert_matches_model(name, got, want, tol, off=0):
    sc = S.scene(name)
    n = sc["n"]
    for k in INT_KEYS:
        assert int(got[k]) == int(want[k]), (name, k, int(got[k]), int(want[k]))
    assert np.array_equal(got["inliers"][:n], want["inliers"]), name
    assert (got["inliers"][n:] == FILL).all() and (got["frame_mp"][n:] == FILL_MP).all(), name
    mp = want["frame_mp"].copy()
    mp[mp >= 0] += off
    assert np.array_equal(got["frame_mp"][:n], mp), name
    assert_close(got["Tcw"], want["Tcw"], tol, (name, "Tcw"))
    assert_close(got["best_Tcw"], want["best_Tcw"], tol, (name, "best_Tcw"))


def schedule_of(name):
    g = S.guard_for(name)
    plan = S.scene(name)["plan"]
    return g, list(plan) if plan is not None else [5] * len(g["outs"])


@pytest.mark.parametrize("name", list(S.SCENES))
def test_parity_under_the_devices_conventions(solver, name):
    g, sched = schedule_of(name)
    res = run_batch(solver, [name], sched)
    assert len(res) == len(g["outs"])
    for r, want in zip(res, g["outs"]):
        assert_matches_model(name, one(r, 0), want, 8 * g["spread_a"])


@pytest.mark.parametrize("name", [k for k, v in S.SCENES.items() if v["blind"]])
def test_convention_blind_parity(solver, name):
    """One find() against every family-B variant.  `iterations` is not compared: the variants'
    hypotheses differ (that is what the family varies), so each stops at another iteration;
    what they return after Refine is what agrees."""
    g = S.guard_for(name)
    spread_b = max(S.guard_for(k)["spread_b"] for k, v in S.SCENES.items() if v["blind"])   # what pnp_spread.py prints
    got = one(run_batch(solver, [name], [300])[0], 0)
    n = S.scene(name)["n"]
    for fam in g["family_b"] + [g["base_b"]]:
        want = fam[-1]
        assert int(got["found"]) == int(want["found"]) and int(got["n_inliers"]) == int(want["n_inliers"]), name
        assert np.array_equal(got["inliers"][:n], want["inliers"]), name
        assert_close(got["Tcw"], want["Tcw"], 8 * spread_b, (name, "Tcw"), floor=False)


def same_bytes(a, b, what):
    for k in a:
        if not k.startswith("_"):
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_bytes_batch_of_16_against_each_alone(solver):
    names = (REF_SCENES * 2)[:16]
    for k in names:
        S.guard_for(k)
    both = run_batch(solver, names, [5, 5])
    for b, name in enumerate(names):
        alone = run_batch(solver, [name], [5, 5])
        for c in range(2):
            x, y = one(both[c], b), one(alone[c], 0)
            mp = y["frame_mp"].copy()
            mp[mp >= 0] += both[c]["_offsets"][b]
            y = dict(y, frame_mp=mp)
            same_bytes({k: v for k, v in x.items() if not k.startswith("_")},
                       {k: v for k, v in y.items() if not k.startswith("_")}, name)


@pytest.mark.parametrize("name", ["coplanar_64", "repeat_64"])
def test_a_degenerate_minimal_set_does_not_qualify(solver, name):
    """Iteration 0 draws a coplanar set / the same correspondence twice: it costs its iteration
    and nothing else, however the call is cut, and the pose found later is the true one."""
    g, sc = S.guard_for(name), S.scene(name)
    assert sc["degenerate"] == (0,)
    first = one(run_batch(solver, [name], [1])[0], 0)      # a first call runs on to the cap (cc:226)
    assert int(first["status"]) == 0 and int(first["found"]) == 1 and int(first["refined"]) == 1
    assert int(first["best_iteration"]) > 0 and int(first["iterations"]) == int(first["best_iteration"]) + 1
    assert int(first["best_iteration"]) == int(g["outs"][0]["best_iteration"])
    T = first["Tcw"].reshape(3, 4)
    # exact keypoints: the refined pose is the true one up to the float32 MapPoints and keypoints (1e-5, as
    # tests/test_pnp_model.py asks of the model on such scenes)
    assert np.abs(T[:, :3] - sc["R"]).max() < 1e-5 and np.abs(T[:, 3] - sc["t"]).max() < 1e-5
    assert set(np.nonzero(first["inliers"][:sc["n"]])[0]) == set(sc["inl_slots"])


@pytest.mark.parametrize("name", ["blind_100", "blind_63", "baddraw_64", "coplanar_64", "repeat_64"])
def test_bytes_whatever_the_first_call_asks_for(solver, name):
    """A first call runs to the cap unless it returns (cc:226), so iterate(1), iterate(5),
    iterate(7) and iterate(300) of a scene that returns below the cap are the same call."""
    S.guard_for(name)
    ref = run_batch(solver, [name], [5])[0]
    assert int(ref["found"][0]) == 1 and int(ref["iterations"][0]) < int(ref["max_its_used"][0])
    for step in (1, 7, 300):
        same_bytes(one(run_batch(solver, [name], [step])[0], 0), one(ref, 0), (name, step))


@pytest.mark.parametrize("name,cuts", [("none_100", ([5, 2], [1, 2], [7, 1], [0, 1, 1])),      # the cap is 6
                                       ("all_10", ([5, 3], [1, 7], [7, 1], [0, 1, 6]))])       # the cap is 1
def test_bytes_however_the_iterations_are_cut(solver, name, cuts):
    """Scenes whose Refine never succeeds, cap below 8: every cut that reaches 8 iterations
    leaves the same outputs (a first call of n runs max(n, cap) iterations, a later one n)."""
    S.guard_for(name)
    ref = run_batch(solver, [name], [8])[-1]
    assert int(ref["iterations"][0]) == 8 and int(ref["max_its_used"][0]) < 8 and int(ref["refined"][0]) == 0
    for cut in cuts:
        same_bytes(one(run_batch(solver, [name], cut)[-1], 0), one(ref, 0), (name, cut))


def test_single_host_call_gives_the_batch_bytes(solver, orbx_built):
    from orbslam2commentedbyxcm_amd.pnp import PnPsolver
    for name in ("blind_100", "noisy_63", "few_3", "all_10", "coplanar_64", "repeat_64"):
        sc = S.scene(name)
        S.guard_for(name)
        p = sc["params"]
        h = PnPsolver(sc["keys"], sc["matches"], sc["pos"], S.SIGMA2, S.K, draws=sc["draws"], cap=S.CAP)
        h.SetRansacParameters(p["probability"], p["min_inliers"], p["max_iterations"], p["min_set"], p["epsilon"],
                              p["th2"])
        dev = run_batch(solver, [name], [5, 5])
        for c in range(2):
            o = h.iterate_host(5)
            d = one(dev[c], 0)
            for k in INT_KEYS:
                assert int(o[k][0]) == int(d[k]), (name, k)
            assert o["Tcw"].tobytes() == d["Tcw"].tobytes() and o["best_Tcw"].tobytes() == d["best_Tcw"].tobytes()
            assert o["inliers"].tobytes() == d["inliers"][:sc["n"]].tobytes()
            assert o["frame_mp"].tobytes() == d["frame_mp"][:sc["n"]].tobytes()
        h.close()


def test_set_resets_the_state(solver):
    S.guard_for("cont_100")
    a = run_batch(solver, ["cont_100"], [5, 5])
    b = run_batch(solver, ["cont_100"], [5, 5])
    for x, y in zip(a, b):
        same_bytes(one(x, 0), one(y, 0), "cont_100")
    assert int(a[1]["iterations"][0]) > int(a[0]["iterations"][0])   # the second call went on


def test_argument_errors_with_a_live_solver(solver):
    import torch

    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda", solver.device)
    P = S.pack(["blind_11"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    keep = [t(P["kps"].view(np.uint8)), t(P["n"]), t(P["matches"]), t(P["pos"]), t(P["draws"])]
    sig = np.ascontiguousarray(S.SIGMA2)

    def batch(**kw):
        q = L.PnpBatch()
        q.batch, q.cap = 1, S.CAP
        q.kps, q.n, q.matches, q.mp_pos, q.draws = (C.c_void_p(x.data_ptr()) for x in keep)
        q.n_mp, q.level_sigma2, q.nlevels = len(P["pos"]), sig.ctypes.data_as(C.POINTER(C.c_float)), 8
        q.fx, q.fy, q.cx, q.cy = (float(v) for v in S.K)
        q.probability, q.min_inliers, q.max_iterations, q.min_set, q.epsilon, q.th2 = 0.99, 10, 50, 4, 0.5, 5.991
        q.n_draws = S.N_DRAWS
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    h = solver._h
    assert lib.orbx_pnp_set_batch_device(h, C.byref(batch()), None) == L.ORBX_OK
    for bad in (dict(min_set=3), dict(min_set=5), dict(cap=S.CAP + 1), dict(max_iterations=S.N_DRAWS + 1),
                dict(n_draws=S.N_DRAWS + 1), dict(kps=None), dict(n=None), dict(matches=None), dict(draws=None),
                dict(mp_pos=None), dict(level_sigma2=None), dict(batch=17), dict(probability=1.0)):
        assert lib.orbx_pnp_set_batch_device(h, C.byref(batch(**bad)), None) == L.ORBX_ERR_ARG, bad
    assert lib.orbx_pnp_set_batch_device(h, None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_pnp_iterate_device(h, 5, None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_pnp_iterate_device(h, -1, C.byref(L.PnpResult()), None) == L.ORBX_ERR_ARG
    assert lib.orbx_pnp_iterate_device(h, 5, C.byref(L.PnpResult()), None) == L.ORBX_OK   # every output is nullable
    torch.cuda.synchronize(dev)
