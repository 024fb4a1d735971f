"""tests/essential_graph_model.py against closed forms and Optimizer::OptimizeEssentialGraph's
schedule (src/Optimizer.cc:873-1150), the host helpers orbx_essential_graph_envelope and
essential_graph_edges on hand-written graphs, and the argument checks of
orbx_optimize_essential_graph*.  No GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import essential_graph_model as M


def _x(omega, upsilon, sigma):
    return np.concatenate([omega, upsilon, [sigma]])


@pytest.mark.parametrize("branch,theta,sigma", [(0, 1e-4, 0.0), (0, 5e-5, 5e-6), (1, 0.3, 0.0), (1, 2.0, -4e-6),
                                                (2, 5e-6, 0.1), (2, 1e-6, -0.3), (3, 0.3, 0.2), (3, 1.5, -0.4)])
def test_log_inverts_exp_in_each_branch(branch, theta, sigma):
    """All four branches of Sim3::log (BRANCHES).  In branch 2 (small rotation, free scale) theta is
    below exp's own threshold of 1e-5, so that exp and log take the same branch with the same B."""
    rng = np.random.default_rng(branch * 10 + int(theta * 100))
    w = rng.normal(size=3)
    x = _x(w / np.linalg.norm(w) * theta, rng.normal(size=3), sigma)
    hist = np.zeros(4, np.int64)
    got = M.s_log(M.s_exp(x)[:, None], hist)[:, 0]
    assert hist[branch] == 1 and hist.sum() == 1
    assert np.abs(got - x).max() < 1e-12


def test_log_and_exp_switch_branches_at_different_rotations():
    """exp takes its small-rotation branch below theta = 1e-5, log below d = 1 - 1e-5, which is
    theta = 4.5e-3.  Between the two, with a free scale, log's B = (0.5 sigma^2 - sigma + 1) s /
    sigma^3 (sim3.h:199; it has no "- 1" and grows like 1 / sigma^3) meets an exp that used the
    large-rotation B: log(exp(x)) is x along omega and in sigma, and across omega the more wrong the
    larger theta^2 / sigma^3 is."""
    x = _x(np.array([1e-3, 0.0, 0.0]), np.array([0.5, 0.0, 0.0]), 0.1)
    hist = np.zeros(4, np.int64)
    got = M.s_log(M.s_exp(x)[:, None], hist)[:, 0]
    assert hist[2] == 1
    assert np.abs(got[[0, 1, 2, 6]] - x[[0, 1, 2, 6]]).max() < 1e-9 and abs(got[3] - 0.5) < 1e-6
    y = _x(np.array([2e-3, 0.0, 0.0]), np.array([0.0, 0.5, 0.0]), 3e-4)
    assert abs(M.s_log(M.s_exp(y)[:, None])[4, 0]) < 0.01         # far from 0.5: B theta^2 = theta^2 / sigma^3 >> C


def test_lu_solve_against_numpy():
    rng = np.random.default_rng(5)
    W = rng.normal(size=(3, 3, 200))
    W[0, 0, :50] = 0.0                                              # a pivot search that must swap
    W[1, 0, 50:60] = W[0, 0, 50:60]                                 # a tie: the first row stays
    t = rng.normal(size=(3, 200))
    x = np.stack(M.lu3_solve([[W[i][j] for j in range(3)] for i in range(3)], [t[i] for i in range(3)]))
    for n in range(200):
        want = np.linalg.solve(W[:, :, n], t[:, n])
        assert np.abs(x[:, n] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())


def test_a_graph_measured_from_its_own_estimates_stays():
    sc = M.make_scene(21, 7, n_corr=0, band=3, loops=((6, 0),))
    r = M.essential_graph(sc)
    # the float poses' rotations are orthonormal to 1e-7 and their quaternions are not normalised,
    # so Sji * S_i * S_j^-1 is the identity to 1e-7: chi2 is 0 up to the square of that
    assert r["chi2"][0] < 1e-12 and r["chi2"][1] <= r["chi2"][0] and r["status"] == 0
    assert np.abs(r["Scw"] - M.Graph(sc).S0.T).max() < 1e-5


def test_pair_converges_to_the_closed_form():
    sc = M.scene("pair")
    G = M.Graph(sc)
    r = M.essential_graph(sc)
    want = M.s_mul(M.s_inv(G.meas[:, 0]), G.S0[:, 0])               # log(C S_1 S_0^-1) = 0
    got = r["Scw"][1]
    sign = np.sign(got[3] * want[3])
    assert np.abs(got[:4] * sign - want[:4]).max() < 1e-7 and np.abs(got[4:] - want[4:]).max() < 1e-7
    assert r["chi2"][1] < 1e-12 < r["chi2"][0]
    assert r["Scw"][0].tobytes() == G.S0[:, 0].copy().tobytes()     # the fixed keyframe


def test_a_fixed_scale_leaves_every_scale_exactly_one():
    for name in ("ring-9-fixed-scale", "bad-edges"):
        r = M.essential_graph(M.scene(name))
        assert r["trace"][0] >= 4 and (r["Scw"][:, 7] == 1.0).all()
    assert (M.essential_graph(M.scene("ring-9"))["Scw"][1:, 7] != 1.0).all()


def test_the_scenes_take_all_four_branches_of_log():
    hist = sum(M.essential_graph(M.scene(n), iterations=M.exact_iterations(n))["hist"]
               for n in ("ring-9", "ring-9-fixed-scale", "tiny", "large"))
    assert (hist > 0).all(), dict(zip(M.BRANCHES, hist.tolist()))
    assert M.essential_graph(M.scene("tiny"), iterations=4)["hist"][2] > 0
    assert M.essential_graph(M.scene("large"), iterations=4)["hist"][3] > 0


def test_status_cases_of_the_model():
    sc = M.scene("ring-9")
    need = M.envelope(9, 0, sc["edge_v"])[2]
    over = M.essential_graph(sc, max_env_blocks=need - 1)
    assert over["status"] == M.STATUS_CAPACITY and not over["trace"].any()
    assert over["Tcw"].tobytes() == sc["Tcw"].tobytes() and over["pos"].tobytes() == sc["pos"].tobytes()
    none = M.essential_graph(dict(sc, loop=9))
    assert none["status"] == M.STATUS_NO_FIXED_KF and none["Tcw"].tobytes() == sc["Tcw"].tobytes()
    bad = M.scene("bad-edges")
    r = M.essential_graph(bad, iterations=2)
    assert r["status"] == M.STATUS_BAD_INDEX and len(M.Graph(bad).index) == len(bad["edge_v"]) - 5
    out = (bad["pt_ref"] < 0) | (bad["pt_ref"] >= 9)
    assert r["pos"][out].tobytes() == bad["pos"][out].tobytes()
    iso = M.scene("isolated")
    r = M.essential_graph(iso, iterations=2)
    assert r["Scw"][-1].tobytes() == M.Graph(iso).S0[:, -1].copy().tobytes()


@pytest.mark.parametrize("name", ["pair", "ring-9", "fixed-mid"])
def test_envelope_solve_equals_dense_solve_bytewise(name):
    import optimize_sim3_model as O
    sc = M.scene(name)
    G = M.Graph(sc)
    idx, first, blocks = M._envelope(G.K, G.loop, G.ev)
    F = len(first)
    incs = [np.concatenate([q, t, [s]]) for q, t, s in O.probe_increments(False)]
    _, H, b = M.linearize(G, G.S0, idx, F, incs, "forward")
    A = H + 1e-3 * np.eye(7 * F)
    env = M.ldlt_solve_env(A, b, first)
    dense = M.ldlt_solve_env(A, b, np.zeros(F, int))
    loops = M.ldlt_solve_dense(A, b)
    assert env.tobytes() == dense.tobytes() == loops.tobytes()
    full = np.triu(A) + np.triu(A, 1).T
    assert np.abs(full @ env - b).max() < 1e-9
    if name != "pair":
        assert blocks < F * (F + 1) // 2
    A[0, 0] = 0.0
    assert M.ldlt_solve_env(A, b, first) is None and M.ldlt_solve_dense(A, b) is None


def test_envelope_helper(orbx_built):
    from orbslam2commentedbyxcm_amd.optimizer import essential_graph_envelope
    # 6 keyframes, 2 fixed; vertices 0 1 3 4 5 -> indices 0 1 2 3 4; 5 -- 0 makes a long column
    ev = np.array([[1, 0], [3, 1], [4, 3], [5, 4], [5, 0], [3, 2], [2, 4]], np.int32)
    assert essential_graph_envelope(6, 2, ev) == 1 + 2 + 2 + 2 + 5
    # an isolated keyframe (4), a repeated pair, both orientations, bad rows and i == j are no edges
    ev = np.array([[1, 0], [0, 1], [1, 0], [2, 1], [7, 1], [-1, 2], [3, 3], [5, 3]], np.int32)
    assert essential_graph_envelope(6, 0, ev) == 1 + 2 + 1 + 2     # vertices 1 2 3 5
    assert essential_graph_envelope(6, 9, ev) == 1 + 2 + 2 + 1 + 2  # nothing fixed inside the rows
    assert essential_graph_envelope(0, 0, np.zeros((0, 2), np.int32)) == 0
    for name in M.SPECS:
        sc = M.scene(name)
        assert essential_graph_envelope(len(sc["Tcw"]), sc["loop"], sc["edge_v"]) == \
            M.envelope(len(sc["Tcw"]), sc["loop"], sc["edge_v"])[2], name


def test_essential_graph_edges_follows_the_references_order_and_filters():
    from orbslam2commentedbyxcm_amd.optimizer import essential_graph_edges
    ids = [0, 2, 3, 5, 8, 9]                      # mnIds (1, 4, 6, 7 are bad keyframes)
    parent = [-1, 0, 2, 3, 5, 8]
    children = [[2], [3], [5], [8], [9], []]
    loop_edges = [[9], [], [], [], [], [0]]       # AddLoopEdge on both sides
    cov = [
        [(2, 300), (3, 150)],
        [(0, 300), (3, 250), (5, 120)],
        [(2, 250), (0, 150), (5, 140), (9, 101)],
        [(3, 140), (2, 120), (0, 99), (4, 500)],   # 0: below minFeat; 4: a bad keyframe
        [(5, 200), (3, 130), (2, 100)],            # 5 the parent; 3: inserted by LoopConnections
        [(8, 400), (0, 350), (2, 180), (3, 101), (5, 100)],  # 8 the parent, 0 a loop edge
    ]
    # the current keyframe 9 and the loop keyframe 0: kept whatever its weight (cc:966);
    # 9 -- 2 has too few features; 8 -- 3 passes and blocks the covisibility edge 8 -- 3
    conns = [(9, [(0, 10), (2, 99), (3, 100)]), (8, [(3, 100), (0, 10)])]
    ev, kind = essential_graph_edges(ids, parent, children, loop_edges, cov, conns, cur_id=9, loop_id=0)
    r = {m: k for k, m in enumerate(ids)}
    want = [(9, 0, 0), (9, 3, 0), (8, 3, 0),
            (2, 0, 1),
            (3, 2, 1), (3, 0, 1),
            (5, 3, 1), (5, 2, 1),
            (8, 5, 1), (8, 2, 1),
            (9, 8, 1), (9, 0, 1), (9, 2, 1), (9, 5, 1)]
    assert [(ids[i], ids[j], k) for (i, j), k in zip(ev.tolist(), kind.tolist())] == want
    assert ev.dtype == np.int32 and kind.dtype == np.int32 and r[9] == 5
    # the order of LoopConnections is taken as given
    ev2, _ = essential_graph_edges(ids, parent, children, loop_edges, cov, conns[::-1], cur_id=9, loop_id=0)
    assert [(ids[i], ids[j]) for i, j in ev2[:3].tolist()] == [(8, 3), (9, 0), (9, 3)]


def test_argument_checks_need_no_gpu(orbx_built):
    """orbx_optimize_essential_graph_batch_device / orbx_optimize_essential_graph reject bad
    arguments before any GPU call."""
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)

    def batch(**kw):
        q = L.EssentialGraphBatch(batch=2, kf_off=fake, n_kf=4, kf_Tcw=fake, kf_corr=fake, corr_S=fake, n_corr=2,
                                  loop_kf=fake, edge_off=fake, n_edges=5, edge_v=fake, edge_kind=fake, pt_off=fake,
                                  n_pt=8, pt_pos=fake, pt_ref=fake, fix_scale=0, iterations=0, max_env_blocks=16,
                                  dense=0, kf_Tcw_opt=fake, pt_pos_opt=fake, Scw_opt=None, trace=None, chi2=None,
                                  status=fake)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    h = C.c_void_p(0x2000)      # never dereferenced: the checks come first
    dev, host = lib.orbx_optimize_essential_graph_batch_device, lib.orbx_optimize_essential_graph
    assert dev(None, C.byref(batch()), None) == L.ORBX_ERR_ARG
    assert dev(h, None, None) == L.ORBX_ERR_ARG
    off = (C.c_int32 * 2)(0, 3)
    good = dict(kf_off=C.cast((C.c_int32 * 2)(0, 4), C.c_void_p), edge_off=C.cast((C.c_int32 * 2)(0, 5), C.c_void_p),
                pt_off=C.cast((C.c_int32 * 2)(0, 8), C.c_void_p), loop_kf=C.cast((C.c_int32 * 1)(0), C.c_void_p))
    for kw in (dict(batch=-1), dict(n_kf=-1), dict(n_corr=-1), dict(n_edges=-1), dict(n_pt=-1), dict(iterations=-1),
               dict(max_env_blocks=-1), dict(max_env_blocks=1 << 31), dict(kf_off=None), dict(edge_off=None),
               dict(pt_off=None), dict(loop_kf=None), dict(status=None), dict(kf_Tcw=None), dict(kf_corr=None),
               dict(kf_Tcw_opt=None), dict(corr_S=None), dict(edge_v=None), dict(edge_kind=None), dict(pt_pos=None),
               dict(pt_ref=None), dict(pt_pos_opt=None)):
        assert dev(h, C.byref(batch(**kw)), None) == L.ORBX_ERR_ARG, kw
        if "batch" not in kw:
            assert host(h, C.byref(batch(**{**good, "batch": 1, **kw}))) == L.ORBX_ERR_ARG, kw
    assert host(h, C.byref(batch())) == L.ORBX_ERR_ARG          # batch 2
    assert b"one problem" in lib.orbx_last_error()
    for name in ("kf_off", "edge_off", "pt_off"):               # offsets that do not span the table
        q = batch(**{**good, "batch": 1, name: C.cast(off, C.c_void_p)})
        assert host(h, C.byref(q)) == L.ORBX_ERR_ARG, name
        assert b"offsets" in lib.orbx_last_error()
    rev = (C.c_int32 * 2)(4, 0)                                  # descending
    assert host(h, C.byref(batch(**{**good, "batch": 1, "kf_off": C.cast(rev, C.c_void_p)}))) == L.ORBX_ERR_ARG
    n = C.c_int64(0)
    env = lib.orbx_essential_graph_envelope
    assert env(-1, 0, None, 0, C.byref(n)) == L.ORBX_ERR_ARG and env(3, 0, None, 2, C.byref(n)) == L.ORBX_ERR_ARG
    assert env(3, 0, None, 0, None) == L.ORBX_ERR_ARG
