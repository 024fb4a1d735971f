"""The CorrectLoop model (tests/correct_loop_model.py): the parallel forms that the device runs
equal the sequential restatement of the reference on every scene, and the scenes reach every
boundary that the GPU tests rely on.  CPU only (the host-only essential_graph_edges and
orbx_essential_graph_envelope come from the built library)."""
from __future__ import annotations

import numpy as np
import pytest

import correct_loop_model as M
import covisibility_model as CM

STATE = ("poses", "mp_pos", "mp_corrected_by_kf", "mp_corrected_ref", "normal", "max_distance", "min_distance", "conn",
         "corr_S", "kf_corr", "kf_Tcw_nc")
TABLES = ("lc_member", "lc_off", "lc_kf", "lc_w", "kf_ids", "kf_row", "kf_corr_rows", "kf_Tcw_rows", "edge_v", "edge_kind",
          "pt_ref")


@pytest.fixture(scope="module")
def runs(orbx_built):
    """Each scene once in the sequential and once in the parallel form."""
    return {name: (M.run(name), M.run(name, parallel=True, snapshot=True)) for name in M.SCENES}


def same_graph(a: CM.Graph, b: CM.Graph):
    x, y = a.arrays(), b.arrays()
    assert x["row"] == y["row"] and x["ordered"] == y["ordered"]
    for k in ("parent", "first", "status"):
        assert np.array_equal(x[k], y[k]), k


@pytest.mark.parametrize("name", M.SCENES)
def test_ownership_and_interleaved_poses_equal_the_sequential_walk(runs, name):
    (_, seq, _, _, g_seq), (_, par, _, _, g_par) = runs[name]
    for k in STATE:
        assert np.array_equal(seq[k], par[k]), k  # float64 / float32 bytes, no tolerance
    assert seq["status"] == par["status"]
    same_graph(g_seq, g_par)


@pytest.mark.parametrize("name", M.SCENES)
def test_snapshot_loop_connections_equal_the_sequential_form(runs, name):
    (_, _, seq, g_seq, _), (_, _, par, g_par, _) = runs[name]
    assert seq["lc"] == par["lc"]
    for k in TABLES:
        assert np.array_equal(seq[k], par[k]), k
    assert seq["loop_row"] == par["loop_row"] and seq["env_blocks"] == par["env_blocks"]
    same_graph(g_seq, g_par)


def test_ordered_list_alone_is_not_the_previous_neighbours(runs):
    """Why the snapshot holds the rows too: AddConnection re-orders a keyframe's whole row
    (KeyFrame.cc:139-153, 160-182), entries below 15 included, so a member updated after another
    sees more previous neighbours than its ordered list at entry had."""
    differs = False
    for name in M.SCENES:
        sc, st = M.scene(name)
        g = M.graph_of(sc)
        out = M.propagate(g, st, sc["cur"], sc["Scw"])
        g.refresh_observations(sc["kf_mp_fused"], sc["kf_n"], sc["kf_bad"], sc["mp_bad"])
        conn = [int(k) for k in out["conn"]]
        prev = {i: set(g.ordered[i]) for i in conn}
        lc = dict(M.loop_connections(g, conn))
        naive = {i: sorted(set(g.row[i]) - prev[i] - set(conn)) for i in conn}
        differs |= any(naive[i] != [k for k, _ in lc[i]] for i in conn)
    assert differs


def test_hand_scene_reaches_every_boundary(runs):
    sc, out, asm, g, _ = runs["hand"][0]
    cur, loop, mf = sc["cur"], sc["loop"], sc["min_feat"]
    _, obs, _ = CM.observations(sc["kf_mp"], sc["kf_n"], sc["kf_bad"], len(sc["mp_bad"]))
    members = set(out["conn"].tolist())
    assert len(members) >= 3 and cur in members and loop not in members
    # a point held by two members: the lower id owns it
    shared = [p for p in range(len(obs)) if len(members & set(obs[p])) >= 2 and not sc["mp_bad"][p] and p not in sc["already"]]
    assert shared and all(out["mp_corrected_ref"][p] == min(members & set(obs[p])) for p in shared)
    # whose normal mixes corrected and input poses: an observer above the owner is a member too
    assert any(max(members & set(obs[p])) > out["mp_corrected_ref"][p] for p in shared)
    # a point already marked corrected by cur keeps its bytes
    _, st0 = M.scene("hand")
    for p in sc["already"]:
        assert st0["mp_corrected_by_kf"][p] == cur and np.array_equal(out["mp_pos"][p], st0["mp_pos"][p])
        assert out["mp_corrected_ref"][p] == loop and any(k in members for k in obs[p])
    # a bad point and a NULL entry in a member's row
    assert any(sc["mp_bad"][p] and members & set(obs[p]) for p in range(len(obs)))
    assert all(out["mp_corrected_by_kf"][p] != cur for p in np.flatnonzero(sc["mp_bad"]))
    assert all((sc["kf_mp"][k, :sc["kf_n"][k]] < 0).any() for k in members)
    # a reference keyframe that is not an observer, among the corrected points
    assert out["status"] & M.REF_NOT_OBSERVER
    assert any(out["mp_corrected_by_kf"][p] == cur and st0["mp_ref_kf"][p] not in obs[p] for p in range(len(obs)))
    # LoopConnections weights 99 and 100, the cur - loop pair below min_feat
    lc = {i: dict(c) for i, c in asm["lc"]}
    weights = {w for c in lc.values() for w in c.values()}
    assert mf in weights and mf - 1 in weights
    assert 0 < lc[cur][loop] < mf
    kind0 = {(int(asm["kf_ids"][a]), int(asm["kf_ids"][b])) for (a, b), k in zip(asm["edge_v"], asm["edge_kind"]) if k == 0}
    assert (cur, loop) in kind0
    assert all((i, k) in kind0 if (w >= mf or (i, k) == (cur, loop)) else (i, k) not in kind0 for i, c in lc.items() for k, w in c.items())
    # covisibility edges at weights 99 and 100
    kind1 = {(int(asm["kf_ids"][a]), int(asm["kf_ids"][b])) for (a, b), k in zip(asm["edge_v"], asm["edge_kind"]) if k == 1}
    inp = asm["inputs"]
    row = {k: r for r, k in enumerate(inp["ids"])}
    cov = {(k, n): w for k in inp["ids"] for n, w in inp["covis"][row[k]]}
    assert cov[(2, 1)] == mf and (2, 1) in kind1
    assert cov[(3, 0)] == mf - 1 and inp["parent"][row[3]] != 0 and (3, 0) not in kind1
    # a pair already inserted as kind 0 is skipped by the covisibility walk
    skipped = [(k, n) for (k, n), w in cov.items() if w >= mf and n < k and ((k, n) in kind0 or (n, k) in kind0)]
    assert skipped and all(e not in kind1 for e in skipped)
    # a covisible at or above min_feat that is the parent, a child, a loop edge
    strong = [(k, n) for (k, n), w in cov.items() if w >= mf]
    assert any(inp["parent"][row[k]] == n for k, n in strong)
    assert any(n in inp["children"][row[k]] and n < k for k, n in strong)
    assert any(n in inp["loops"][row[k]] and n < k for k, n in strong)
    n_edges = len(asm["edge_v"])
    assert n_edges == len({(a, b, k) for (a, b), k in zip(asm["edge_v"].tolist(), asm["edge_kind"].tolist())})  # each once
    # a bad keyframe in the middle of the ids: rows are compacted
    bad = int(np.flatnonzero(sc["kf_bad"])[0])
    assert 0 < bad < len(sc["kf_bad"]) - 1 and asm["kf_row"][bad] == -1 and asm["kf_row"][bad + 1] == bad
    # a keyframe with no edge at all
    lonely = row[9]
    assert not (asm["edge_v"] == lonely).any()


@pytest.mark.parametrize("name", ["geo10", "band24"])
def test_random_scenes_are_not_trivial(runs, name):
    sc, out, asm, _, _ = runs[name][0]
    assert len(out["conn"]) >= 4 and (out["mp_corrected_by_kf"] == sc["cur"]).sum() > 50
    assert (asm["edge_kind"] == 0).any() and (asm["edge_kind"] == 1).any() and any(c for _, c in asm["lc"])
    assert np.all(asm["pt_ref"][sc["mp_bad"] != 0] == -1) and (asm["pt_ref"] >= 0).sum() > 100


def test_update_normal_and_depth_over_ids_and_all(runs):
    sc, out, _, g, _ = runs["hand"][0]
    st = dict(out)
    n_all = M.update_normal_and_depth(g, st)
    ids = [5, 700, 3, len(sc["mp_bad"]) + 4, -1]
    n_ids = M.update_normal_and_depth(g, st, ids)
    assert n_ids[3] & M.BAD_INDEX and n_all[3] & M.REF_NOT_OBSERVER
    for p in (5, 700, 3):
        assert np.array_equal(n_ids[0][p], n_all[0][p]) and n_ids[1][p] == n_all[1][p]
    untouched = [p for p in range(len(sc["mp_bad"])) if sc["mp_bad"][p] or not g.obs[p]]
    assert untouched and all(np.array_equal(n_all[0][p], st["normal"][p]) for p in untouched)
    # unit-length-or-shorter mean ray, and the distance pair
    seen = [p for p in range(len(sc["mp_bad"])) if g.obs[p] and not sc["mp_bad"][p]]
    assert np.all(np.linalg.norm(n_all[0][seen], axis=1) <= 1.0 + 1e-6)
    assert np.allclose(n_all[2][seen] * st["scale"][-1], n_all[1][seen], rtol=1e-6)
