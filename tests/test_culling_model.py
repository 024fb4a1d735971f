"""The culling model (tests/culling_model.py) on its hand-built scenes: each case that the GPU
tests rely on is shown here by the model alone, by name, so that a scene that stops covering a
case fails here and not silently on the GPU."""
from __future__ import annotations

import numpy as np
import pytest

import culling_model as C


def run(name, **kw):
    m = C.copy_maps(C.SCENES[name]() if isinstance(name, str) else name)
    g = C.build_graph(m)
    r = C.key_frame_culling(g, m, m["cur"], kw.get("monocular", m["monocular"]), m["not_erase"])
    C.assert_refreshed(g, m)
    return m, g, r


def counts_of(r, k):
    return r["cand_counts"][r["cand"].tolist().index(k)].tolist()


def contribution(name, k, p):
    """What MapPoint p adds to candidate k's (nMPs, nRedundant) on the entry state."""
    m = C.copy_maps(C.SCENES[name]())
    g = C.build_graph(m)
    with_p = C.evaluate(g, m, k, m["monocular"])
    m["kf_mp"][k][m["kf_mp"][k] == p] = -1
    g = C.build_graph(m)
    without = C.evaluate(g, m, k, m["monocular"])
    return with_p[0] - without[0], with_p[1] - without[1]


def test_ratio_boundaries_and_special_candidates():
    m, g, r = run("bounds")
    assert 0 in r["cand"].tolist() and counts_of(r, 0) == [0, 0, 0] and not m["kf_bad"][0]  # id 0 in the list
    assert counts_of(r, 1) == [10, 9, 0]     # 9 > 9.0 is false
    assert counts_of(r, 2) == [10, 10, 1]
    assert counts_of(r, 3) == [20, 18, 0]    # 18 > 0.9 * 20 is false
    assert counts_of(r, 4) == [20, 19, 1]
    assert counts_of(r, 6) == [0, 0, 0] and not m["kf_bad"][6]  # nMPs = 0
    assert r["culled"].tolist() == [5, 4, 2]


def test_not_erase_candidate_is_only_marked():
    m, g, r = run("bounds")
    assert counts_of(r, 7)[2] == 2 and m["to_be_erased"][7] == 1 and not m["kf_bad"][7] and 7 not in r["culled"]
    # the state is what it would be had 7 not been a candidate at all
    m2 = C.copy_maps(C.SCENES["bounds"]())
    g2 = C.build_graph(m2)
    cand = [k for k in g2.ordered[m2["cur"]] if k != 7]
    for k in cand:
        if k > 0 and not g2._kf_is_bad(k):
            a, b = C.evaluate(g2, m2, k, False)
            if b > 0.9 * a:
                C.set_bad_flag(g2, m2, k, None)
    assert np.array_equal(m["kf_mp"], m2["kf_mp"]) and np.array_equal(m["kf_bad"], m2["kf_bad"])
    assert g.arrays()["row"] == g2.arrays()["row"] and g.parent == g2.parent
    # SetErase: the caller clears mbNotErase and SetBadFlag runs
    assert C.set_bad_flag(g, m, 7, None)[0] == 1 and m["kf_bad"][7]
    C.assert_refreshed(g, m)


def test_nobs_scale_and_depth_boundaries():
    n = C.SCENES["bounds"]()["names"]
    assert contribution("bounds", 1, n["nobs3"]) == (1, 0)                  # nObs 3: not tested further
    assert contribution("bounds", 5, n["nobs4"]) == (1, 1)                  # nObs 4
    assert contribution("bounds", 4, n["stereo_two_observers"]) == (1, 0)   # nObs 4 from two stereo observers, one other
    assert contribution("bounds", 3, n["two_of_four_pass"]) == (1, 0)       # four monocular others, two pass the scale test
    assert contribution("bounds", 5, n["scale_plus1"]) == (1, 1)            # scaleLeveli == scaleLevel + 1
    assert contribution("bounds", 3, n["scale_plus2"]) == (1, 0)            # + 2
    assert contribution("bounds", 5, n["depth_far"]) == (0, 0)              # mvDepth > mThDepth
    assert contribution("bounds", 5, n["depth_negative"]) == (0, 0)         # mvDepth < 0
    assert contribution("bounds", 5, n["depth_at_threshold"]) == (1, 1)     # == mThDepth: counted
    # monocular: no depth filter, the glue and the filtered points count
    _, _, r = run("bounds", monocular=True)
    assert counts_of(r, 5)[0] == 6 + 2 + 16


def test_cascade_matters_and_does_not():
    m0 = C.SCENES["cascade"]()
    g0 = C.build_graph(m0)
    entry = {k: C.evaluate(g0, m0, k, False) for k in (1, 2, 3, 4)}
    m, g, r = run("cascade")
    assert r["culled"].tolist() == [2, 3, 4]
    # 1: culled on the entry state, kept at its turn
    assert entry[1][1] > 0.9 * entry[1][0] and counts_of(r, 1) == [12, 0, 0]
    # 4: the same verdict either way
    assert list(entry[4]) == counts_of(r, 4)[:2] and counts_of(r, 4)[2] == 1
    # a MapPoint that went bad by nObs <= 2 changes a later candidate's nMPs
    (p,) = m0["names"]["fragile"]
    assert m["mp_bad"][p] and not m0["mp_bad"][p] and entry[3][0] == 11 and counts_of(r, 3)[0] == 10
    assert (m["kf_mp"][5] != p).all() and (m["kf_mp"][2] == p).any()  # nulled in the observers, kept in the culled row
    assert r["n_new_bad_mp"] >= 1


def test_nothing_culled_leaves_every_byte():
    m0 = C.SCENES["late"]()
    m, g, r = run("late")
    assert len(r["culled"]) == 0 and r["n_new_bad_mp"] == 0
    for k in ("kf_mp", "kf_bad", "mp_bad", "to_be_erased"):
        assert np.array_equal(m[k], m0[k])


def test_reparenting_rounds_ties_and_leftover():
    t = C.TREE
    m, g, r = run("tree")
    assert r["culled"].tolist() == [t["B"]]
    p = g.parent
    assert p[t["C1"]] == t["A"]        # adopted through a connection to the parent
    assert p[t["C2"]] == t["C1"]       # the second round is won through the promoted child
    assert p[t["C5"]] == t["A"] and p[t["C6"]] == t["C5"]   # a weight tie: the lower child id goes first
    assert p[t["C7"]] == t["C6"]       # equal weights in one list: the earlier position (the higher id)
    assert p[t["C3"]] == t["A"]
    assert p[t["C4"]] == t["A"]        # the leftover child is handed to the grandparent
    assert p[t["B"]] == t["A"] and r["status"] == 0
    # SetBadFlag on its own gives the same tree
    m2 = C.copy_maps(C.SCENES["tree"]())
    g2 = C.build_graph(m2)
    assert C.set_bad_flag(g2, m2, t["B"])[0] == 1 and g2.parent == p
    C.assert_refreshed(g2, m2)


def test_entries_below_15_from_an_earlier_cull_change_the_new_parent():
    t = C.LATE
    m = C.copy_maps(C.SCENES["late"]())
    g = C.build_graph(m)
    assert g.parent[t["C"]] == t["B"] and t["B"] not in g.row[t["C"]] and g.ordered[t["C"]] == [t["X"]]
    C.set_bad_flag(g, m, t["B"])
    C.assert_refreshed(g, m)
    assert g.parent[t["C"]] == t["P"] and g.parent[t["Cp"]] == t["P"]
    m = C.copy_maps(C.SCENES["late"]())
    g = C.build_graph(m)
    C.set_bad_flag(g, m, t["X"])
    assert g.ordered[t["C"]] == [t["Cp"]] and g.weights[t["C"]] == [9]
    C.set_bad_flag(g, m, t["B"])
    C.assert_refreshed(g, m)
    assert g.parent[t["C"]] == t["Cp"] and g.parent[t["Cp"]] == t["P"]


def test_culled_keyframe_without_parent():
    m = C.copy_maps(C.SCENES["tree"]())
    g = C.build_graph(m)
    g.parent[C.TREE["B"]] = -1
    res, status, _ = C.set_bad_flag(g, m, C.TREE["B"])
    assert res == 1 and status == C.NO_PARENT and g.parent[C.TREE["C1"]] == -1


@pytest.mark.parametrize("name", ["band", "big"])
def test_random_scenes_cull_and_stay_refreshed(name):
    m0 = C.SCENES[name]() if name in C.SCENES else C.big_scene()
    m, g, r = run(m0)
    assert len(r["culled"]) >= 2
    if name == "big":
        assert (np.argwhere(m0["kf_mp"] >= 0)[:, 1] >= 1024).any()


@pytest.mark.parametrize("monocular", [False, True])
def test_map_point_culling_branches(monocular):
    m = C.copy_maps(C.SCENES["band"]())
    g = C.build_graph(m)
    recent, found, visible, first = C.recent_case(m, g, 3, 150)
    br = {}
    kept, n = C.map_point_culling(g, m, recent, 10, monocular, found, visible, first, br)
    C.assert_refreshed(g, m)
    assert set(br) == {"bad", "ratio", "few_observations", "old", "kept"}, br
    assert n == br["ratio"] + br["few_observations"] and len(kept) == br["kept"]
    # visible = 0 (0 / 0 and 3 / 0) and found / visible exactly 0.25 are not below the ratio
    m2 = C.copy_maps(C.SCENES["band"]())
    g2 = C.build_graph(m2)
    for j in range(3):
        br2 = {}
        C.map_point_culling(g2, m2, recent[j:j + 1], 10, monocular, found, visible, first, br2)
        assert "ratio" not in br2 and "bad" not in br2, (j, br2)
    # both cnThObs: a point with exactly 3 observations is culled by the second test unless monocular
    counts = C.observation_counts(g2, m2["u_right"])
    p = int(np.flatnonzero((counts == 3) & (m2["mp_bad"] == 0))[0])
    found[p], visible[p], first[p] = 4, 4, 8
    br3 = {}
    C.map_point_culling(g2, m2, [p], 10, monocular, found, visible, first, br3)
    assert br3 == ({"kept": 1} if monocular else {"few_observations": 1})


def test_observation_counts_mono_and_stereo():
    m = C.copy_maps(C.SCENES["band"]())
    g = C.build_graph(m)
    mono, stereo = C.observation_counts(g, None), C.observation_counts(g, m["u_right"])
    assert (mono[m["mp_bad"] == 1] == 0).all() and (stereo >= mono).all() and (stereo > mono).any()
    p = int(np.flatnonzero(mono > 0)[0])
    assert mono[p] == len(g.obs[p])
