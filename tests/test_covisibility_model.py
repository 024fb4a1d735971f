"""The covisibility model (tests/covisibility_model.py) against answers worked by hand, the
premise of the device's parallel batch (a batch's result does not depend on the order of its
ids), the argument checks that need no GPU, and guards that the scenes of the GPU tests reach
every case they are meant to."""
import ctypes as C
import itertools

import numpy as np
import pytest

import covisibility_model as M


def table(rows, cap=None):
    cap = cap or max(len(r) for r in rows)
    t = np.full((len(rows), cap), -1, np.int32)
    for k, r in enumerate(rows):
        t[k, :len(r)] = r
    return t, np.array([len(r) for r in rows], np.int32)


def graph(rows, kf_bad=None, mp_bad=None, n_mp=None, max_conn=8192):
    t, n = table(rows)
    n_mp = n_mp or int(t.max()) + 1
    g = M.Graph(len(rows), max_conn)
    g.refresh_observations(t, n, kf_bad, mp_bad, n_mp)
    return g


def test_two_keyframes_sharing_three_points():
    g = graph([[0, 1, 2], [0, 1, 2, 3]])
    g.update_connections(1)
    assert g.row[1] == {0: 3} and g.ordered[1] == [0] and g.weights[1] == [3]  # pKFmax alone
    assert g.parent[1] == 0 and not g.first[1]
    assert g.row[0] == {1: 3} and g.ordered[0] == [1]  # AddConnection on pKFmax
    g.update_connections(0)
    assert g.row[0] == {1: 3} and g.ordered[0] == [1] and g.weights[0] == [3]
    assert g.parent[0] == -1 and g.first[0]  # nothing for id 0


def test_threshold_14_and_15():
    a, b = list(range(0, 14)), list(range(100, 115))
    g = graph([a, b, a + b])
    g.update_connections(2)
    assert g.row[2] == {0: 14, 1: 15}
    assert g.ordered[2] == [1] and g.weights[2] == [15]
    assert g.row[1] == {2: 15} and g.ordered[1] == [2]
    assert g.row[0] == {} and g.ordered[0] == []  # 14 sends no message


def test_equal_weights():
    a, b, c = list(range(0, 20)), list(range(100, 120)), list(range(200, 220))
    g = graph([a, b, c, a + b + c])
    g.update_connections(3)
    assert g.ordered[3] == [2, 1, 0] and g.weights[3] == [20, 20, 20]  # ids descending
    assert g.parent[3] == 2
    g = graph([a[:5], b[:5], c[:5], a[:5] + b[:5] + c[:5]])
    g.update_connections(3)
    assert g.ordered[3] == [0] and g.weights[3] == [5]  # the lowest id among the maxima
    assert g.row[3] == {0: 5, 1: 5, 2: 5}
    assert g.row[0] == {3: 5} and g.row[1] == {} and g.row[2] == {}


def _three():
    a, b, c = list(range(0, 20)), list(range(100, 105)), list(range(200, 216))
    rows = [a + b + c, a, b, c]
    t, n = table(rows)
    n3 = n.copy()
    n3[3] = 0  # keyframe 3 arrives later
    g = M.Graph(4)
    g.refresh_observations(t, n3, None, None, 300)
    g.update_connections(0)
    assert g.row[0] == {1: 20, 2: 5} and g.ordered[0] == [1]
    return g, t, n


def test_same_weight_leaves_list_and_new_entry_reorders_all():
    g, t, n = _three()
    g.update_connections(1)  # sends (1, 20) to keyframe 0, which holds it: nothing is touched
    assert g.ordered[0] == [1] and g.weights[0] == [20]
    g.update_connections(2)  # pKFmax = 0 with weight 5: held as well
    assert g.ordered[0] == [1]
    g.refresh_observations(t, n, None, None, 300)
    g.update_connections(3)  # a new entry: the whole row is ordered, the entry below 15 included
    assert g.row[0] == {1: 20, 2: 5, 3: 16}
    assert g.ordered[0] == [1, 3, 2] and g.weights[0] == [20, 16, 5]
    assert g.parent[3] == 0 and g.parent[0] == -1


def test_covisibles_by_weight_quirk():
    g, t, n = _three()
    g.refresh_observations(t, n, None, None, 300)
    g.update_connections(3)
    assert g.weights[0] == [20, 16, 5]
    assert g.covisibles_by_weight(0, 16) == [1, 3]
    assert g.covisibles_by_weight(0, 17) == [1]
    assert g.covisibles_by_weight(0, 21) == []   # upper_bound at begin
    assert g.covisibles_by_weight(0, 5) == [1, 3, 2]
    assert g.covisibles_by_weight(0, 1) == [1, 3, 2]  # the end reached, but the last weight is not below w
    assert g.covisibles_by_weight(2, 1) == []   # an empty list
    assert g.best_covisibles(0, 2) == [1, 3] and g.best_covisibles(0, 10) == [1, 3, 2]


def test_erase():
    g, t, n = _three()
    g.refresh_observations(t, n, None, None, 300)
    g.update_connections(3)
    g.erase_keyframe(0)  # id 0 is never erased
    assert g.ordered[0] == [1, 3, 2]
    g.erase_keyframe(3)
    assert g.row[3] == {} and g.ordered[3] == []
    assert g.row[0] == {1: 20, 2: 5} and g.ordered[0] == [1, 2]  # re-ordered: the whole row
    g.erase_keyframe(2)  # keyframe 2 never updated itself: its row is empty, nobody is told
    assert g.row[0] == {1: 20, 2: 5}


def test_duplicates_and_bad_rows_in_the_observations():
    t, n = table([[4, 7, 4, 9], [7, 7, 50, -1], [9, 4, 2, 1]])
    clean, obs, dup = M.observations(t, n, np.array([0, 0, 1], np.uint8), 10)
    assert clean.tolist() == [[4, 7, -1, 9], [7, -1, -1, -1], [9, 4, 2, 1]]
    assert dup.tolist() == [True, True, False]
    assert obs[4] == {0: 0} and obs[7] == {0: 1, 1: 0} and obs[9] == {0: 3} and obs[2] == {}


def _final(g):
    a = g.arrays()
    return (a["row"], a["ordered"], a["parent"].tolist(), a["first"].tolist(), a["status"].tolist())


@pytest.mark.parametrize("seed", range(24))
def test_batch_result_does_not_depend_on_the_order(seed):
    """The premise of the parallel batch: from one start state, UpdateConnections over the
    batch's ids in order, reversed and in random orders ends in one state -- whether the graph
    is fresh or already holds (stale) connections from before a change of the map."""
    kf_mp, kf_n, kf_bad, mp_bad = M.scene(seed)
    K = len(kf_mp)
    rng = np.random.default_rng(1000 + seed)
    all_ids = list(range(K))
    subset = sorted(rng.permutation(K)[:K // 3].tolist())
    kf_mp2 = M.mutate(kf_mp, subset, rng)

    def run(first_order, second_order):
        g = M.Graph(K)
        g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
        for k in first_order:
            g.update_connections(k)
        s1 = _final(g)
        g.refresh_observations(kf_mp2, kf_n, kf_bad, mp_bad)
        for k in second_order:
            g.update_connections(k)
        return s1, _final(g)

    want = run(all_ids, subset)
    assert run(all_ids[::-1], subset[::-1]) == want
    for _ in range(3):
        assert run(rng.permutation(all_ids).tolist(), rng.permutation(subset).tolist()) == want


def test_small_batches_all_permutations():
    kf_mp, kf_n, kf_bad, mp_bad = M.scene(3, K=8, bad_kfs=(2,))
    ids = [1, 3, 4, 6]
    want = None
    for order in itertools.permutations(ids):
        g = M.Graph(8)
        g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
        for k in (0, 5, 7):
            g.update_connections(k)
        for k in order:
            g.update_connections(k)
        want = want or _final(g)
        assert _final(g) == want


@pytest.mark.parametrize("name", sorted(M.GPU_SCENES))
def test_gpu_scenes_are_not_vacuous(name):
    kf_mp, kf_n, kf_bad, mp_bad = M.scene(**M.GPU_SCENES[name])
    K = len(kf_mp)
    g = M.Graph(K)
    g.refresh_observations(kf_mp, kf_n, kf_bad, mp_bad)
    counters, pkfmax, ties = [], 0, 0
    for k in range(K):
        g.update_connections(k)
        if not kf_bad[k]:
            counters.append(len(g.row[k]))
            if g.row[k] and max(g.row[k].values()) < M.TH:
                pkfmax += 1
            ties += len(set(g.weights[k])) < len(g.weights[k])
    assert 0 in counters            # a keyframe whose counter is empty
    assert pkfmax > 0               # one on the pKFmax path
    assert ties > 0                 # equal weights in a list
    assert any(len(g.obs[p]) < sum(1 for k in range(K) if p in set(M.observations(kf_mp, kf_n, None, len(mp_bad))[0][k].tolist()))
               for p in range(len(mp_bad)))  # a point that a bad keyframe observes
    # outside a second batch: a list that changes and one that does not
    rng = np.random.default_rng(5)
    subset = M.GPU_SUBSET
    kf_mp2 = M.mutate(kf_mp, subset, rng)
    lists = [list(o) for o in g.ordered]
    g.refresh_observations(kf_mp2, kf_n, kf_bad, mp_bad)
    for k in subset:
        g.update_connections(k)
    outside = [k for k in range(K) if k not in subset]
    assert any(g.ordered[k] != lists[k] for k in outside)
    assert any(g.ordered[k] == lists[k] and lists[k] for k in outside)
    # the assembly: a fixed camera and a local point that only one local keyframe sees
    poses = np.zeros((K, 12), np.float32)
    pos = np.zeros((len(mp_bad), 3), np.float32)
    fixed = lonely = 0
    for cur in M.GPU_CURRENT:
        t = M.assemble_local_ba(g, cur, poses, pos)
        nl = 1 + sum(1 for k in g.ordered[cur] if not kf_bad[k])
        fixed += len(t["kf_id"]) - nl
        for j in range(len(t["pt_id"])):
            rows = t["obs_kf"][t["obs_off"][j]:t["obs_off"][j + 1]]
            lonely += int((rows < nl).sum() == 1)
    assert fixed > 0 and lonely > 0


def test_arguments_are_checked_without_a_gpu(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.orbx_covis_create(0, 16, 64, 100, 8193, C.byref(h)) == L.ORBX_ERR_ARG and not h.value
    assert b"8192" in lib.orbx_last_error()
    for args in ((0, -1, 64, 100, 16), (0, 16, -64, 100, 16), (0, 16, 64, -100, 16), (0, 16, 64, 100, -1),
                 (-1, 16, 64, 100, 16), (0, 0, 64, 100, 16)):
        assert lib.orbx_covis_create(*args, C.byref(h)) == L.ORBX_ERR_ARG and not h.value
    assert lib.orbx_covis_create(0, 16, 64, 100, 16, None) == L.ORBX_ERR_ARG
    ids = np.array([3, 5, 3], np.int32)
    assert lib.orbx_covis_update_connections_device(None, L.i32ptr(ids), 3, None) == L.ORBX_ERR_ARG
    assert b"repeated" in lib.orbx_last_error()
    assert lib.orbx_covis_update_connections_device(None, L.i32ptr(ids), 2, None) == L.ORBX_ERR_ARG
    assert b"null" in lib.orbx_last_error()
    assert lib.orbx_covis_update_connections_device(None, L.i32ptr(ids), -1, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_refresh_observations_device(None, 1, None, None, None, 1, None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_erase_keyframe_device(None, 1, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_view_device(None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_best_covisibles_device(None, 10, None, None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_covisibles_by_weight_device(None, 10, None, None, None) == L.ORBX_ERR_ARG
    n = C.c_int()
    assert lib.orbx_covis_ordered(None, 0, None, None, 0, C.byref(n)) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_read(None, None, None, 0) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_stream(None) is None
    lib.orbx_covis_destroy(None)
    L.debug_set("covis_lds_keyframes", 8)
    L.debug_set("covis_lds_keyframes", -1)
