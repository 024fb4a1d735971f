"""KeyFrameDatabase, the parts that need no GPU: the host L1 score (orbx_bow_score) against
the pure-Python model (tests/kfdb_model.py), argument errors of the orbx_kfdb_* entry
points, the model's own known answers, and guards that the scenes the GPU tests use
(tests/test_gpu_kfdb.py) are not vacuous.  Every comparison is exact."""
from __future__ import annotations

import ctypes as C

import numpy as np

import kfdb_model as M

RELOC_SEED = 1  # shared with tests/test_gpu_kfdb.py
LOOP_SEED = 1


def _bits(x: float) -> int:
    return int(np.float64(x).view(np.uint64))


def _score(v1, v2) -> float:
    from orbslam2commentedbyxcm_amd.database import bow_score
    return bow_score(v1, v2)


def test_bow_score_matches_model_bit_for_bit(orbx_built):
    rng = np.random.default_rng(7)
    for _ in range(300):
        a = M.random_bow(rng, int(rng.integers(0, 120)), 200)
        b = M.random_bow(rng, int(rng.integers(0, 120)), 200)
        assert _bits(_score(a, b)) == _bits(M.l1_score(a, b))
        assert _bits(_score(b, a)) == _bits(M.l1_score(b, a))


def test_bow_score_edge_cases(orbx_built):
    """Worked by hand: v1 = {1: 0.5, 3: 0.5}, v2 = {3: 0.25, 4: 0.75} share word 3 only:
    |0.5 - 0.25| - 0.5 - 0.25 = -0.5, score = 0.5 / 2 = 0.25.  Identical L1-normalised
    vectors of dyadic values score exactly 1; disjoint (or empty) vectors -0.0."""
    assert _score({1: 0.5, 3: 0.5}, {3: 0.25, 4: 0.75}) == 0.25
    v = {2: 0.25, 5: 0.5, 9: 0.25}
    assert _score(v, v) == 1.0
    rng = np.random.default_rng(8)
    a = M.random_bow(rng, 50, 100)
    assert _bits(_score(a, a)) == _bits(M.l1_score(a, a))
    minus_zero = _bits(-0.0)
    assert minus_zero != _bits(0.0)
    assert _bits(_score({1: 0.5, 2: 0.5}, {3: 1.0})) == minus_zero == _bits(M.l1_score({1: 0.5, 2: 0.5}, {3: 1.0}))
    assert _bits(_score({}, a)) == minus_zero and _bits(_score(a, {})) == minus_zero
    assert _bits(_score({}, {})) == minus_zero
    # one shared word at either end
    lo = {0: 0.3, 50: 0.7}, {0: 0.6, 10: 0.1, 20: 0.3}
    hi = {5: 0.3, 99: 0.7}, {1: 0.2, 99: 0.8}
    for x, y in (lo, hi):
        assert _bits(_score(x, y)) == _bits(M.l1_score(x, y))
        assert _bits(_score(y, x)) == _bits(M.l1_score(y, x))


def test_kfdb_arguments_rejected_without_gpu(orbx_built):
    """orbx_bow_score and the orbx_kfdb_* entry points check their arguments before any
    device call."""
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    w = np.array([1, 2], np.int32)
    v = np.array([0.5, 0.5], np.float64)
    out = C.c_double()
    wp, vp = w.ctypes.data_as(C.POINTER(C.c_int32)), v.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.orbx_bow_score(wp, vp, 2, wp, vp, 2, None) == L.ORBX_ERR_ARG
    assert lib.orbx_bow_score(None, vp, 2, wp, vp, 2, C.byref(out)) == L.ORBX_ERR_ARG
    assert lib.orbx_bow_score(wp, vp, -1, wp, vp, 2, C.byref(out)) == L.ORBX_ERR_ARG
    assert lib.orbx_bow_score(None, None, 0, wp, vp, 2, C.byref(out)) == L.ORBX_OK
    h = C.c_void_p()
    assert lib.orbx_kfdb_create(None, 16, 16, None) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_create(None, 16, 16, C.byref(h)) == L.ORBX_ERR_ARG and not h.value
    assert lib.orbx_kfdb_create(None, 0, 16, C.byref(h)) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_create(None, 16, 0, C.byref(h)) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_create(None, 8193, 16, C.byref(h)) == L.ORBX_ERR_UNSUPPORTED
    assert lib.orbx_kfdb_create(None, 16, 8193, C.byref(h)) == L.ORBX_ERR_UNSUPPORTED
    lib.orbx_kfdb_destroy(None)
    fake = C.c_void_p(0x1000)  # never dereferenced
    n = C.c_int()
    ids = (C.c_int32 * 2)(0, 1)
    assert lib.orbx_kfdb_info(None, None, None, C.byref(n)) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_stream(None) is None
    assert lib.orbx_kfdb_add_batch_device(None, 2, ids, fake, fake, fake, 4, None) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_add(None, 0, wp, vp, 2) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_erase(None, 0) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_clear(None) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_set_covisibility(None, 0, ids, 2) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_reloc_scores(None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_score_device(None, fake, fake, fake, 4, fake, 1, fake, None) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_detect_relocalization_candidates_device(None, 1, fake, fake, fake, 4, fake, 4, fake, None,
                                                                 None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_detect_loop_candidates_device(None, 1, fake, fake, fake, 4, fake, fake, fake, fake, 4, fake,
                                                       None, None, None) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_detect_relocalization_candidates(None, wp, vp, 2, ids, 2, C.byref(n)) == L.ORBX_ERR_ARG
    assert lib.orbx_kfdb_detect_loop_candidates(None, wp, vp, 2, ids, 2, 0.5, ids, 2, C.byref(n)) == L.ORBX_ERR_ARG


def _four():
    db = M.Database()
    db.add(0, {1: 0.5, 2: 0.5})
    db.add(1, {2: 0.5, 3: 0.5})
    db.add(2, {1: 1.0})
    db.add(3, {9: 1.0})
    db.set_covisibility(0, [2, 1])
    db.set_covisibility(1, [0])
    return db


def test_model_relocalization_known_answer():
    """Four keyframes, query q = {1: .5, 2: .25, 3: .25}.  Walking q's words: word 1 lists
    [0, 2], word 2 [0, 1], word 3 [1]: sharing list [0, 2, 1] with 2, 1, 2 words;
    minCommonWords = (int)(2 * 0.8f) = 1, so keyframe 2 (exactly 1 word) is not scored.
    s(q, 0) = 0.75, s(q, 1) = 0.5.  Group of 0: 0.75 + mRelocScore(2) = 0 (pinned) + 0.5 =
    1.25, best 0; group of 1: 0.5 + 0.75 = 1.25, best 0.  Both pass 0.75 * 1.25; the repeat
    is dropped: [0].  Then {1: 1.0} scores keyframe 2 with 1.0 (result [2]), and q again
    finds that stale 1.0 in the group of 0: 0.75 + 1.0 + 0.5 = 2.25, best 2 -> [2]."""
    db = _four()
    q = {1: 0.5, 2: 0.25, 3: 0.25}
    assert db.detect_relocalization_candidates(q) == [0]
    assert db.diag["words"] == {0: 2, 2: 1, 1: 2} and list(db.diag["words"]) == [0, 2, 1]
    assert db.diag["scores"] == {0: np.float32(0.75), 1: np.float32(0.5)}
    assert db.diag["removed_repeat"] and db.diag["at_threshold"]
    assert db.detect_relocalization_candidates({1: 1.0}) == [2]
    assert db.detect_relocalization_candidates(q) == [2]
    assert db.reloc_scores(4).tolist() == [0.75, 0.5, 1.0, 0.0]
    assert db.detect_relocalization_candidates({7: 1.0}) == []
    assert db.detect_relocalization_candidates({}) == []


def test_model_loop_known_answer():
    """The same four keyframes and query.  Connected {1}: sharing [0, 2], keyframe 0 scores
    0.75 >= minScore 0.75 and forms the only group (its neighbour 2 has 1 word, not over
    the threshold; neighbour 1 is connected): [0].  One float above 0.75 drops it.  With
    no connected set and minScore 0.5 both 0 and 1 are listed, both groups name 0."""
    q = {1: 0.5, 2: 0.25, 3: 0.25}
    db = _four()
    assert db.detect_loop_candidates(q, [1], 0.75) == [0]
    assert db.diag["dropped_by_connected"] and not db.diag["dropped_by_min_score"]
    assert db.detect_loop_candidates(q, [1], np.nextafter(np.float32(0.75), np.float32(1))) == []
    assert db.diag["dropped_by_min_score"]
    assert db.detect_loop_candidates(q, [], 0.5) == [0]
    assert db.diag["removed_repeat"]
    assert db.detect_loop_candidates(q, [], 0.6) == [0]     # 1 is scored but not listed; it still counts as neighbour
    assert db.detect_loop_candidates(q, [0, 1, 2], 0.0) == []
    # erase keeps the others' order, a keyframe added again goes to the end
    db.erase(0)
    db.add(0, {1: 0.5, 2: 0.5})
    db.detect_loop_candidates(q, [], 0.0)
    assert list(db.diag["words"]) == [2, 0, 1]


def test_scene_guards_relocalization():
    """The GPU relocalisation scene exercises every stage: several candidates, a repeat
    dropped in the selection, a stale mRelocScore that changes a result, a keyframe exactly
    at words == minCommonWords, an empty query and a query without candidates."""
    ops, queries = M.reloc_scene(RELOC_SEED)
    assert any(op[0] == "erase" for op in ops)
    erased = {op[1] for op in ops if op[0] == "erase"}
    assert any(op[0] == "covis" and erased & set(op[2]) for op in ops)
    assert any(op[0] == "covis" and 0 < len(op[2]) < 10 for op in ops)
    assert any(op[0] == "add" and not op[2] for op in ops)
    db, db0 = M.replay(ops), M.replay(ops)
    ge2 = repeat = threshold = stale = False
    sizes = []
    for q in queries:
        a = db.detect_relocalization_candidates(q)
        sizes.append(len(a))
        ge2 |= len(a) >= 2
        repeat |= db.diag["removed_repeat"]
        threshold |= db.diag["at_threshold"]
        stale |= a != db0.detect_relocalization_candidates(q, stale_as_zero=True)
    assert ge2 and repeat and threshold and stale
    assert queries[2] == {} and sizes[2] == 0 and sizes[5] == 0 and len(queries[5]) > 0


def test_scene_guards_loop():
    """The GPU loop scene drops candidates by minScore and by the connected set, returns
    several candidates somewhere, and uses a minScore equal to a candidate's score, one
    float above it and one below."""
    ops, queries = M.loop_scene(LOOP_SEED)
    db = M.replay(ops)
    by_score = by_conn = ge2 = equal = False
    for bow, conn, ms in queries:
        a = db.detect_loop_candidates(bow, conn, ms)
        by_score |= db.diag["dropped_by_min_score"]
        by_conn |= db.diag["dropped_by_connected"]
        ge2 |= len(a) >= 2
        equal |= any(s == ms for s in db.diag["scores"].values())
    assert by_score and by_conn and ge2 and equal
