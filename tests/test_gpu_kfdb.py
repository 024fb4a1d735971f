"""GPU parity of the device KeyFrameDatabase (orbx_kfdb_*, csrc/orbx_kfdb.hip) with the
pure-Python model of KeyFrameDatabase.cc:31-307 / ScoringObject.cpp:23-68
(tests/kfdb_model.py): candidate ids, their order, the counts, and the float scores by bit
pattern.  BowVectors are synthesised directly (sorted random words out of 1000, values
L1-normalised in word order) except in the end-to-end test, which goes through the
vocabulary transform.  tests/test_kfdb_host.py checks on the CPU that the scenes used here
reach every stage."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import kfdb_model as M
import vocab_scenes as VS
from test_kfdb_host import LOOP_SEED, RELOC_SEED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voc(orbx_built):
    from orbslam2commentedbyxcm_amd.vocabulary import ORBVocabulary

    V = ORBVocabulary(0)
    assert V.loadFromText(VS.make_vocab(71, k=10, L=3).text())
    assert V.size() == 1000
    yield V
    V.close()


def _db(voc, max_keyframes, cap=320):
    from orbslam2commentedbyxcm_amd import KeyFrameDatabase

    return KeyFrameDatabase(voc, max_keyframes, cap)


def _apply(db, ops):
    """Replay model ops on the device database (consecutive adds as one batch)."""
    ids, bows = [], []

    def flush():
        if ids:
            db.add_batch(ids, bows)
            ids.clear()
            bows.clear()

    for op in ops:
        if op[0] == "add":
            ids.append(op[1])
            bows.append(op[2])
            continue
        flush()
        if op[0] == "erase":
            db.erase(op[1])
        else:
            db.set_covisibility(op[1], op[2])
    flush()


def bow_tables(bows):
    """Host BowVectors in the transform_batch_device layout: words, values, counts."""
    from orbslam2commentedbyxcm_amd.database import bow_arrays
    arrs = [bow_arrays(b) for b in bows]
    cap = max([len(w) for w, _ in arrs] + [1])
    W, V, N = np.zeros((len(arrs), cap), np.int32), np.zeros((len(arrs), cap), np.float64), np.zeros(len(arrs), np.int32)
    for i, (w, v) in enumerate(arrs):
        W[i, :len(w)], V[i, :len(w)], N[i] = w, v, len(w)
    return dict(word=W, value=V, n=N)


def run_add(db, ids, bows, io=None, decoy=None, decoy_ids=None):
    """kfdb_add_batch_device of host BowVectors through io (a stream_order I/O object; default:
    blocking uploads, a device synchronise around the call)."""
    import torch

    import stream_order as SO
    io = io or SO.SyncIO(torch.device("cuda", db.device))
    T, Q = bow_tables(bows), bow_tables(bows if decoy is None else decoy)
    d = {k: io.up(T[k], Q[k]) for k in T}
    h_ids = io.host(np.asarray(ids, np.int32), decoy_ids)
    io.begin()
    db.add_batch_device(h_ids, d["word"], d["value"], d["n"], T["word"].shape[1], stream=io.stream_ptr)
    io.end()


LOOP_CONNECTED = ([3, 7, 11], [])          # GetConnectedKeyFrames() of the two loop queries
LOOP_MIN_SCORE = (0.01, 0.0)
DECOY_MIN_SCORE = (0.4, 0.3)              # in place of LOOP_MIN_SCORE until an ordered run's real upload
QUERY_KEYS = ("score", "cand", "ncand", "loop_cand", "loop_ncand")


def run_queries(db, query, score_ids, reloc_queries, io=None, decoy=None, max_cand=32, min_score=LOOP_MIN_SCORE,
                switch_io=None):
    """kfdb_score_device of one query against score_ids, then one batched
    DetectRelocalizationCandidates and one batched DetectLoopCandidates of reloc_queries, on io's
    stream with nothing read back in between.  decoy = (query, reloc_queries) with the same words.
    switch_io: the I/O object whose stream the calls after the score go to (the stream switch)."""
    import torch

    import stream_order as SO
    io = io or SO.SyncIO(torch.device("cuda", db.device))
    dq, dr = (query, reloc_queries) if decoy is None else decoy
    T, Q = bow_tables([query]), bow_tables([dq])
    R, RQ = bow_tables(reloc_queries), bow_tables(dr)
    q = {k: io.up(T[k], Q[k]) for k in T}
    r = {k: io.up(R[k], RQ[k]) for k in R}
    d_ids = io.up(np.asarray(score_ids, np.int32))
    d_score = io.full((len(score_ids),), -7.0, torch.float32)
    B = len(reloc_queries)
    conn_off = np.concatenate([[0], np.cumsum([len(c) for c in LOOP_CONNECTED[:B]])]).astype(np.int32)
    conn_ids = np.asarray([i for c in LOOP_CONNECTED[:B] for i in c] + [0], np.int32)
    d_coff, d_cids = io.up(conn_off), io.up(conn_ids)
    d_min = io.up(np.asarray(min_score[:B], np.float32), None if decoy is None else np.asarray(DECOY_MIN_SCORE[:B], np.float32))
    out = {"cand": io.full((B, max_cand), -1, torch.int32), "ncand": io.full((B,), -9, torch.int32), "words": None,
           "score": None}
    loop = {"cand": io.full((B, max_cand), -1, torch.int32), "ncand": io.full((B,), -9, torch.int32), "words": None,
            "score": None}
    io.begin()
    db.score_device(q["word"], q["value"], q["n"], T["word"].shape[1], d_ids, d_score, stream=io.stream_ptr)
    io.end()
    io2 = switch_io or io
    db.detect_relocalization_candidates_device(r["word"], r["value"], r["n"], R["word"].shape[1], out,
                                               stream=io2.stream_ptr)
    if switch_io is None:
        io.end()
    else:
        switch_io.first_stream_done = io.stream.query()      # read as soon as the switched call returns
    db.detect_loop_candidates_device(r["word"], r["value"], r["n"], R["word"].shape[1], d_coff, d_cids, d_min, loop,
                                     stream=io2.stream_ptr)
    if switch_io is None:
        io.end()
    return dict(score=io.down(d_score), cand=io2.down(out["cand"]), ncand=io2.down(out["ncand"]),
                loop_cand=io2.down(loop["cand"]), loop_ncand=io2.down(loop["ncand"]))


def test_device_runners_equal_model(voc):
    """The runners of the stream-order tests against the model: add + score at n = 65 and one
    batched relocalisation detection."""
    rng = np.random.default_rng(165)
    n = 65
    bows = [M.random_bow(rng, int(rng.integers(1, 301))) for _ in range(n)]
    model, db = M.Database(), _db(voc, n)
    for i, b in enumerate(bows):
        model.add(i, b)
    run_add(db, list(range(n)), bows)
    ids = [int(i) for i in rng.permutation(n)]
    q = M.random_bow(rng, 150)
    rq = [M.perturbed(rng, bows[7], 0.7, 20), M.random_bow(rng, 200)]
    got = run_queries(db, q, ids, rq, max_cand=n)
    assert np.array_equal(_u32(got["score"]), _u32(model.score(q, ids)))
    for b, x in enumerate(rq):
        want = model.detect_relocalization_candidates(x)
        assert got["cand"][b, :got["ncand"][b]].tolist() == want, b
    assert got["ncand"].max() > 0
    for b, x in enumerate(rq):
        want = model.detect_loop_candidates(x, set(LOOP_CONNECTED[b]), LOOP_MIN_SCORE[b])
        assert got["loop_cand"][b, :got["loop_ncand"][b]].tolist() == want, ("loop", b)
    db.close()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_diag(model, words, score, b, nkf):
    """The stages of query b against the model's: shared-word counts, then si."""
    want_w = np.zeros(nkf, np.int32)
    want_s = np.full(nkf, -1.0, np.float32)
    for k, w in model.diag["words"].items():
        want_w[k] = w
    for k, s in model.diag["scores"].items():
        want_s[k] = s
    assert np.array_equal(words[b], want_w), ("sharing stage", b, np.nonzero(words[b] != want_w)[0][:8])
    assert np.array_equal(_u32(score[b]), _u32(want_s)), ("scoring stage", b)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_score_device_matches_model(voc, n):
    rng = np.random.default_rng(100 + n)
    model = M.Database()
    bows = []
    for i in range(n):
        nw = (0, 300, 1, 64, 65)[i] if i < 5 and n > 5 else int(rng.integers(0, 301))
        bows.append(dict(bows[3]) if i % 9 == 8 else M.random_bow(rng, nw))  # duplicates of one keyframe among them
        model.add(i, bows[-1])
    db = _db(voc, n)
    db.add_batch(list(range(n)), bows)
    ids = [int(i) for i in rng.permutation(n)] + [0]
    for q in (M.random_bow(rng, 150), bows[n // 2], {}, {5: 1.0}):
        got = db.score(q, ids)
        assert np.array_equal(_u32(got), _u32(model.score(q, ids)))
    db.close()


def test_relocalization_single_and_batch_match_model(voc):
    ops, queries = M.reloc_scene(RELOC_SEED)
    nkf = 300
    model = M.replay(ops)
    one, many = _db(voc, nkf), _db(voc, nkf)
    _apply(one, ops)
    _apply(many, ops)
    assert one.size() == len(model.live)
    want = []
    for q in queries:  # one call at a time
        want.append(model.detect_relocalization_candidates(q))
        assert one.DetectRelocalizationCandidates(q) == want[-1]
    assert want[2] == [] and want[5] == []  # the empty query, the query that shares no word
    assert np.array_equal(_u32(one.reloc_scores()), _u32(model.reloc_scores(nkf)))
    # the same 8 queries as one batch on a fresh identical database
    model2 = M.replay(ops)
    cands, words, score = many.detect_relocalization_candidates_batch(queries, diagnostics=True)
    for b, q in enumerate(queries):
        assert model2.detect_relocalization_candidates(q) == want[b]
        _check_diag(model2, words, score, b, nkf)
        assert cands[b] == want[b], b
    assert np.array_equal(_u32(many.reloc_scores()), _u32(model.reloc_scores(nkf)))
    assert np.array_equal(_u32(many.reloc_scores()), _u32(one.reloc_scores()))
    # an empty database: after clear(), and a fresh one
    many.clear()
    assert many.size() == 0 and many.DetectRelocalizationCandidates(queries[0]) == []
    fresh = _db(voc, 8)
    assert fresh.DetectRelocalizationCandidates(queries[0]) == []
    for d in (one, many, fresh):
        d.close()


def test_order_after_erase_and_add_again(voc):
    """List order = (smallest shared word, add order): three equal keyframes come out in
    add order, a keyframe added again goes to the end, and a later keyframe that shares a
    smaller word comes first."""
    same = {1: 0.5, 2: 0.5}
    q = {0: 0.25, 1: 0.375, 2: 0.375}
    model, db = M.Database(), _db(voc, 8)
    for i in range(3):
        model.add(i, same)
        db.add(i, same)
    assert db.DetectRelocalizationCandidates(q) == model.detect_relocalization_candidates(q) == [0, 1, 2]
    model.erase(0)
    db.erase(0)
    assert db.DetectRelocalizationCandidates(q) == model.detect_relocalization_candidates(q) == [1, 2]
    model.add(0, same)
    db.add(0, same)
    assert db.DetectRelocalizationCandidates(q) == model.detect_relocalization_candidates(q) == [1, 2, 0]
    model.add(5, {0: 0.5, 2: 0.5})
    db.add(5, {0: 0.5, 2: 0.5})
    assert db.DetectRelocalizationCandidates(q) == model.detect_relocalization_candidates(q) == [5, 1, 2, 0]
    assert db.DetectLoopCandidates(q, [2], 0.0) == model.detect_loop_candidates(q, [2], 0.0) == [5, 1, 0]
    db.close()


def test_loop_single_and_batch_match_model(voc):
    ops, queries = M.loop_scene(LOOP_SEED)
    nkf = 120
    model = M.replay(ops)
    db = _db(voc, nkf)
    _apply(db, ops)
    want = []
    for bow, conn, ms in queries:
        want.append(model.detect_loop_candidates(bow, conn, ms))
        assert db.DetectLoopCandidates(bow, conn, ms) == want[-1]
    cands, words, score = db.detect_loop_candidates_batch([q[0] for q in queries], [q[1] for q in queries],
                                                          [q[2] for q in queries], diagnostics=True)
    for b, (bow, conn, ms) in enumerate(queries):
        assert model.detect_loop_candidates(bow, conn, ms) == want[b]
        _check_diag(model, words, score, b, nkf)
        assert cands[b] == want[b], b
    # min_score above, below and equal to a candidate's own score; min_score as the
    # bestAccScore floor (cc:145) at 0 and below it
    bow, conn, _ = queries[1]
    model.detect_loop_candidates(bow, conn, 0.0)
    for s in sorted(set(model.diag["scores"].values()))[:6]:
        for ms in (s, np.nextafter(s, np.float32(2)), np.nextafter(s, np.float32(-1)), np.float32(0), np.float32(-1)):
            assert db.DetectLoopCandidates(bow, conn, ms) == model.detect_loop_candidates(bow, conn, ms), ms
    assert db.DetectLoopCandidates(bow, [], 0.0) == model.detect_loop_candidates(bow, [], 0.0)
    assert db.DetectLoopCandidates({}, conn, 0.0) == []
    db.close()


def test_errors(voc):
    from orbslam2commentedbyxcm_amd import KeyFrameDatabase, OrbxError
    from orbslam2commentedbyxcm_amd import _lib as L
    from orbslam2commentedbyxcm_amd.vocabulary import ORBVocabulary

    def code(fn, *a):
        with pytest.raises(OrbxError) as e:
            fn(*a)
        return e.value.code

    db = KeyFrameDatabase(voc, 4, 8)
    bow = {1: 0.5, 2: 0.5}
    db.add(0, bow)
    assert code(db.add, 0, bow) == L.ORBX_ERR_STATE                    # duplicate live id
    assert code(db.add_batch, [1, 1], [bow, bow]) == L.ORBX_ERR_STATE
    assert code(db.add, 4, bow) == L.ORBX_ERR_ARG                      # id outside [0, max_keyframes)
    assert code(db.add, 1, {w: 1 / 9 for w in range(9)}) == L.ORBX_ERR_CAPACITY  # cap overflow
    assert db.size() == 1
    assert code(db.erase, 2) == L.ORBX_ERR_STATE
    assert code(db.set_covisibility, 0, list(range(11))) == L.ORBX_ERR_ARG
    db.add_batch([1, 2, 3], [bow, bow, bow])
    assert db.size() == 4
    assert code(db.add, 2, bow) == L.ORBX_ERR_CAPACITY                 # full database
    assert code(db.DetectRelocalizationCandidates, bow, 2) == L.ORBX_ERR_CAPACITY  # 4 candidates, room for 2
    db.erase(2)
    db.add(2, bow)
    assert db.DetectRelocalizationCandidates(bow) == [0, 1, 3, 2]
    db.close()
    V2 = ORBVocabulary(0)
    assert V2.loadFromText(VS.make_vocab(72, k=4, L=2, scoring=1).text())
    h = C.c_void_p()
    assert L.lib().orbx_kfdb_create(V2._h, 4, 8, C.byref(h)) == L.ORBX_ERR_UNSUPPORTED and not h.value
    assert code(KeyFrameDatabase, V2, 4, 8) == L.ORBX_ERR_UNSUPPORTED
    assert code(V2.score, bow, bow) == L.ORBX_ERR_UNSUPPORTED
    assert voc.score(bow, {2: 1.0}) == M.l1_score(bow, {2: 1.0})
    V2.close()


def test_end_to_end_transform_add_detect(oracle, orbx_built):
    """transform_batch_device -> add_batch_device -> detect_relocalization_candidates_device,
    all in HBM on the vocabulary's stream, against the model fed with the C oracle's
    transform of the same descriptors."""
    import torch

    from orbslam2commentedbyxcm_amd import KeyFrameDatabase
    from orbslam2commentedbyxcm_amd.vocabulary import ORBVocabulary

    t = VS.make_vocab(81, k=10, L=3)
    text = t.text()
    V, O = ORBVocabulary(0), oracle.Vocab(text)
    assert V.loadFromText(text)
    rng = np.random.default_rng(82)
    nkf, cap, nq = 24, 256, 6
    counts = [int(c) for c in rng.integers(150, cap + 1, size=nkf)]
    desc = np.zeros((nkf, cap, 32), np.uint8)
    for b in range(nkf):
        if b % 4:   # a place seen before: most descriptors of the previous keyframe, some new
            desc[b] = desc[b - 1]
            fresh = rng.random(cap) < 0.3
            desc[b][fresh] = VS.queries(900 + b, t, cap)[fresh]
        else:
            desc[b] = VS.queries(900 + b, t, cap)
    # queries: perturbed copies of stored keyframes' descriptors
    src = [int(s) for s in rng.integers(0, nkf, size=nq)]
    qdesc = desc[src].copy()
    qcounts = [counts[s] for s in src]
    for b in range(nq):
        for i in rng.choice(cap, size=40, replace=False):
            qdesc[b, i] = VS._flip(rng, qdesc[b, i], int(rng.integers(1, 12)))

    def transform(d, n):
        out = ORBVocabulary.alloc_batch_outputs(len(n), cap)
        V.transform_batch_device(torch.from_numpy(d).cuda(), torch.tensor(n, dtype=torch.int32).cuda(), cap, 4, out)
        torch.cuda.synchronize()  # the inputs are released on return
        return out

    def bows(d, n):
        res = []
        for b in range(len(n)):
            bw, bv = O.transform(d[b, :n[b]], 4)[:2]
            res.append({int(w): float(v) for w, v in zip(bw, bv)})
        return res

    torch.cuda.synchronize()
    kf = transform(desc, counts)
    db = KeyFrameDatabase(V, nkf, cap)
    db.add_batch_device(list(range(nkf)), kf["bow_word"], kf["bow_value"], kf["nbow"], cap, stream=V.stream)
    model = M.Database()
    for b, bow in enumerate(bows(desc, counts)):
        model.add(b, bow)
    for b in range(nkf):
        lst = [int(x) for x in rng.integers(0, nkf, size=int(rng.integers(0, 11))) if x != b]
        model.set_covisibility(b, lst)
        db.set_covisibility(b, lst)
    q = transform(qdesc, qcounts)
    out = db.alloc_outputs(nq, nkf, diagnostics=True)
    db.detect_relocalization_candidates_device(q["bow_word"], q["bow_value"], q["nbow"], cap, out, stream=V.stream)
    cands, words, score = db._download(out)
    nonempty = 0
    for b, bow in enumerate(bows(qdesc, qcounts)):
        want = model.detect_relocalization_candidates(bow)
        _check_diag(model, words, score, b, nkf)
        assert cands[b] == want, b
        nonempty += bool(want)
    assert nonempty == nq  # every query is a view of a stored keyframe
    assert np.array_equal(_u32(db.reloc_scores()), _u32(model.reloc_scores(nkf)))
    db.close()
    V.close()


@pytest.mark.parametrize("max_kf", [1025, 8192])
def test_scattered_ids_up_to_the_ceiling(voc, max_kf):
    """The relocalisation scene with its ids scattered over [0, max_kf), the last id
    included: the candidate sort takes 2 (1025) and 8 (8192, the ceiling) keys per thread."""
    ops, queries = M.reloc_scene(RELOC_SEED)
    rng = np.random.default_rng(max_kf)
    remap = rng.choice(max_kf - 1, size=300, replace=False)
    remap[7] = max_kf - 1
    ops = [(op[0], int(remap[op[1]])) + ((op[2],) if op[0] == "add" else ([int(remap[k]) for k in op[2]],)
                                         if op[0] == "covis" else ()) for op in ops]
    model = M.replay(ops)
    db = _db(voc, max_kf, 128)
    _apply(db, ops)
    cands, words, score = db.detect_relocalization_candidates_batch(queries, diagnostics=True)
    for b, q in enumerate(queries):
        want = model.detect_relocalization_candidates(q)
        _check_diag(model, words, score, b, max_kf)
        assert cands[b] == want, b
    assert np.array_equal(_u32(db.reloc_scores()), _u32(model.reloc_scores(max_kf)))
    db.close()


def test_thousands_of_candidates(voc):
    """2500 keyframes that all pass the threshold (three variants of one place, covisibility
    lists in a ring): lists longer than the workgroup, repeats dropped all along the
    list, in both forms."""
    rng = np.random.default_rng(5)
    place = M.random_bow(rng, 40)
    variants = [place, M.perturbed(rng, place, 0.95, 2), M.perturbed(rng, place, 0.9, 3)]
    n, max_kf = 2500, 4096
    ids = [int(i) for i in rng.permutation(max_kf)[:n]]
    bows = [variants[int(v)] for v in rng.integers(0, 3, size=n)]
    model, db = M.Database(), _db(voc, max_kf, 64)
    for i, b in zip(ids, bows):
        model.add(i, b)
    db.add_batch(ids, bows)
    for j, i in enumerate(ids):
        lst = [ids[(j + 1) % n], ids[(j + 7) % n]]  # equal list lengths: every group passes 0.75 * best
        model.set_covisibility(i, lst)
        db.set_covisibility(i, lst)
    q = M.perturbed(rng, place, 0.97, 1)
    want = model.detect_relocalization_candidates(q)
    assert len(want) > 1024 and model.diag["removed_repeat"] and len(model.diag["scores"]) == n
    assert db.DetectRelocalizationCandidates(q) == want
    conn = ids[100:140]
    ms = sorted(set(model.diag["scores"].values()))[1]
    want = model.detect_loop_candidates(q, conn, ms)
    assert len(want) > 1024 and model.diag["dropped_by_min_score"] and model.diag["removed_repeat"]
    assert db.DetectLoopCandidates(q, conn, ms) == want
    db.close()
