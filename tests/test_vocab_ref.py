"""The oracle's DBoW2 frame transform against the reference's own compiled code.

DBoW2's BowVector.cpp and FeatureVector.cpp are the only part of the reference path that
builds without OpenCV: oracle/ref_dbow2.mk compiles them where they lie under
/root/reference into oracle/_ref/libdbow2_ref.so (with the harness
oracle/ref_dbow2_capi.cpp).  The oracle's per-feature tree walk
(TemplatedVocabulary.h:1220-1259, restated: TemplatedVocabulary.h includes OpenCV) feeds
the reference containers, which accumulate (addWeight / addIfNotExist), scale and
normalise exactly as the reference binary would; the result must equal the oracle's
own BowVector / FeatureVector bit for bit (doubles included).  The GPU vocabulary tests
compare liborbx with the oracle, so this pins k_vocab_frame's double arithmetic to the
reference's code.

tests/golden/dbow2_ref_frames.npz holds what the reference containers returned for every
case here (recorded by tests/golden/make_dbow2_ref.py from a run of that library).  The
oracle is compared with the record everywhere; where the library is there it is also run,
and must return the record.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import vocab_scenes as VS

GOLDEN = Path(__file__).resolve().parent / "golden" / "dbow2_ref_frames.npz"
LEVELSUP = [0, 2, 4]
EDGE_INPUTS = {"empty": (np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int32), 0, 0),
               "stopped": (np.array([3, 4]), np.array([0.0, 0.0]), np.array([1, 1]), 0, 0),
               "tfidf_dot": (np.array([7, 7, 7], np.int32), np.array([0.1, 0.2, 0.7]), np.array([2, 2, 2]), 0, 5),
               "idf_dot": (np.array([7, 7, 7], np.int32), np.array([0.1, 0.2, 0.7]), np.array([2, 2, 2]), 2, 5)}


@pytest.fixture(scope="module")
def ref(oracle):
    """The reference-built containers, or None where they cannot be built (the record alone
    is the reference's answer there)."""
    return oracle.ref_dbow2()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case_inputs(oracle, scoring, weighting, levelsup):
    """-> (the oracle's Vocab, the queries, their per-feature (word, weight, node))."""
    seed = 10 * scoring + weighting
    t = VS.make_vocab(seed, k=6, L=4, scoring=scoring, weighting=weighting, irregular=bool(seed % 2),
                      tie_frac=0.1, stop_frac=0.1)
    V = oracle.Vocab(t.text())
    assert V.ok
    q = VS.queries(seed + 7, t, 300)
    return V, q, V.transform_features(q, levelsup)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype or g.dtype.kind == w.dtype.kind
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)) if g.dtype == w.dtype else np.array_equal(g, w)


def _record(golden, key):
    return tuple(golden[f"{key}_{i}"] for i in range(5))


# every (scoring, weighting) family: L1 / L2 / chi-square / KL / Bhattacharyya / dot
# product x TF-IDF / TF / IDF / BINARY, regular, irregular, tied and stopped trees
CASES = [(s, w) for s in range(6) for w in range(4)]


@pytest.mark.parametrize("scoring,weighting", CASES)
@pytest.mark.parametrize("levelsup", LEVELSUP)
def test_oracle_frame_transform_matches_reference_containers(oracle, ref, golden, scoring, weighting, levelsup):
    V, q, (word, weight, node) = case_inputs(oracle, scoring, weighting, levelsup)
    got = V.transform(q, levelsup)
    want = _record(golden, f"s{scoring}w{weighting}l{levelsup}")
    if ref is not None:  # the library itself, where it is built: it returns the record
        _same(oracle.ref_frame(ref, word, weight, node, weighting, scoring), want)
    _same(got, want)
    assert len(want[4]) > 100  # features kept (BINARY trees of this generator may map them to few words)


def test_reference_containers_edge_cases(oracle, ref, golden):
    """No features; every feature stopped (weight 0); one word repeated (addWeight sums in
    feature order, addIfNotExist keeps the first)."""
    out = {k: _record(golden, f"edge_{k}") for k in EDGE_INPUTS}
    if ref is not None:
        for k, args in EDGE_INPUTS.items():
            _same(oracle.ref_frame(ref, *args), out[k])
    e, s = out["empty"], out["stopped"]
    assert len(e[0]) == 0 and len(e[2]) == 0
    assert len(s[0]) == 0 and len(s[2]) == 0
    a = out["tfidf_dot"]  # TF-IDF, dot product: summed / size
    assert a[1][0] == (0.1 + 0.2 + 0.7) / 1.0
    b = out["idf_dot"]  # IDF: first kept
    assert b[1][0] == 0.1
    assert list(a[4]) == [0, 1, 2]
