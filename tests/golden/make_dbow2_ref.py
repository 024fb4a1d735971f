"""Regenerate tests/golden/dbow2_ref_frames.npz (run from the repo root, where
oracle.ref_dbow2() can build the reference's DBoW2 containers).

The record is what that library returned -- the BowVector / FeatureVector of every case of
tests/test_vocab_ref.py, five arrays each (bow_word, bow_value, fv_node, fv_off, fv_idx) --
for the per-feature (word, weight, node) triples the oracle's tree walk produced from
seeded synthetic vocabularies and queries (tests/vocab_scenes.py).
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "tests"):
    sys.path.insert(0, str(p))
import test_vocab_ref as T  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.build()
L = O.ref_dbow2()
if L is None:
    raise SystemExit("the reference's DBoW2 containers are not built and cannot be built here")
out = {}
for scoring, weighting in T.CASES:
    for levelsup in T.LEVELSUP:
        V, q, (word, weight, node) = T.case_inputs(O, scoring, weighting, levelsup)
        for i, a in enumerate(O.ref_frame(L, word, weight, node, weighting, scoring)):
            out[f"s{scoring}w{weighting}l{levelsup}_{i}"] = a
for k, args in T.EDGE_INPUTS.items():
    for i, a in enumerate(O.ref_frame(L, *args)):
        out[f"edge_{k}_{i}"] = a
np.savez_compressed(T.GOLDEN, **out)
print("wrote", T.GOLDEN, len(out), "arrays,", T.GOLDEN.stat().st_size, "bytes")
