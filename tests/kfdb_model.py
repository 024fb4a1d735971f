"""Pure-Python restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc:
31-307) and DBoW2's L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68),
with dicts and lists in place of std::map / std::list.  Python's float is the reference's
double and np.float32 its float.  The L1 expression holds no product, so no compiler can
fuse it and this restatement is exact: the tests compare ids, order, counts and score bit
patterns.

A keyframe is an id; its BowVector a dict {word: value} (iterated in ascending word
order, like the std::map).  The per-keyframe query marks (mnRelocQuery / mnRelocWords /
mRelocScore, mnLoopQuery / mnLoopWords / mLoopScore) live on ``KF`` objects and persist
between queries as they do in the reference.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def l1_score(v1: dict, v2: dict) -> float:
    """ScoringObject.cpp:23-68: the shared words in ascending order, one term at a time
    from 0.0, then -score / 2.0 (no shared word: -0.0)."""
    score = 0.0
    for w in sorted(v1):  # the two lower_bound walks visit exactly the shared words, ascending
        if w in v2:
            vi, wi = v1[w], v2[w]
            score += abs(vi - wi) - abs(vi) - abs(wi)  # cpp:41
    return -score / 2.0  # cpp:65


class KF:
    def __init__(self, kid: int, bow: dict):
        self.id = kid
        self.bow = {int(w): float(bow[w]) for w in sorted(bow)}
        self.best_covis: list = []   # GetBestCovisibilityKeyFrames(10): KF objects (erased ones included)
        self.reloc_query = -1        # mnRelocQuery (KeyFrame.cc:32-64 sets it to 0; query ids here start at 1)
        self.reloc_words = 0
        self.reloc_score = f32(0.0)  # mRelocScore: never initialised by KeyFrame.cc:32-64; pinned to 0.0f
        self.loop_query = -1
        self.loop_words = 0
        self.loop_score = f32(0.0)


class Database:
    def __init__(self):
        self.inv: dict = {}          # mvInvertedFile: word -> list of KF in add() order
        self.kfs: dict = {}          # every KF ever added by id (the newest object of that id)
        self.live: dict = {}
        self.nquery = 0              # F->mnId / pKF->mnId: one fresh id per query
        self.diag = None             # the last query's stages: words, scores

    # -- KeyFrameDatabase.cc:37-66 ------------------------------------------------------
    def add(self, kid: int, bow: dict) -> KF:
        assert kid not in self.live
        kf = KF(kid, bow)
        self.kfs[kid] = kf
        self.live[kid] = kf
        for w in kf.bow:                     # cc:40-42
            self.inv.setdefault(w, []).append(kf)
        return kf

    def erase(self, kid: int) -> None:
        kf = self.live.pop(kid)
        for w in kf.bow:                     # cc:49-58
            self.inv[w].remove(kf)

    def clear(self) -> None:                 # cc:63-66
        self.inv = {}
        self.live = {}

    def set_covisibility(self, kid: int, best: list) -> None:
        """The caller's GetBestCovisibilityKeyFrames(10) list of keyframe ids; an id that
        was never added stands for a keyframe outside the database (it is never a
        candidate) and is kept as a placeholder."""
        self.live[kid].best_covis = [int(b) for b in best[:10]]

    def _neigh(self, kid2: int):
        return self.kfs.get(kid2)

    def score(self, bow: dict, ids) -> list:
        """float si = mpVoc->score(query, KF) per id."""
        return [f32(l1_score(bow, self.live[i].bow)) for i in ids]

    # -- KeyFrameDatabase.cc:206-307 ----------------------------------------------------
    def detect_relocalization_candidates(self, bow: dict, stale_as_zero: bool = False) -> list:
        self.nquery += 1
        fid = self.nquery
        sharing = []
        for w in sorted(bow):                # cc:213-227
            for kf in self.inv.get(w, []):
                if kf.reloc_query != fid:
                    kf.reloc_words = 0
                    kf.reloc_query = fid
                    sharing.append(kf)
                kf.reloc_words += 1
        self.diag = {"words": {k.id: k.reloc_words for k in sharing}, "scores": {}, "removed_repeat": False,
                     "at_threshold": False}
        if not sharing:
            return []
        max_common = max(k.reloc_words for k in sharing)          # cc:233-238
        min_common = int(f32(max_common) * f32(0.8))              # cc:240
        self.diag["at_threshold"] = any(k.reloc_words == min_common for k in sharing)
        score_and_match = []
        scored = set()
        for kf in sharing:                   # cc:245-255
            if kf.reloc_words > min_common:
                si = f32(l1_score(bow, kf.bow))
                kf.reloc_score = si
                scored.add(kf.id)
                self.diag["scores"][kf.id] = si
                score_and_match.append((si, kf))
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = f32(0.0)                  # cc:261
        for si, kf in score_and_match:       # cc:265-286
            best_score, acc, best_kf = si, si, kf
            for kid2 in kf.best_covis:
                kf2 = self._neigh(kid2)
                if kf2 is None or kf2.reloc_query != fid:          # cc:275-276
                    continue
                s2 = kf2.reloc_score
                if stale_as_zero and kf2.id not in scored:
                    s2 = f32(0.0)
                acc = f32(acc + s2)
                if s2 > best_score:
                    best_kf, best_score = kf2, s2
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._select(acc_and_match, best_acc)

    # -- KeyFrameDatabase.cc:79-195 -----------------------------------------------------
    def detect_loop_candidates(self, bow: dict, connected, min_score) -> list:
        self.nquery += 1
        qid = self.nquery
        min_score = f32(min_score)
        connected = set(int(c) for c in connected)
        sharing = []
        for w in sorted(bow):                # cc:88-105
            for kf in self.inv.get(w, []):
                if kf.loop_query != qid:
                    kf.loop_words = 0
                    if kf.id not in connected:
                        kf.loop_query = qid
                        sharing.append(kf)
                kf.loop_words += 1
        self.diag = {"words": {k.id: k.loop_words for k in sharing}, "scores": {}, "removed_repeat": False,
                     "at_threshold": False, "dropped_by_min_score": False,
                     "dropped_by_connected": any(self.live[c].bow.keys() & bow.keys() for c in connected
                                                 if c in self.live)}
        if not sharing:
            return []
        max_common = max(k.loop_words for k in sharing)            # cc:115-120
        min_common = int(f32(max_common) * f32(0.8))               # cc:122
        self.diag["at_threshold"] = any(k.loop_words == min_common for k in sharing)
        score_and_match = []
        for kf in sharing:                   # cc:126-138
            if kf.loop_words > min_common:
                si = f32(l1_score(bow, kf.bow))
                kf.loop_score = si
                self.diag["scores"][kf.id] = si
                if si >= min_score:
                    score_and_match.append((si, kf))
                else:
                    self.diag["dropped_by_min_score"] = True
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = min_score                 # cc:145
        for si, kf in score_and_match:       # cc:149-173
            best_score, acc, best_kf = si, si, kf
            for kid2 in kf.best_covis:
                kf2 = self._neigh(kid2)
                if kf2 is not None and kf2.loop_query == qid and kf2.loop_words > min_common:  # cc:161
                    acc = f32(acc + kf2.loop_score)
                    if kf2.loop_score > best_score:
                        best_kf, best_score = kf2, kf2.loop_score
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._select(acc_and_match, best_acc)

    def _select(self, acc_and_match, best_acc) -> list:
        """cc:176-194 / 289-306."""
        retain = f32(f32(0.75) * best_acc)
        out, seen = [], set()
        for acc, kf in acc_and_match:
            if acc > retain:
                if kf.id not in seen:
                    out.append(kf.id)
                    seen.add(kf.id)
                else:
                    self.diag["removed_repeat"] = True
        return out

    def reloc_scores(self, n: int) -> np.ndarray:
        """reloc_score of the live keyframes by id (0 elsewhere), as the device keeps it."""
        out = np.zeros(n, np.float32)
        for kid, kf in self.live.items():
            out[kid] = kf.reloc_score
        return out


# ---- synthetic scenes shared by the CPU guards and the GPU tests ----------------------
def random_bow(rng, nwords: int, vocab_words: int = 1000) -> dict:
    """Sorted random words out of `vocab_words`, values L1-normalised in word order."""
    if nwords == 0:
        return {}
    words = np.sort(rng.choice(vocab_words, size=nwords, replace=False))
    vals = rng.uniform(0.05, 6.0, nwords)
    s = 0.0
    for v in vals:
        s += abs(float(v))
    return {int(w): float(v) / s for w, v in zip(words, vals)}


def perturbed(rng, bow: dict, keep: float, extra: int, vocab_words: int = 1000) -> dict:
    """A query near `bow`: a fraction of its words with new values plus a few fresh ones."""
    out = {w: float(rng.uniform(0.05, 6.0)) for w in bow if rng.random() < keep}
    for w in rng.choice(vocab_words, size=extra, replace=False):
        out.setdefault(int(w), float(rng.uniform(0.05, 6.0)))
    s = 0.0
    for w in sorted(out):
        s += abs(out[w])
    return {w: out[w] / s for w in sorted(out)} if s > 0 else {}


def reloc_scene(seed: int, nkf: int = 300):
    """The relocalisation scene: `nkf` ids of which some are erased again, covisibility
    lists that include erased ids, never-added ids, keyframes that share nothing with the
    queries, and fewer than 10 entries; then 8 queries -- views of the places the
    keyframes saw (runs of 8 consecutive ids share a place), an empty one and one over words no keyframe uses (words >= 900 are left
    to it).  Returns (ops, queries): ops is a list of ("add", id, bow) / ("erase", id) /
    ("covis", id, list)."""
    rng = np.random.default_rng(seed)
    ops = []
    bows = {}
    base = [random_bow(rng, int(rng.integers(20, 60)), 900) for _ in range(12)]  # places seen again and again
    for kid in range(nkf):
        if kid % 37 == 5:
            bow = {}
        elif kid % 11 == 3:
            bow = dict(bows[kid - 1])  # duplicate of its predecessor
        else:
            bow = perturbed(rng, base[(kid // 8) % len(base)], 0.8, int(rng.integers(0, 40)), 900)
        bows[kid] = bow
        ops.append(("add", kid, bow))
    erased = [int(e) for e in rng.choice(nkf, size=nkf // 10, replace=False)]
    for e in erased:
        ops.append(("erase", e))
    live = [k for k in range(nkf) if k not in erased]
    for kid in live:
        n = int(rng.integers(0, 11))
        near = [int(min(nkf - 1, max(0, kid + d))) for d in rng.integers(-6, 7, size=n)]
        lst = [k for k in near if k != kid]
        if rng.random() < 0.3 and lst:
            lst[int(rng.integers(0, len(lst)))] = int(rng.choice(erased))
        if rng.random() < 0.2 and lst:
            lst[int(rng.integers(0, len(lst)))] = int(rng.integers(0, nkf))
        ops.append(("covis", kid, lst))
    queries = []
    for i in range(8):
        if i == 2:
            queries.append({})
        elif i == 5:
            queries.append({w + 900: v for w, v in random_bow(rng, 30, 100).items()})
        else:
            queries.append(perturbed(rng, base[int(rng.integers(0, len(base)))], 0.85, 10, 900))
    return ops, queries


def replay(ops, db=None) -> Database:
    db = db or Database()
    for op in ops:
        if op[0] == "add":
            db.add(op[1], op[2])
        elif op[0] == "erase":
            db.erase(op[1])
        else:
            db.set_covisibility(op[1], op[2])
    return db


def loop_scene(seed: int, nkf: int = 120):
    """The loop scene: ops as in reloc_scene, and queries (bow, connected ids, min_score):
    each query is a stored keyframe, its connected set the neighbours in id order, and
    min_score the lowest L1 score against them (LoopClosing.cc:119-132), or the median si of
    the scored candidates, or that float's neighbours above and below."""
    rng = np.random.default_rng(seed)
    ops, _ = reloc_scene(seed, nkf)
    db = replay(ops)
    live = sorted(db.live)
    queries = []
    for i in range(8):
        kid = live[int(rng.integers(10, len(live) - 10))]
        bow = db.live[kid].bow
        connected = [k for k in range(kid - 3, kid + 4) if k in db.live]
        probe = replay(ops)
        probe.detect_loop_candidates(bow, connected, 0.0)
        scored = sorted(probe.diag["scores"].values())
        if i % 4 == 0 or not scored:
            ms = min([f32(l1_score(bow, db.live[k].bow)) for k in connected if k != kid] or [f32(0.0)])
        else:
            s = scored[len(scored) // 2]  # a scored candidate's own si
            ms = s if i % 4 == 1 else (np.nextafter(s, f32(2.0)) if i % 4 == 2 else np.nextafter(s, f32(-1.0)))
        queries.append((bow, connected, f32(ms)))
    return ops, queries
