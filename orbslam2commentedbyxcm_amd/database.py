"""KeyFrameDatabase mirror (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:31-307) on
the device-resident database in liborbx.so (orbx_kfdb_*, include/orbx.h).

Method names follow the reference: ``add``, ``erase``, ``clear``, ``DetectLoopCandidates``,
``DetectRelocalizationCandidates``.  Keyframes are caller-chosen integer ids; a BowVector is
a dict {word: value} (the ``ORBVocabulary.transform`` result) or a pair of arrays (words
ascending, values).  The ``*_device`` methods take torch tensors in the
``ORBVocabulary.transform_batch_device`` layout and leave their results in HBM.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L

I32P = C.POINTER(C.c_int32)
DP = C.POINTER(C.c_double)
FP = C.POINTER(C.c_float)

MAX_KEYFRAMES = 8192  # ORBX_KFDB_MAX_KEYFRAMES
MAX_WORDS = 8192      # words per keyframe / query
COVIS = 10            # GetBestCovisibilityKeyFrames(10)


def bow_arrays(bow):
    """BowVector -> (words int32 ascending, values float64)."""
    if isinstance(bow, dict):
        ws = sorted(bow)
        return np.asarray(ws, np.int32), np.asarray([bow[w] for w in ws], np.float64)
    w, v = bow
    return np.ascontiguousarray(w, np.int32), np.ascontiguousarray(v, np.float64)


def bow_score(v1, v2) -> float:
    """L1Scoring::score(v1, v2) (DBoW2 ScoringObject.cpp:23-68) on the host (orbx_bow_score)."""
    w1, a1 = bow_arrays(v1)
    w2, a2 = bow_arrays(v2)
    out = C.c_double()
    L.check(L.lib().orbx_bow_score(w1.ctypes.data_as(I32P), a1.ctypes.data_as(DP), len(w1), w2.ctypes.data_as(I32P),
                                   a2.ctypes.data_as(DP), len(w2), C.byref(out)))
    return out.value


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class KeyFrameDatabase:
    def __init__(self, voc, max_keyframes: int = 4096, cap: int = 2048):
        """KeyFrameDatabase(voc): on the vocabulary's device, for ids below `max_keyframes`
        of up to `cap` words each."""
        self._h = None
        self._destroy = L.lib().orbx_kfdb_destroy  # held: module globals may be gone at exit
        self._voc = voc  # the vocabulary outlives the database
        self.max_keyframes, self.cap = int(max_keyframes), int(cap)
        h = C.c_void_p()
        L.check(L.lib().orbx_kfdb_create(voc._h, self.max_keyframes, self.cap, C.byref(h)))
        self._h = h
        self.device = voc.device
        L.track(self)

    def close(self) -> None:
        """Release the database (orbx_kfdb_destroy); idempotent."""
        self._release()

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self._release()

    def _release(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    @property
    def stream(self) -> int:
        return L.lib().orbx_kfdb_stream(self._h)

    def size(self) -> int:
        n = C.c_int()
        L.check(L.lib().orbx_kfdb_info(self._h, None, None, C.byref(n)))
        return n.value

    # -- membership -----------------------------------------------------------------
    def _torch_dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _upload(self, bows):
        """Host BowVectors -> tensors in the transform_batch_device layout."""
        import torch
        arrs = [bow_arrays(b) for b in bows]
        cap = max([len(w) for w, _ in arrs] + [1])
        W = np.zeros((len(arrs), cap), np.int32)
        V = np.zeros((len(arrs), cap), np.float64)
        N = np.zeros(len(arrs), np.int32)
        for i, (w, v) in enumerate(arrs):
            W[i, :len(w)], V[i, :len(w)], N[i] = w, v, len(w)
        dev = self._torch_dev()
        return torch.from_numpy(W).to(dev), torch.from_numpy(V).to(dev), torch.from_numpy(N).to(dev), cap

    def add(self, kf_id: int, bow) -> None:
        """KeyFrameDatabase::add(pKF) with pKF->mBowVec = bow (orbx_kfdb_add)."""
        w, v = bow_arrays(bow)
        L.check(L.lib().orbx_kfdb_add(self._h, int(kf_id), w.ctypes.data_as(I32P), v.ctypes.data_as(DP), len(w)))

    def add_batch(self, ids, bows) -> None:
        W, V, N, cap = self._upload(bows)
        self.add_batch_device(ids, W, V, N, cap)
        self._sync()

    def add_batch_device(self, ids, bow_word, bow_value, nbow, cap: int, stream=None) -> None:
        """orbx_kfdb_add_batch_device: keyframe ids[i] stores row i of the device tensors."""
        ids = np.ascontiguousarray(ids, np.int32)
        L.check(L.lib().orbx_kfdb_add_batch_device(self._h, len(ids), ids.ctypes.data_as(I32P), _p(bow_word),
                                                   _p(bow_value), _p(nbow), int(cap),
                                                   C.c_void_p(stream) if stream else None))

    def erase(self, kf_id: int) -> None:
        L.check(L.lib().orbx_kfdb_erase(self._h, int(kf_id)))

    def clear(self) -> None:
        L.check(L.lib().orbx_kfdb_clear(self._h))

    def set_covisibility(self, kf_id: int, best) -> None:
        """The keyframe's GetBestCovisibilityKeyFrames(10) list (ids, in its order)."""
        b = np.ascontiguousarray(best, np.int32)
        L.check(L.lib().orbx_kfdb_set_covisibility(self._h, int(kf_id), b.ctypes.data_as(I32P), len(b)))

    def reloc_scores(self) -> np.ndarray:
        """mRelocScore by id (0 for ids that are not stored)."""
        out = np.zeros(self.max_keyframes, np.float32)
        L.check(L.lib().orbx_kfdb_reloc_scores(self._h, out.ctypes.data_as(FP)))
        return out

    def _sync(self):
        import torch
        torch.cuda.synchronize(self.device)

    # -- scoring and detection ------------------------------------------------------
    def score(self, bow, ids) -> np.ndarray:
        """float si = mpVoc->score(bow, KF) for the stored keyframes `ids` (float32)."""
        import torch
        W, V, N, cap = self._upload([bow])
        d_ids = torch.as_tensor(np.ascontiguousarray(ids, np.int32), device=self._torch_dev())
        out = torch.empty(len(d_ids), dtype=torch.float32, device=self._torch_dev())
        self.score_device(W, V, N, cap, d_ids, out)
        self._sync()
        return out.cpu().numpy()

    def score_device(self, qword, qvalue, qn, qcap: int, ids, out, stream=None) -> None:
        L.check(L.lib().orbx_kfdb_score_device(self._h, _p(qword), _p(qvalue), _p(qn), int(qcap), _p(ids),
                                               int(ids.numel()), _p(out), C.c_void_p(stream) if stream else None))

    def DetectRelocalizationCandidates(self, bow, max_cand: int | None = None) -> list:
        """vector<KeyFrame*> DetectRelocalizationCandidates(F) with F->mBowVec = bow: ids."""
        w, v = bow_arrays(bow)
        m = self.max_keyframes if max_cand is None else int(max_cand)
        cand = np.zeros(max(m, 1), np.int32)
        n = C.c_int()
        L.check(L.lib().orbx_kfdb_detect_relocalization_candidates(self._h, w.ctypes.data_as(I32P),
                                                                   v.ctypes.data_as(DP), len(w),
                                                                   cand.ctypes.data_as(I32P), m, C.byref(n)))
        return cand[:n.value].tolist()

    def DetectLoopCandidates(self, bow, connected, min_score: float, max_cand: int | None = None) -> list:
        """vector<KeyFrame*> DetectLoopCandidates(pKF, minScore) with pKF->mBowVec = bow and
        pKF->GetConnectedKeyFrames() = connected (ids)."""
        w, v = bow_arrays(bow)
        c = np.ascontiguousarray(list(connected), np.int32)
        m = self.max_keyframes if max_cand is None else int(max_cand)
        cand = np.zeros(max(m, 1), np.int32)
        n = C.c_int()
        L.check(L.lib().orbx_kfdb_detect_loop_candidates(self._h, w.ctypes.data_as(I32P), v.ctypes.data_as(DP), len(w),
                                                         c.ctypes.data_as(I32P), len(c), float(min_score),
                                                         cand.ctypes.data_as(I32P), m, C.byref(n)))
        return cand[:n.value].tolist()

    def alloc_outputs(self, batch: int, max_cand: int, diagnostics: bool = False) -> dict:
        import torch
        dev = self._torch_dev()
        out = {"cand": torch.full((batch, max_cand), -1, dtype=torch.int32, device=dev),
               "ncand": torch.zeros(batch, dtype=torch.int32, device=dev), "words": None, "score": None}
        if diagnostics:
            out["words"] = torch.zeros(batch, self.max_keyframes, dtype=torch.int32, device=dev)
            out["score"] = torch.zeros(batch, self.max_keyframes, dtype=torch.float32, device=dev)
        self._sync()  # the fills run on torch's stream, the database on its own
        return out

    def detect_relocalization_candidates_device(self, qword, qvalue, qn, qcap: int, out: dict, stream=None) -> None:
        """Batched DetectRelocalizationCandidates over device tensors (qword / qvalue [B][qcap],
        qn [B]); `out` from alloc_outputs.  Equal to B single calls in order."""
        L.check(L.lib().orbx_kfdb_detect_relocalization_candidates_device(
            self._h, int(qn.numel()), _p(qword), _p(qvalue), _p(qn), int(qcap), _p(out["cand"]),
            int(out["cand"].shape[1]), _p(out["ncand"]), _p(out["words"]), _p(out["score"]),
            C.c_void_p(stream) if stream else None))

    def detect_loop_candidates_device(self, qword, qvalue, qn, qcap: int, conn_off, conn_ids, min_score, out: dict,
                                      stream=None) -> None:
        """Batched DetectLoopCandidates: conn_off [B + 1] / conn_ids the connected sets as CSR,
        min_score [B] float32 (device tensors)."""
        L.check(L.lib().orbx_kfdb_detect_loop_candidates_device(
            self._h, int(qn.numel()), _p(qword), _p(qvalue), _p(qn), int(qcap), _p(conn_off), _p(conn_ids),
            _p(min_score), _p(out["cand"]), int(out["cand"].shape[1]), _p(out["ncand"]), _p(out["words"]),
            _p(out["score"]), C.c_void_p(stream) if stream else None))

    def detect_relocalization_candidates_batch(self, bows, max_cand: int | None = None, diagnostics: bool = False):
        """Host BowVectors in, list of candidate id lists out (and the diagnostics arrays)."""
        W, V, N, cap = self._upload(bows)
        out = self.alloc_outputs(len(bows), self.max_keyframes if max_cand is None else max_cand, diagnostics)
        self.detect_relocalization_candidates_device(W, V, N, cap, out)
        return self._download(out)

    def detect_loop_candidates_batch(self, bows, connected, min_scores, max_cand: int | None = None,
                                     diagnostics: bool = False):
        import torch
        W, V, N, cap = self._upload(bows)
        off = np.zeros(len(bows) + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in connected])
        ids = np.asarray([i for c in connected for i in c] + [0], np.int32)
        dev = self._torch_dev()
        out = self.alloc_outputs(len(bows), self.max_keyframes if max_cand is None else max_cand, diagnostics)
        self.detect_loop_candidates_device(W, V, N, cap, torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev),
                                           torch.as_tensor(np.asarray(min_scores, np.float32), device=dev), out)
        return self._download(out)

    def _download(self, out):
        self._sync()
        n = out["ncand"].cpu().numpy()
        c = out["cand"].cpu().numpy()
        cands = [c[b, :min(int(n[b]), c.shape[1])].tolist() for b in range(len(n))]
        if out["words"] is None:
            return cands
        return cands, out["words"].cpu().numpy(), out["score"].cpu().numpy()
