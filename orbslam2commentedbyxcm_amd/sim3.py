"""Sim3Solver on the GPU (include/orbx.h, csrc/orbx_sim3.hip).

Sim3Solver mirrors include/Sim3Solver.h (src/Sim3Solver.cc:37-534): Horn's closed form under
RANSAC between the matched MapPoints of two keyframes, as LoopClosing::ComputeSim3 drives it
(LoopClosing.cc:243-377).  One candidate on host arrays keeps the reference's surface
(construction, SetRansacParameters, iterate, find, GetEstimatedRotation / Translation /
Scale); set_batch_device / iterate_batch_device run B candidates resident in HBM.

The library owns no random generator: the draws of every iteration are an input
(`reference_draws` gives the reference's, over the C library's rand()).
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L

F32P = C.POINTER(C.c_float)
I32P = C.POINTER(C.c_int32)

RESULT_FIELDS = ("found", "no_more", "n_inliers", "inliers", "T12", "best_R", "best_t", "best_s", "best_inliers",
                 "best_iteration", "iterations", "n_pairs", "status")


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def reference_draws(n: int, iterations: int) -> np.ndarray:
    """(iterations, 3) i32: RandomInt(0, n - 1 - j) for the three draws of every iteration
    (DUtils/Random.cpp:47-49) from the C library's rand(), all iterations up front."""
    out = np.zeros((max(0, int(iterations)), 3), np.int32)
    L.check(L.lib().orbx_sim3_draws(out.ctypes.data_as(I32P), int(n), len(out)))
    return out


class Sim3Solver:
    """Owns the solver handle (workspace and per-candidate state) and, unless `matcher` is given,
    the matcher handle whose device and stream it runs on.

    With the candidate's arrays -- Sim3Solver(mp1, mp2, oct1, oct2, mp_pos, Tcw1, Tcw2,
    level_sigma2, K1, K2, fix_scale) -- it is the reference's object: mp1 / mp2 are
    vpKeyFrameMP1 / vpMatched12 as MapPoint ids into mp_pos ((n_mp, 3) GetWorldPos(); -1 where
    the reference skips the slot: NULL, isBad(), GetIndexInKeyFrame() < 0), oct1 / oct2 the
    octaves of the two keypoints, Tcw1 / Tcw2 12 floats (rows 0..2), K1 / K2 fx fy cx cy.
    Without them (Sim3Solver(max_batch=B, cap=..., max_iterations=...)) it serves the batch
    calls on device tensors."""

    def __init__(self, mp1=None, mp2=None, oct1=None, oct2=None, mp_pos=None, Tcw1=None, Tcw2=None,
                 level_sigma2=None, K1=None, K2=None, fix_scale: bool = False, draws=None, device: int = 0,
                 matcher=None, max_batch: int = 1, cap: int | None = None, max_iterations: int = 300):
        self._h = None
        self._m = None
        self._own = matcher is None
        self._matcher = matcher
        self.last = None
        self._keep = None
        self._cand = None
        if mp1 is not None:
            a, b = _i32(mp1).reshape(-1), _i32(mp2).reshape(-1)
            if len(b) > len(a):
                raise ValueError("vpMatched12 is longer than the keyframe's MapPoints")
            n1 = len(b)                                                  # cc:47 mN1 = vpMatched12.size()
            self._cand = dict(n1=n1, mp1=a[:n1].copy(), mp2=b, oct1=_i32(oct1).reshape(-1)[:n1].copy(),
                              oct2=_i32(oct2).reshape(-1)[:n1].copy(), pos=_f32(mp_pos).reshape(-1, 3),
                              Tcw1=_f32(Tcw1).reshape(-1)[:12].copy(), Tcw2=_f32(Tcw2).reshape(-1)[:12].copy(),
                              sig=_f32(level_sigma2).reshape(-1), K1=_f32(K1).reshape(-1)[:4].copy(),
                              K2=_f32(K2).reshape(-1)[:4].copy(), fix=bool(fix_scale),
                              draws=None if draws is None else _i32(draws).reshape(-1, 3))
            if len(self._cand["oct1"]) != n1 or len(self._cand["oct2"]) != n1:
                raise ValueError("one octave per slot of vpMatched12")
            cap = max(1, n1) if cap is None else cap
            if cap < n1:
                raise ValueError("cap below the number of slots")
        self.max_batch, self.cap, self.max_iterations = int(max_batch), int(1024 if cap is None else cap), 0
        lib = L.lib()
        if matcher is not None:
            self.device = matcher.device
            self._m = matcher._h
        else:
            self.device = int(device)
            m = C.c_void_p()
            L.check(lib.orbx_matcher_create(self.device, 0.6, 1, C.byref(m)))
            self._destroy_matcher = lib.orbx_matcher_destroy  # held: module globals may be gone at exit
            self._m = m
        self._destroy = lib.orbx_sim3_destroy
        L.track(self)
        self._reserve(max_iterations)
        if self._cand is not None:
            self.SetRansacParameters(max_iterations=max_iterations)    # cc:128

    def _reserve(self, max_iterations: int) -> None:
        if self._h is not None and max_iterations <= self.max_iterations:
            return
        if self._h is not None:
            self._destroy(self._h)
            self._h = None
        h = C.c_void_p()
        L.check(L.lib().orbx_sim3_create(self._m, self.max_batch, self.cap, int(max_iterations), C.byref(h)))
        self._h = h
        self.max_iterations = int(max_iterations)

    def close(self) -> None:
        """Release the handles (waits for the stream); idempotent.  A borrowed matcher is left alone."""
        if getattr(self, "_h", None):
            self._destroy(self._h)
        self._h = None
        if getattr(self, "_m", None) and self._own:
            self._destroy_matcher(self._m)
        self._m = None
        self._keep = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def last_call_us(self) -> float:
        """Wall time of the newest host iterate inside the library."""
        return float(L.lib().orbx_matcher_last_call_us(self._m))

    # ---- the reference's surface, one candidate on host arrays ----------------------------------
    def n_pairs(self) -> int:
        """N: the slots whose two ids are valid (cc:70-87)."""
        c = self._cand
        n_mp = len(c["pos"])
        return int(((c["mp1"] >= 0) & (c["mp1"] < n_mp) & (c["mp2"] >= 0) & (c["mp2"] < n_mp)).sum())

    def SetRansacParameters(self, probability: float = 0.99, min_inliers: int = 6, max_iterations: int = 300,
                            draws=None) -> None:
        """cc:132-185.  `draws` (max_iterations, 3) i32 replaces the constructor's; without
        either, reference_draws(N, max_iterations)."""
        c = self._cand
        if c is None:
            raise ValueError("no candidate: this solver serves the batch calls")
        self._reserve(max_iterations)
        if draws is not None:
            c["draws"] = _i32(draws).reshape(-1, 3)
        d = c["draws"]
        if d is None:
            d = reference_draws(self.n_pairs(), max_iterations)
        if len(d) < max_iterations:
            raise ValueError("fewer draws than max_iterations")
        d = np.ascontiguousarray(d[:max_iterations])
        n1 = np.array([c["n1"]], np.int32)
        q = L.Sim3Batch()
        q.batch, q.cap = 1, self.cap
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        q.n1, q.mp1, q.mp2, q.oct1, q.oct2 = ptr(n1), ptr(c["mp1"]), ptr(c["mp2"]), ptr(c["oct1"]), ptr(c["oct2"])
        q.n_mp, q.mp_pos, q.Tcw1, q.Tcw2 = len(c["pos"]), ptr(c["pos"]), ptr(c["Tcw1"]), ptr(c["Tcw2"])
        q.level_sigma2, q.nlevels = c["sig"].ctypes.data_as(F32P), len(c["sig"])
        q.K1, q.K2 = c["K1"].ctypes.data_as(F32P), c["K2"].ctypes.data_as(F32P)
        q.fix_scale, q.probability = int(c["fix"]), float(probability)
        q.min_inliers, q.max_iterations, q.draws = int(min_inliers), int(max_iterations), ptr(d)
        L.check(L.lib().orbx_sim3_set(self._h, C.byref(q)))
        self.last = None

    def iterate_host(self, n_iterations: int) -> dict:
        """One orbx_sim3_iterate: every output of the call as host arrays."""
        n1 = self._cand["n1"]
        o = dict(found=np.zeros(1, np.int32), no_more=np.zeros(1, np.int32), n_inliers=np.zeros(1, np.int32),
                 inliers=np.zeros(max(1, n1), np.uint8), T12=np.zeros(16, np.float32), best_R=np.zeros(9, np.float32),
                 best_t=np.zeros(3, np.float32), best_s=np.zeros(1, np.float32), best_inliers=np.zeros(1, np.int32),
                 best_iteration=np.zeros(1, np.int32), iterations=np.zeros(1, np.int32),
                 n_pairs=np.zeros(1, np.int32), status=np.zeros(1, np.int32))
        r = L.Sim3Result()
        for k in RESULT_FIELDS:
            setattr(r, k, C.c_void_p(o[k].ctypes.data))
        L.check(L.lib().orbx_sim3_iterate(self._h, int(n_iterations), C.byref(r)))
        o["inliers"] = o["inliers"][:n1]
        self.last = o
        return o

    def iterate(self, n_iterations: int):
        """cc:188-274: (T12 (4, 4) f32 or None, bNoMore, vbInliers (mN1,) bool, nInliers)."""
        o = self.iterate_host(n_iterations)
        T = o["T12"].reshape(4, 4).copy() if o["found"][0] else None
        return T, bool(o["no_more"][0]), o["inliers"].astype(bool), int(o["n_inliers"][0])

    def find(self):
        """cc:277-281: (T12 or None, vbInliers12, nInliers)."""
        T, _, inl, n = self.iterate(self.max_iterations)
        return T, inl, n

    def GetEstimatedRotation(self) -> np.ndarray:
        return (self.last["best_R"].reshape(3, 3).copy() if self.last else np.full((3, 3), np.nan, np.float32))

    def GetEstimatedTranslation(self) -> np.ndarray:
        return self.last["best_t"].copy() if self.last else np.full(3, np.nan, np.float32)

    def GetEstimatedScale(self) -> float:
        return float(self.last["best_s"][0]) if self.last else float("nan")

    # ---- B candidates in HBM ----------------------------------------------------------------------
    def set_batch_device(self, d_n1, d_mp1, d_mp2, d_oct1, d_oct2, d_mp_pos, d_Tcw1, d_Tcw2, level_sigma2, K1, K2,
                         d_draws, fix_scale: bool = False, probability: float = 0.99, min_inliers: int = 20,
                         max_iterations: int = 300, stream=None) -> None:
        """orbx_sim3_set_batch_device on device tensors: d_n1 (B,) i32, d_mp1 / d_mp2 / d_oct1 /
        d_oct2 (B, cap) i32, d_mp_pos (n_mp, 3) f32, d_Tcw1 / d_Tcw2 (B, 12) f32, d_draws
        (B, max_iterations, 3) i32 (kept alive here until the next set); level_sigma2, K1, K2
        host arrays.  Asynchronous on `stream` (a torch stream or a raw handle) or the matcher's;
        a null handle -- torch's default stream -- also means the matcher's, which is not
        ordered with torch's work: pass a torch.cuda.Stream to order the two."""
        B, cap = d_mp1.shape[0], d_mp1.shape[1]
        if tuple(d_draws.shape) != (B, max_iterations, 3):
            raise ValueError("d_draws must be (B, max_iterations, 3)")
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        sig, k1, k2 = _f32(level_sigma2).reshape(-1), _f32(K1).reshape(-1), _f32(K2).reshape(-1)
        q = L.Sim3Batch()
        q.batch, q.cap = B, cap
        q.n1, q.mp1, q.mp2, q.oct1, q.oct2 = ptr(d_n1), ptr(d_mp1), ptr(d_mp2), ptr(d_oct1), ptr(d_oct2)
        q.n_mp, q.mp_pos, q.Tcw1, q.Tcw2 = int(d_mp_pos.shape[0]), ptr(d_mp_pos), ptr(d_Tcw1), ptr(d_Tcw2)
        q.level_sigma2, q.nlevels, q.K1, q.K2 = sig.ctypes.data_as(F32P), len(sig), k1.ctypes.data_as(F32P), \
            k2.ctypes.data_as(F32P)
        q.fix_scale, q.probability = int(bool(fix_scale)), float(probability)
        q.min_inliers, q.max_iterations, q.draws = int(min_inliers), int(max_iterations), ptr(d_draws)
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_sim3_set_batch_device(self._h, C.byref(q), s))
        self._keep = (d_n1, d_mp1, d_mp2, d_oct1, d_oct2, d_mp_pos, d_Tcw1, d_Tcw2, d_draws)
        self._cand = None

    def iterate_batch_device(self, n_iterations: int, stream=None, **out) -> None:
        """orbx_sim3_iterate_device: keyword arguments name the outputs wanted (RESULT_FIELDS:
        found, no_more, n_inliers, best_inliers, best_iteration, iterations, n_pairs, status
        (B,) i32; inliers (B, cap) u8; T12 (B, 16), best_R (B, 9), best_t (B, 3), best_s (B,)
        f32), each a device tensor.  Asynchronous on `stream` (or the matcher's)."""
        r = L.Sim3Result()
        for k, t in out.items():
            if k not in RESULT_FIELDS:
                raise ValueError(f"unknown output {k}")
            setattr(r, k, None if t is None else C.c_void_p(t.data_ptr()))
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_sim3_iterate_device(self._h, int(n_iterations), C.byref(r), s))
