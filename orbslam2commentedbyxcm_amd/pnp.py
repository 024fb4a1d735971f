"""PnPsolver on the GPU (include/orbx.h, csrc/orbx_pnp.hip, csrc/orbx_epnp.h).

PnPsolver mirrors include/PnPsolver.h (src/PnPsolver.cc:80-1345): EPnP under RANSAC between a
lost frame's keypoints and the MapPoints a candidate keyframe matched to them, as
Tracking::Relocalization drives it (Tracking.cc:1511-1684).  One candidate on host arrays keeps
the reference's surface (construction from the frame's keypoints and vpMapPointMatches,
SetRansacParameters, iterate, find); set_batch_device / iterate_batch_device run B candidates
resident in HBM.

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

RESULT_FIELDS = L.PNP_RESULT_FIELDS


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def reference_draws(n: int, iterations: int) -> np.ndarray:
    """(iterations, 4) i32: RandomInt(0, n - 1 - j) for the four draws of every iteration
    (DUtils/Random.cpp:47-49) from the C library's rand(), all iterations up front."""
    out = np.zeros((max(0, int(iterations)), 4), np.int32)
    L.check(L.lib().orbx_pnp_draws(out.ctypes.data_as(I32P), int(n), len(out)))
    return out


def _fill(q, *, batch, cap, kps, n, matches, n_mp, mp_pos, sig, K, probability, min_inliers, max_iterations, min_set,
          epsilon, th2, draws, n_draws) -> None:
    q.batch, q.cap, q.kps, q.n, q.matches = batch, cap, kps, n, matches
    q.n_mp, q.mp_pos = n_mp, mp_pos
    q.level_sigma2, q.nlevels = sig.ctypes.data_as(F32P), len(sig)
    q.fx, q.fy, q.cx, q.cy = (float(v) for v in K)
    q.probability, q.min_inliers, q.max_iterations = float(probability), int(min_inliers), int(max_iterations)
    q.min_set, q.epsilon, q.th2, q.draws, q.n_draws = int(min_set), float(epsilon), float(th2), draws, int(n_draws)


class PnPsolver:
    """Owns the solver handle (workspace and per-candidate state) and, unless `matcher` is given,
    the matcher handle whose device and stream it runs on.

    With the candidate's arrays -- PnPsolver(keys, matches, mp_pos, level_sigma2, K) -- it is the
    reference's object: keys is F.mvKeysUn (KEYPOINT_DTYPE), matches vpMapPointMatches as
    MapPoint ids into mp_pos ((n_mp, 3) GetWorldPos(); -1 where the reference skips the slot:
    NULL or isBad()), K = fx fy cx cy.  Without them (PnPsolver(max_batch=B, cap=...,
    max_draws=...)) it serves the batch calls on device tensors."""

    def __init__(self, keys=None, matches=None, mp_pos=None, level_sigma2=None, K=None, draws=None, device: int = 0,
                 matcher=None, max_batch: int = 1, cap: int | None = None, max_draws: int = 600):
        self._h = None
        self._m = None
        self._own = matcher is None
        self._matcher = matcher
        self.last = None
        self._keep = None
        self._cand = None
        if keys is not None:
            k = np.ascontiguousarray(keys, dtype=L.KEYPOINT_DTYPE).reshape(-1)
            m = _i32(matches).reshape(-1)
            if len(m) > len(k):
                raise ValueError("vpMapPointMatches is longer than the frame's keypoints")
            n = len(m)
            self._cand = dict(n=n, keys=k[:n].copy(), matches=m, pos=_f32(mp_pos).reshape(-1, 3),
                              sig=_f32(level_sigma2).reshape(-1), K=_f32(K).reshape(-1)[:4].copy(),
                              draws=None if draws is None else _i32(draws).reshape(-1, 4))
            cap = max(1, n) if cap is None else cap
            if cap < n:
                raise ValueError("cap below the number of slots")
        self.max_batch, self.cap, self.max_draws = int(max_batch), int(1024 if cap is None else cap), 0
        self.max_iterations = 0
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
        self._destroy = lib.orbx_pnp_destroy
        L.track(self)
        self._reserve(max_draws)
        if self._cand is not None:
            self.SetRansacParameters()                                   # cc:127

    def _reserve(self, max_draws: int) -> None:
        if self._h is not None and max_draws <= self.max_draws:
            return
        if self._h is not None:
            self._destroy(self._h)
            self._h = None
        h = C.c_void_p()
        L.check(L.lib().orbx_pnp_create(self._m, self.max_batch, self.cap, int(max_draws), C.byref(h)))
        self._h = h
        self.max_draws = int(max_draws)

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
    def n_correspondences(self) -> int:
        """N: the slots with a valid MapPoint id (cc:96-118)."""
        c = self._cand
        return int(((c["matches"] >= 0) & (c["matches"] < len(c["pos"]))).sum())

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 8, maxIterations: int = 300,
                            minSet: int = 4, epsilon: float = 0.4, th2: float = 5.991, draws=None,
                            n_draws: int | None = None) -> None:
        """cc:141-190 (the defaults of PnPsolver.h).  `draws` (n_draws, 4) i32 replaces the
        constructor's; without either, reference_draws(N, n_draws) with n_draws = 2 *
        maxIterations: the first iterate runs to the cap, later ones beyond it (cc:226)."""
        c = self._cand
        if c is None:
            raise ValueError("no candidate: this solver serves the batch calls")
        if draws is not None:
            c["draws"] = _i32(draws).reshape(-1, 4)
        d = c["draws"]
        if d is None:
            d = reference_draws(self.n_correspondences(), 2 * maxIterations if n_draws is None else n_draws)
        elif n_draws is not None:
            d = d[:n_draws]
        d = np.ascontiguousarray(d)
        self._reserve(len(d))
        n = np.array([c["n"]], np.int32)
        q = L.PnpBatch()
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        _fill(q, batch=1, cap=self.cap, kps=ptr(c["keys"]), n=ptr(n), matches=ptr(c["matches"]), n_mp=len(c["pos"]),
              mp_pos=ptr(c["pos"]), sig=c["sig"], K=c["K"], probability=probability, min_inliers=minInliers,
              max_iterations=maxIterations, min_set=minSet, epsilon=epsilon, th2=th2, draws=ptr(d), n_draws=len(d))
        L.check(L.lib().orbx_pnp_set(self._h, C.byref(q)))
        self.max_iterations = int(maxIterations)
        self.last = None

    def iterate_host(self, n_iterations: int) -> dict:
        """One orbx_pnp_iterate: every output of the call as host arrays."""
        n = self._cand["n"]
        i32 = lambda: np.zeros(1, np.int32)  # noqa: E731
        o = dict(found=i32(), no_more=i32(), n_inliers=i32(), inliers=np.zeros(max(1, n), np.uint8),
                 Tcw=np.zeros(12, np.float32), frame_mp=np.full(max(1, n), -1, np.int32),
                 best_Tcw=np.zeros(12, np.float32), best_inliers=i32(), best_iteration=i32(), refined=i32(),
                 iterations=i32(), n_corr=i32(), min_inliers_used=i32(), max_its_used=i32(), status=i32())
        r = L.PnpResult()
        for k in RESULT_FIELDS:
            setattr(r, k, C.c_void_p(o[k].ctypes.data))
        L.check(L.lib().orbx_pnp_iterate(self._h, int(n_iterations), C.byref(r)))
        o["inliers"] = o["inliers"][:n]
        o["frame_mp"] = o["frame_mp"][:n]
        self.last = o
        return o

    def iterate(self, nIterations: int):
        """cc:200-323: (Tcw (4, 4) f32 or None, bNoMore, vbInliers (n,) bool, nInliers)."""
        o = self.iterate_host(nIterations)
        T = None
        if o["found"][0]:
            T = np.eye(4, dtype=np.float32)
            T[:3] = o["Tcw"].reshape(3, 4)
        return T, bool(o["no_more"][0]), o["inliers"].astype(bool), int(o["n_inliers"][0])

    def find(self):
        """cc:193-197: (Tcw or None, vbInliers, nInliers)."""
        T, _, inl, n = self.iterate(self.max_iterations)
        return T, inl, n

    # ---- B candidates in HBM ----------------------------------------------------------------------
    def set_batch_device(self, d_kps, d_n, d_matches, d_mp_pos, level_sigma2, K, d_draws, probability: float = 0.99,
                         min_inliers: int = 10, max_iterations: int = 300, min_set: int = 4, epsilon: float = 0.5,
                         th2: float = 5.991, stream=None) -> None:
        """orbx_pnp_set_batch_device on device tensors: d_kps (B, cap, 28) u8 or (B, cap, 7) f32 /
        i32 storage of orbx_keypoint, d_n (B,) i32, d_matches (B, cap) i32, d_mp_pos (n_mp, 3)
        f32, d_draws (B, n_draws, 4) i32 (kept alive here until the next set); level_sigma2 and
        K = fx fy cx cy host arrays.  The parameter defaults are Tracking::Relocalization's
        (Tracking.cc:1556).  Asynchronous on `stream` (a torch stream or a raw handle) or the
        matcher's; a null handle -- torch's default stream -- also means the matcher's, which is
        not ordered with torch's work: pass a torch.cuda.Stream to order the two."""
        B, cap = d_matches.shape[0], d_matches.shape[1]
        if d_draws.dim() != 3 or d_draws.shape[0] != B or d_draws.shape[2] != 4:
            raise ValueError("d_draws must be (B, n_draws, 4)")
        if d_kps.numel() * d_kps.element_size() != B * cap * 28:
            raise ValueError("d_kps must hold B x cap orbx_keypoint")
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        q = L.PnpBatch()
        _fill(q, batch=B, cap=cap, kps=ptr(d_kps), n=ptr(d_n), matches=ptr(d_matches), n_mp=int(d_mp_pos.shape[0]),
              mp_pos=ptr(d_mp_pos), sig=_f32(level_sigma2).reshape(-1), K=_f32(K).reshape(-1)[:4],
              probability=probability, min_inliers=min_inliers, max_iterations=max_iterations, min_set=min_set,
              epsilon=epsilon, th2=th2, draws=ptr(d_draws), n_draws=int(d_draws.shape[1]))
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_pnp_set_batch_device(self._h, C.byref(q), s))
        self._keep = (d_kps, d_n, d_matches, d_mp_pos, d_draws)
        self._cand = None
        self.max_iterations = int(max_iterations)

    def iterate_batch_device(self, n_iterations: int, stream=None, **out) -> None:
        """orbx_pnp_iterate_device: keyword arguments name the outputs wanted (RESULT_FIELDS:
        found, no_more, n_inliers, best_inliers, best_iteration, refined, iterations, n_corr,
        min_inliers_used, max_its_used, status (B,) i32; inliers (B, cap) u8; frame_mp (B, cap)
        i32; Tcw, best_Tcw (B, 12) f32), each a device tensor.  Asynchronous on `stream` (or
        the matcher's)."""
        r = L.PnpResult()
        for k, t in out.items():
            if k not in RESULT_FIELDS:
                raise ValueError(f"unknown output {k}")
            setattr(r, k, None if t is None else C.c_void_p(t.data_ptr()))
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_pnp_iterate_device(self._h, int(n_iterations), C.byref(r), s))
