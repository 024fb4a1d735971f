"""Initializer on the GPU (include/orbx.h, csrc/orbx_initializer.hip).

Initializer mirrors include/Initializer.h (src/Initializer.cc:64-1415): the H / F RANSAC over
the matches of SearchForInitialization and the two-view reconstruction of the chosen model, as
Tracking::MonocularInitialization calls it.  One frame pair on host arrays keeps the
reference's surface (Initialize); initialize_batch_device runs B pairs resident in HBM.

The library owns no random generator: the 8-point sets of every iteration are an input
(`reference_sets` gives the reference's, over the C library's rand()).
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L

F32P = C.POINTER(C.c_float)
I32P = C.POINTER(C.c_int32)

RESULT_FIELDS = L.INITIALIZER_RESULT_FIELDS
# per pair: dtype and trailing shape (kcap stands for the row length)
RESULT_LAYOUT = dict(ok=("i4", ()), model=("i4", ()), n_matches=("i4", ()), SH=("f4", ()), SF=("f4", ()),
                     RH=("f4", ()), best_it_H=("i4", ()), best_it_F=("i4", ()), H21=("f4", (9,)), F21=("f4", (9,)),
                     inliers_H=("u1", ("kcap",)), inliers_F=("u1", ("kcap",)), n_inliers_H=("i4", ()),
                     n_inliers_F=("i4", ()), R21=("f4", (9,)), t21=("f4", (3,)), p3d=("f4", ("kcap", 3)),
                     triangulated=("u1", ("kcap",)), best_good=("i4", ()), second_good=("i4", ()),
                     n_similar=("i4", ()), parallax=("f4", ()), status=("i4", ()))


def reference_sets(n: int, iterations: int) -> np.ndarray:
    """(iterations, 8) i32: mvSets of Initializer.cc:103-123 for n correspondences, from srand(0)."""
    out = np.zeros((max(0, int(iterations)), 8), np.int32)
    L.check(L.lib().orbx_initializer_sets(out.ctypes.data_as(I32P), int(n), len(out)))
    return out


def _keys(a) -> np.ndarray:
    """KEYPOINT_DTYPE records from records or from an (n, 2) array of x, y."""
    a = np.asarray(a)
    if a.dtype == L.KEYPOINT_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    xy = np.asarray(a, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), L.KEYPOINT_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return k


class Initializer:
    """Owns the solver handle (its workspace) and, unless `matcher` is given, the matcher handle
    whose device and stream it runs on.  Initializer(max_batch, kcap, max_iterations=200,
    sigma=1.0) is the reference's Initializer(ReferenceFrame, sigma, iterations) without the
    frame: the reference frame's keypoints are an argument of every call."""

    def __init__(self, max_batch: int = 1, kcap: int = 1024, max_iterations: int = 200, sigma: float = 1.0,
                 device: int = 0, matcher=None):
        self._h = None
        self._m = None
        self._own = matcher is None
        self._matcher = matcher
        self._keep = None
        self.max_batch, self.kcap, self.max_iterations, self.sigma = int(max_batch), int(kcap), int(max_iterations), \
            float(sigma)
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
        self._destroy = lib.orbx_initializer_destroy
        L.track(self)
        h = C.c_void_p()
        L.check(lib.orbx_initializer_create(self._m, self.max_batch, self.kcap, self.max_iterations, C.byref(h)))
        self._h = h

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
        """Wall time of the newest host Initialize inside the library."""
        return float(L.lib().orbx_matcher_last_call_us(self._m))

    # ---- the reference's surface, one frame pair on host arrays -----------------------------------
    def initialize_host(self, keys1, keys2, matches12, K, sets=None, max_iterations: int | None = None) -> dict:
        """One orbx_initializer_initialize: every output of the call as host arrays (the
        per-keypoint ones n1 long).  keys1 / keys2: KEYPOINT_DTYPE records or (n, 2) x, y;
        matches12 (n1,) i32; K fx fy cx cy; sets (max_iterations, 8) i32 or None: reference_sets."""
        k1, k2 = _keys(keys1), _keys(keys2)
        m = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        if len(m) != len(k1):
            raise ValueError("one vMatches12 entry per keypoint of the reference frame")
        n1, n2 = len(k1), len(k2)
        if max(n1, n2) > self.kcap:
            raise ValueError("more keypoints than kcap")
        its = self.max_iterations if max_iterations is None else int(max_iterations)
        if sets is None:
            sets = reference_sets(int(((m >= 0) & (m < n2)).sum()), its)
        sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
        if len(sets) < its:
            raise ValueError("fewer sets than max_iterations")
        sets = np.ascontiguousarray(sets[:its])
        kk = np.ascontiguousarray(K, np.float32).reshape(-1)[:4].copy()
        nn = np.array([n1, n2], np.int32)
        kcap = max(1, n1, n2)
        q = L.InitializerBatch()
        q.batch, q.kcap = 1, kcap
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        q.n1, q.n2, q.keys1, q.keys2, q.matches12 = ptr(nn), ptr(nn[1:]), ptr(k1), ptr(k2), ptr(m)
        q.K, q.sigma, q.max_iterations, q.sets = kk.ctypes.data_as(F32P), self.sigma, its, ptr(sets)
        o = {}
        for k, (dt, shape) in RESULT_LAYOUT.items():
            o[k] = np.zeros(tuple(max(1, n1) if d == "kcap" else d for d in shape) or (1,), dt)
        r = L.InitializerResult()
        for k in RESULT_FIELDS:
            setattr(r, k, C.c_void_p(o[k].ctypes.data))
        L.check(L.lib().orbx_initializer_initialize(self._h, C.byref(q), C.byref(r)))
        for k, (_, shape) in RESULT_LAYOUT.items():
            if shape and shape[0] == "kcap":
                o[k] = o[k][:n1]
        return o

    def Initialize(self, keys1, keys2, matches12, K, sets=None):
        """cc:64-165: (ok, R21 (3, 3) f32, t21 (3,) f32, vP3D (n1, 3) f32, vbTriangulated (n1,) bool);
        R21 and t21 are None (the empty Mat) when ok is False."""
        o = self.initialize_host(keys1, keys2, matches12, K, sets)
        ok = bool(o["ok"][0])
        return (ok, o["R21"].reshape(3, 3).copy() if ok else None, o["t21"].copy() if ok else None, o["p3d"],
                o["triangulated"].astype(bool))

    # ---- B frame pairs in HBM ---------------------------------------------------------------------
    def initialize_batch_device(self, d_n1, d_n2, d_keys1, d_keys2, d_matches12, K, d_sets, stream=None,
                                **out) -> None:
        """orbx_initializer_initialize_device on device tensors: d_n1 / d_n2 (B,) i32, d_keys1 /
        d_keys2 (B, kcap, 28) u8 (orbx_keypoint records), d_matches12 (B, kcap) i32, d_sets
        (B, max_iterations, 8) i32; K a host array.  Keyword arguments name the outputs wanted
        (RESULT_FIELDS, shapes per pair in RESULT_LAYOUT), each a device tensor.  Asynchronous on
        `stream` (a torch stream or a raw handle) or the matcher's; a null handle -- torch's
        default stream -- also means the matcher's, which is not ordered with torch's work."""
        B, kcap = d_matches12.shape[0], d_matches12.shape[1]
        if d_sets.dim() != 3 or d_sets.shape[0] != B or d_sets.shape[2] != 8:
            raise ValueError("d_sets must be (B, max_iterations, 8)")
        if d_keys1.numel() * d_keys1.element_size() != B * kcap * 28 or \
                d_keys2.numel() * d_keys2.element_size() != B * kcap * 28:
            raise ValueError("d_keys1 / d_keys2 must hold (B, kcap) orbx_keypoint records")
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        kk = np.ascontiguousarray(K, np.float32).reshape(-1)[:4].copy()
        q = L.InitializerBatch()
        q.batch, q.kcap = B, kcap
        q.n1, q.n2, q.keys1, q.keys2, q.matches12 = ptr(d_n1), ptr(d_n2), ptr(d_keys1), ptr(d_keys2), ptr(d_matches12)
        q.K, q.sigma, q.max_iterations, q.sets = kk.ctypes.data_as(F32P), self.sigma, int(d_sets.shape[1]), ptr(d_sets)
        r = L.InitializerResult()
        for k, t in out.items():
            if k not in RESULT_FIELDS:
                raise ValueError(f"unknown output {k}")
            setattr(r, k, None if t is None else C.c_void_p(t.data_ptr()))
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_initializer_initialize_device(self._h, C.byref(q), C.byref(r), s))
        self._keep = (d_n1, d_n2, d_keys1, d_keys2, d_matches12, d_sets, out)
