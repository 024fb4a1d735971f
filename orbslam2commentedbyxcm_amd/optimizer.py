"""Optimizer::PoseOptimization on the GPU (include/orbx.h, csrc/orbx_poseopt.hip).

PoseOptimizer mirrors the one g2o call on ORB-SLAM2's per-frame path
(src/Optimizer.cc:299-502): PoseOptimization for one frame on host arrays, and
pose_optimization_batch_device for B frames in HBM with the callers' epilogue
(Tracking.cc:1004-1017).
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L

F32P = C.POINTER(C.c_float)
I32P = C.POINTER(C.c_int32)
U8P = C.POINTER(C.c_uint8)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


class PoseOptimizer:
    """Owns the library handle (workspace and stream) the optimisation runs on, or borrows
    an ORBmatcher's: PoseOptimizer(matcher=m) enqueues on that matcher's stream."""

    def __init__(self, device: int = 0, matcher=None):
        self._h = None
        self._own = matcher is None
        self._matcher = matcher
        if matcher is not None:
            self.device = matcher.device
            self._h = matcher._h
            return
        self.device = int(device)
        h = C.c_void_p()
        L.check(L.lib().orbx_matcher_create(self.device, 0.6, 1, C.byref(h)))
        self._destroy = L.lib().orbx_matcher_destroy  # held: module globals may be gone at exit
        self._h = h
        L.track(self)

    def close(self) -> None:
        """Release the handle (waits for its stream); idempotent.  A borrowed one is left alone."""
        if getattr(self, "_h", None) and self._own:
            self._destroy(self._h)
        self._h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    def last_call_us(self) -> float:
        return float(L.lib().orbx_matcher_last_call_us(self._h))

    def PoseOptimization(self, keys_un, u_right, frame_mp, mp_pos, inv_level_sigma2, fx, fy, cx, cy, bf, Tcw,
                         outlier=None) -> dict:
        """Optimizer::PoseOptimization(pFrame) on host arrays: keys_un (n,) KEYPOINT_DTYPE
        (mvKeysUn), u_right (n,) f32 or None, frame_mp (n,) MapPoint ids (-1 = NULL), mp_pos
        (n_mp, 3) f32, inv_level_sigma2 (mvInvLevelSigma2), Tcw 12 floats (mTcw rows 0..2).
        Returns Tcw (12,) f32, outlier (n,) u8 (mvbOutlier; starts from `outlier` or zeros),
        ninliers (the return value), ninit (nInitialCorrespondences), trace (4, 2) i32."""
        keys = np.ascontiguousarray(keys_un, dtype=L.KEYPOINT_DTYPE)
        n = len(keys)
        mp = np.ascontiguousarray(frame_mp, dtype=np.int32)
        pos = _f32(mp_pos).reshape(-1, 3)
        ur = None if u_right is None else _f32(u_right)
        sig = _f32(inv_level_sigma2)
        tin = _f32(Tcw).reshape(-1)
        if len(mp) != n or (ur is not None and len(ur) != n) or len(tin) != 12:
            raise ValueError("keys_un, u_right and frame_mp must have one length; Tcw 12 entries")
        out = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, dtype=np.uint8, copy=True)
        if len(out) != n:
            raise ValueError("outlier must have one entry per keypoint")
        tout = np.empty(12, np.float32)
        trace = np.zeros((4, 2), np.int32)
        ninit, ninl = C.c_int(0), C.c_int(0)
        L.check(L.lib().orbx_pose_optimization(
            self._h, C.c_void_p(keys.ctypes.data) if n else None, n, None if ur is None else ur.ctypes.data_as(F32P),
            mp.ctypes.data_as(I32P), pos.ctypes.data_as(F32P), len(pos), sig.ctypes.data_as(F32P), len(sig),
            float(fx), float(fy), float(cx), float(cy), float(bf), tin.ctypes.data_as(F32P),
            tout.ctypes.data_as(F32P), out.ctypes.data_as(U8P), C.byref(ninit), trace.ctypes.data_as(I32P),
            C.byref(ninl)))
        return dict(Tcw=tout, outlier=out, ninliers=ninl.value, ninit=ninit.value, trace=trace)

    def pose_optimization_batch_device(self, d_kps, d_n, d_frame_mp, d_mp_pos, inv_level_sigma2, fx, fy, cx, cy, bf,
                                       d_Tcw, d_Tcw_opt, d_outlier, d_ninliers, d_ninit, d_u_right=None,
                                       d_trace=None, discard_outliers: bool = False, d_mp_obs=None,
                                       d_nmatches_map=None, stream=None) -> None:
        """orbx_pose_optimization_batch_device on device tensors: d_kps (B, cap) keypoints
        (any 28-byte layout), d_n (B,) i32, d_frame_mp (B, cap) i32, d_mp_pos (n_mp, 3) f32,
        d_Tcw / d_Tcw_opt (B, 12) f32, d_outlier (B, cap) u8, d_ninliers / d_ninit (B,) i32,
        optional d_u_right (B, cap) f32, d_trace (B, 4, 2) i32, d_mp_obs (n_mp,) i32 and
        d_nmatches_map (B,) i32.  Asynchronous on `stream` (or the handle's)."""
        B, cap = d_frame_mp.shape[0], d_frame_mp.shape[1]
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        sig = _f32(inv_level_sigma2)
        q = L.PoseOptimizationBatch()
        q.batch, q.cap = B, cap
        q.kps, q.n, q.u_right, q.frame_mp = ptr(d_kps), ptr(d_n), ptr(d_u_right), ptr(d_frame_mp)
        q.n_mp, q.mp_pos = int(d_mp_pos.shape[0]), ptr(d_mp_pos)
        q.inv_level_sigma2, q.nlevels = sig.ctypes.data_as(F32P), len(sig)
        q.fx, q.fy, q.cx, q.cy, q.bf = fx, fy, cx, cy, bf
        q.Tcw, q.Tcw_opt, q.outlier = ptr(d_Tcw), ptr(d_Tcw_opt), ptr(d_outlier)
        q.ninliers, q.ninit, q.trace = ptr(d_ninliers), ptr(d_ninit), ptr(d_trace)
        q.discard_outliers = 1 if discard_outliers else 0
        q.mp_obs, q.nmatches_map = ptr(d_mp_obs), ptr(d_nmatches_map)
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_pose_optimization_batch_device(self._h, C.byref(q), s))


class PoseOptStage:
    """The pipelines' PoseOptimization stage: per-buffer outputs and the batch call (with the
    nmatches_map epilogue) on the tracking matcher's handle and stream, after the search and
    its retry.  mvpMapPoints stay as the search left them: `outlier` says which to discard."""

    def __init__(self, matcher, nbuf: int, B: int, cap: int, device, inv_level_sigma2):
        import torch
        self.opt = PoseOptimizer(matcher=matcher)
        self.sig = _f32(inv_level_sigma2)
        i32 = dict(dtype=torch.int32, device=device)
        self.buf = [{"Tcw_opt": torch.zeros((B, 12), dtype=torch.float32, device=device),
                     "outlier": torch.zeros((B, cap), dtype=torch.uint8, device=device),
                     "ninliers": torch.zeros((B,), **i32), "ninit": torch.zeros((B,), **i32),
                     "nmatches_map": torch.zeros((B,), **i32)} for _ in range(nbuf)]

    def run(self, k: int, d_kps, d_n, d_mp, d_mp_pos, d_Tcw, fx, fy, cx, cy, bf=0.0, d_u_right=None, d_mp_obs=None,
            stream=None) -> None:
        """`stream`: the torch stream to enqueue on.  mvbOutlier starts false in every new Frame
        (Frame.cc:58-60 and the other constructors), so the flags are cleared first."""
        import torch
        o = self.buf[k]
        with torch.cuda.stream(stream):
            o["outlier"].zero_()
        self.opt.pose_optimization_batch_device(
            d_kps, d_n, d_mp, d_mp_pos.view(-1, 3), self.sig, fx, fy, cx, cy, bf, d_Tcw, o["Tcw_opt"], o["outlier"],
            o["ninliers"], o["ninit"], d_u_right=d_u_right, d_mp_obs=None if d_mp_obs is None else d_mp_obs.view(-1),
            d_nmatches_map=o["nmatches_map"], stream=stream.cuda_stream)

    def results(self, k: int) -> dict:
        return dict(self.buf[k])
