"""Optimizer::PoseOptimization, Optimizer::OptimizeSim3, Optimizer::LocalBundleAdjustment,
Optimizer::BundleAdjustment and Optimizer::OptimizeEssentialGraph on the GPU (include/orbx.h,
csrc/orbx_poseopt.hip, csrc/orbx_optsim3.hip, csrc/orbx_localba.hip, csrc/orbx_globalba.hip,
csrc/orbx_essgraph.hip).

PoseOptimizer mirrors the one g2o call on ORB-SLAM2's per-frame path
(src/Optimizer.cc:299-502): PoseOptimization for one frame on host arrays, and
pose_optimization_batch_device for B frames in HBM with the callers' epilogue
(Tracking.cc:1004-1017).  Sim3Optimizer mirrors the one of LoopClosing::ComputeSim3
(src/Optimizer.cc:1173-1358): OptimizeSim3 for one loop candidate on host arrays, and
optimize_sim3_batch_device for B candidates in HBM.  LocalBundleAdjuster mirrors the one of
LocalMapping::Run (src/Optimizer.cc:586-853): LocalBundleAdjustment for one local map on host
arrays, and local_ba_batch_device for B local maps in HBM.  GlobalBundleAdjuster mirrors the
one of Tracking::CreateInitialMapMonocular and LoopClosing::RunGlobalBundleAdjustment
(src/Optimizer.cc:41-281): BundleAdjustment for one map on host arrays, and
global_ba_batch_device for B maps in HBM.  EssentialGraphOptimizer mirrors the
one of LoopClosing::CorrectLoop (src/Optimizer.cc:873-1150): OptimizeEssentialGraph for one map
on host arrays, and essential_graph_batch_device for B maps in HBM; essential_graph_edges
writes the graph's edges in the reference's order on the host.
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


class Sim3Optimizer:
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:1173-1358) on the GPU (csrc/orbx_optsim3.hip):
    OptimizeSim3 for one loop candidate on host arrays and optimize_sim3_batch_device for B
    candidates in HBM, fed by Sim3Solver's best_R / best_t / best_s and SearchBySim3's
    matches.  Owns its library handle or borrows an ORBmatcher's, as PoseOptimizer does."""

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

    def OptimizeSim3(self, keys_un1, mp1, matches12, idx2, keys_un2, mp_pos, Tcw1, Tcw2, inv_level_sigma2_1,
                     inv_level_sigma2_2, K1, K2, R12, t12, s12, th2, fix_scale) -> dict:
        """Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) on host arrays:
        keys_un1 (n1,) / keys_un2 (n2,) KEYPOINT_DTYPE (mvKeysUn), mp1 (n1,) pKF1's MapPoint ids,
        matches12 (n1,) vpMatches1 as MapPoint ids, idx2 (n1,) GetIndexInKeyFrame(pKF2), mp_pos
        (n_mp, 3) f32, Tcw1 / Tcw2 12 floats, K1 / K2 = fx fy cx cy, S12 as R12 (9) t12 (3) s12.
        Returns R12, t12, s12 (f32), matches12 (rejected entries -1), ninliers (the return
        value), ncorr, nbad and trace (2, 2) i32."""
        k1 = np.ascontiguousarray(keys_un1, dtype=L.KEYPOINT_DTYPE)
        k2 = np.ascontiguousarray(keys_un2, dtype=L.KEYPOINT_DTYPE)
        n1, n2 = len(k1), len(k2)
        m1 = np.ascontiguousarray(mp1, dtype=np.int32)
        m12 = np.array(matches12, dtype=np.int32, copy=True)
        i2 = np.ascontiguousarray(idx2, dtype=np.int32)
        if not (len(m1) == len(m12) == len(i2) == n1):
            raise ValueError("keys_un1, mp1, matches12 and idx2 must have one length")

        def room(a, dtype):  # the call takes no null array: an empty one gets one spare element
            return a if len(a) else np.zeros(1, dtype)

        k1, k2 = room(k1, L.KEYPOINT_DTYPE), room(k2, L.KEYPOINT_DTYPE)
        m1, m12, i2 = room(m1, np.int32), room(m12, np.int32), room(i2, np.int32)
        pos = _f32(mp_pos).reshape(-1, 3)
        t1, t2 = _f32(Tcw1).reshape(-1), _f32(Tcw2).reshape(-1)
        sig1, sig2 = _f32(inv_level_sigma2_1), _f32(inv_level_sigma2_2)
        kk1, kk2 = _f32(K1).reshape(-1), _f32(K2).reshape(-1)
        R, t, s = _f32(R12).reshape(-1), _f32(t12).reshape(-1), _f32([s12]).reshape(-1)
        if len(t1) != 12 or len(t2) != 12 or len(kk1) != 4 or len(kk2) != 4 or len(R) != 9 or len(t) != 3:
            raise ValueError("Tcw 12, K 4, R12 9 and t12 3 entries")
        if len(sig1) != len(sig2):
            raise ValueError("both keyframes need one number of levels")
        cn1, cn2 = np.array([n1], np.int32), np.array([n2], np.int32)
        Ro, to, so = np.empty(9, np.float32), np.empty(3, np.float32), np.empty(1, np.float32)
        cnt = np.zeros(3, np.int32)
        trace = np.zeros((2, 2), np.int32)
        vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        q = L.OptimizeSim3Batch()
        q.batch, q.cap1, q.cap2 = 1, max(n1, 1), max(n2, 1)
        q.n1, q.kps1, q.mp1, q.matches12, q.idx2 = vp(cn1), vp(k1), vp(m1), vp(m12), vp(i2)
        q.n2, q.kps2 = vp(cn2), vp(k2)
        q.n_mp, q.mp_pos = len(pos), vp(pos) if len(pos) else None
        q.Tcw1, q.Tcw2 = vp(t1), vp(t2)
        q.inv_level_sigma2_1, q.inv_level_sigma2_2, q.nlevels = sig1.ctypes.data_as(F32P), sig2.ctypes.data_as(F32P), len(sig1)
        q.K1, q.K2 = kk1.ctypes.data_as(F32P), kk2.ctypes.data_as(F32P)
        q.R12, q.t12, q.s12 = vp(R), vp(t), vp(s)
        q.th2, q.fix_scale = float(th2), 1 if fix_scale else 0
        q.R12_opt, q.t12_opt, q.s12_opt = vp(Ro), vp(to), vp(so)
        q.ninliers, q.ncorr, q.nbad = vp(cnt[0:1]), vp(cnt[1:2]), vp(cnt[2:3])
        q.trace = vp(trace)
        L.check(L.lib().orbx_optimize_sim3(self._h, C.byref(q)))
        return dict(R12=Ro, t12=to, s12=so[0], matches12=m12[:n1], ninliers=int(cnt[0]), ncorr=int(cnt[1]),
                    nbad=int(cnt[2]), trace=trace)

    def optimize_sim3_batch_device(self, d_kps1, d_n1, d_mp1, d_matches12, d_idx2, d_kps2, d_n2, d_mp_pos, d_Tcw1,
                                   d_Tcw2, inv_level_sigma2_1, inv_level_sigma2_2, K1, K2, d_R12, d_t12, d_s12, th2,
                                   fix_scale, d_R12_opt, d_t12_opt, d_s12_opt, d_ninliers=None, d_ncorr=None,
                                   d_nbad=None, d_trace=None, cap2=None, stream=None) -> None:
        """orbx_optimize_sim3_batch_device on device tensors: d_kps1 (B, cap1) / d_kps2 (B, cap2)
        keypoints (any 28-byte layout), d_n1 / d_n2 (B,) i32, d_mp1 / d_matches12 (in/out) /
        d_idx2 (B, cap1) i32, d_mp_pos (n_mp, 3) f32, d_Tcw1 / d_Tcw2 (B, 12), d_R12 (B, 9),
        d_t12 (B, 3), d_s12 (B,) f32 -- Sim3Solver's best_R / best_t / best_s as they are --
        and the outputs of the same shapes; optional d_ninliers / d_ncorr / d_nbad (B,) and
        d_trace (B, 2, 2) i32.  cap2: keypoints per row of d_kps2 when its shape does not say (a
        byte tensor is taken as 28 bytes per keypoint).  Asynchronous on `stream` (or the handle's)."""
        B, cap1 = d_mp1.shape[0], d_mp1.shape[1]
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        sig1, sig2 = _f32(inv_level_sigma2_1), _f32(inv_level_sigma2_2)
        if len(sig1) != len(sig2):
            raise ValueError("both keyframes need one number of levels")
        kk1, kk2 = _f32(K1).reshape(-1), _f32(K2).reshape(-1)
        if len(kk1) != 4 or len(kk2) != 4:
            raise ValueError("K1 and K2 are fx fy cx cy")
        q = L.OptimizeSim3Batch()
        q.batch, q.cap1, q.cap2 = B, cap1, self._cap2(d_kps2) if cap2 is None else int(cap2)
        q.n1, q.kps1, q.mp1, q.matches12, q.idx2 = ptr(d_n1), ptr(d_kps1), ptr(d_mp1), ptr(d_matches12), ptr(d_idx2)
        q.n2, q.kps2 = ptr(d_n2), ptr(d_kps2)
        q.n_mp, q.mp_pos = int(d_mp_pos.shape[0]), ptr(d_mp_pos)
        q.Tcw1, q.Tcw2 = ptr(d_Tcw1), ptr(d_Tcw2)
        q.inv_level_sigma2_1, q.inv_level_sigma2_2, q.nlevels = sig1.ctypes.data_as(F32P), sig2.ctypes.data_as(F32P), len(sig1)
        q.K1, q.K2 = kk1.ctypes.data_as(F32P), kk2.ctypes.data_as(F32P)
        q.R12, q.t12, q.s12 = ptr(d_R12), ptr(d_t12), ptr(d_s12)
        q.th2, q.fix_scale = float(th2), 1 if fix_scale else 0
        q.R12_opt, q.t12_opt, q.s12_opt = ptr(d_R12_opt), ptr(d_t12_opt), ptr(d_s12_opt)
        q.ninliers, q.ncorr, q.nbad, q.trace = ptr(d_ninliers), ptr(d_ncorr), ptr(d_nbad), ptr(d_trace)
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_optimize_sim3_batch_device(self._h, C.byref(q), s))

    @staticmethod
    def _cap2(d_kps2) -> int:
        """Keypoints per row of a (B, cap2) structured or (B, cap2 * 28) byte tensor."""
        cols = int(d_kps2.shape[1])
        return cols // 28 if d_kps2.element_size() == 1 else cols


class LocalBundleAdjuster(PoseOptimizer):
    """Optimizer::LocalBundleAdjustment (src/Optimizer.cc:586-853) on the GPU
    (csrc/orbx_localba.hip): LocalBundleAdjustment for one local map on host arrays and
    local_ba_batch_device for B local maps in HBM.  The covisibility walk that chooses the
    keyframes and points is the caller's, or assemble_batch_device's on a CovisibilityGraph
    (csrc/orbx_covis.hip), with apply_batch_device for the way back; the stop flag is not supported.  The handle,
    close() and last_call_us() are PoseOptimizer's."""

    def LocalBundleAdjustment(self, kf_Tcw, kf_fixed, kf_slot, pt_pos, obs_off, obs_kf, obs_kp, keys_un, u_right,
                              inv_level_sigma2, fx, fy, cx, cy, bf, max_free_kf: int = 0) -> dict:
        """One local map on host arrays: kf_Tcw (K, 12) f32, kf_fixed (K,) (lFixedCameras and
        mnId == 0), kf_slot (K,) rows of keys_un / u_right, pt_pos (P, 3) f32, obs_off (P + 1,),
        obs_kf / obs_kp (n_obs,) (keyframe within the K rows, keypoint within its row),
        keys_un (n_slots, cap) KEYPOINT_DTYPE, u_right (n_slots, cap) f32 or None.
        Returns Tcw (K, 12) and pos (P, 3) f32, erase and level1 (n_obs,) u8, n_erase,
        trace (2, 2) i32 and status."""
        T = _f32(kf_Tcw).reshape(-1, 12)
        fixed = np.ascontiguousarray(kf_fixed, dtype=np.uint8)
        slot = np.ascontiguousarray(kf_slot, dtype=np.int32)
        pos = _f32(pt_pos).reshape(-1, 3)
        off = np.ascontiguousarray(obs_off, dtype=np.int32)
        okf = np.ascontiguousarray(obs_kf, dtype=np.int32)
        okp = np.ascontiguousarray(obs_kp, dtype=np.int32)
        keys = np.ascontiguousarray(keys_un, dtype=L.KEYPOINT_DTYPE)
        if keys.ndim != 2:
            raise ValueError("keys_un must be (n_slots, cap)")
        ur = None if u_right is None else _f32(u_right)
        K, P, no = len(T), len(pos), len(okf)
        if len(fixed) != K or len(slot) != K or len(off) != P + 1 or len(okp) != no or \
                (ur is not None and ur.shape != keys.shape):
            raise ValueError("table sizes differ")
        sig = _f32(inv_level_sigma2)
        kf_off = np.array([0, K], np.int32)
        pt_off = np.array([0, P], np.int32)
        out = dict(Tcw=np.zeros((K, 12), np.float32), pos=np.zeros((P, 3), np.float32), erase=np.zeros(no, np.uint8),
                   level1=np.zeros(no, np.uint8), trace=np.zeros((2, 2), np.int32))
        n_erase, status = np.zeros(1, np.int32), np.zeros(1, np.int32)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        q = L.LocalBaBatch()
        q.batch = 1
        q.kf_off, q.n_kf, q.kf_Tcw, q.kf_fixed, q.kf_slot = ptr(kf_off), K, ptr(T), ptr(fixed), ptr(slot)
        q.pt_off, q.n_pt, q.pt_pos = ptr(pt_off), P, ptr(pos)
        q.obs_off, q.n_obs, q.obs_kf, q.obs_kp = ptr(off), no, ptr(okf), ptr(okp)
        q.n_slots, q.cap, q.kps, q.u_right = keys.shape[0], keys.shape[1], ptr(keys), ptr(ur)
        q.inv_level_sigma2, q.nlevels = sig.ctypes.data_as(F32P), len(sig)
        q.fx, q.fy, q.cx, q.cy, q.bf = fx, fy, cx, cy, bf
        q.max_free_kf = int(max_free_kf)
        q.kf_Tcw_opt, q.pt_pos_opt, q.erase, q.level1 = ptr(out["Tcw"]), ptr(out["pos"]), ptr(out["erase"]), ptr(out["level1"])
        q.n_erase, q.trace, q.status = ptr(n_erase), ptr(out["trace"]), ptr(status)
        L.check(L.lib().orbx_local_bundle_adjustment(self._h, C.byref(q)))
        out["n_erase"], out["status"] = int(n_erase[0]), int(status[0])
        return out

    def local_ba_batch_device(self, d_kf_off, d_kf_Tcw, d_kf_fixed, d_kf_slot, d_pt_off, d_pt_pos, d_obs_off, d_obs_kf,
                              d_obs_kp, d_kps, d_u_right, inv_level_sigma2, fx, fy, cx, cy, bf, d_kf_Tcw_opt,
                              d_pt_pos_opt, d_erase, d_n_erase, d_status, d_level1=None, d_trace=None,
                              max_free_kf: int = 0, stream=None) -> None:
        """orbx_local_bundle_adjustment_batch_device on device tensors: d_kf_off / d_pt_off
        (B + 1,) i32, d_kf_Tcw / d_kf_Tcw_opt (n_kf, 12) f32, d_kf_fixed (n_kf,) u8, d_kf_slot
        (n_kf,) i32, d_pt_pos / d_pt_pos_opt (n_pt, 3) f32, d_obs_off (n_pt + 1,) i32, d_obs_kf /
        d_obs_kp (n_obs,) i32, d_kps (n_slots, cap) keypoints (any 28-byte layout), d_u_right
        (n_slots, cap) f32 or None, d_erase / d_level1 (n_obs,) u8, d_n_erase / d_status (B,) i32,
        d_trace (B, 2, 2) i32.  Asynchronous on `stream` (or the handle's)."""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        sig = _f32(inv_level_sigma2)
        q = L.LocalBaBatch()
        q.batch = int(d_kf_off.shape[0]) - 1
        q.kf_off, q.n_kf, q.kf_Tcw = ptr(d_kf_off), int(d_kf_Tcw.shape[0]), ptr(d_kf_Tcw)
        q.kf_fixed, q.kf_slot = ptr(d_kf_fixed), ptr(d_kf_slot)
        q.pt_off, q.n_pt, q.pt_pos = ptr(d_pt_off), int(d_pt_pos.shape[0]), ptr(d_pt_pos)
        q.obs_off, q.n_obs, q.obs_kf, q.obs_kp = ptr(d_obs_off), int(d_obs_kf.shape[0]), ptr(d_obs_kf), ptr(d_obs_kp)
        q.n_slots, q.cap, q.kps, q.u_right = int(d_kps.shape[0]), int(d_kps.shape[1]), ptr(d_kps), ptr(d_u_right)
        q.inv_level_sigma2, q.nlevels = sig.ctypes.data_as(F32P), len(sig)
        q.fx, q.fy, q.cx, q.cy, q.bf = fx, fy, cx, cy, bf
        q.max_free_kf = int(max_free_kf)
        q.kf_Tcw_opt, q.pt_pos_opt, q.erase, q.level1 = ptr(d_kf_Tcw_opt), ptr(d_pt_pos_opt), ptr(d_erase), ptr(d_level1)
        q.n_erase, q.trace, q.status = ptr(d_n_erase), ptr(d_trace), ptr(d_status)
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_local_bundle_adjustment_batch_device(self._h, C.byref(q), s))

    ASSEMBLY_TABLES = (("kf_off", "B1", "int32"), ("kf_Tcw", "K12", "float32"), ("kf_fixed", "K", "uint8"),
                       ("kf_slot", "K", "int32"), ("kf_id", "K", "int32"), ("pt_off", "B1", "int32"),
                       ("pt_pos", "P3", "float32"), ("pt_id", "P", "int32"), ("obs_off", "P1", "int32"),
                       ("obs_kf", "O", "int32"), ("obs_kp", "O", "int32"), ("counts", "B3", "int32"),
                       ("status", "B", "int32"))

    def assemble_batch_device(self, graph, cur_kf, d_kf_pose, d_mp_pos, max_kf_rows: int, max_pt_rows: int,
                              max_obs: int, tables: dict | None = None, stream=None) -> dict:
        """orbx_local_ba_assemble_device: the covisibility walk of Optimizer.cc:526-583 and the
        edge walk of cc:656-760 for the current keyframes cur_kf (host ints) on `graph` (a
        CovisibilityGraph, refreshed), into the tables of local_ba_batch_device plus kf_id, pt_id,
        counts (B, 3) and status (B,).  d_kf_pose (K, 12) / d_mp_pos (n, 3) f32 device tensors by
        id; the capacities are for the whole batch.  Returns the tables (device tensors; those
        passed in `tables` are reused).  Nothing is read back.  Asynchronous."""
        import torch
        cur = np.ascontiguousarray(np.atleast_1d(cur_kf), dtype=np.int32)
        B, K, P, O = len(cur), int(max_kf_rows), int(max_pt_rows), int(max_obs)
        shapes = {"B": (B,), "B1": (B + 1,), "B3": (B, 3), "K": (K,), "K12": (K, 12), "P": (P,), "P1": (P + 1,),
                  "P3": (P, 3), "O": (O,)}
        t = dict(tables or {})
        for name, shape, dtype in self.ASSEMBLY_TABLES:
            if name not in t:
                t[name] = torch.zeros(shapes[shape], dtype=getattr(torch, dtype), device=d_kf_pose.device)
            elif tuple(t[name].shape) != shapes[shape]:
                raise ValueError(f"{name}: shape {tuple(t[name].shape)}, expected {shapes[shape]}")
        a = L.LocalBaAssembly()
        a.batch, a.cur_kf = B, L.i32ptr(cur if B else np.zeros(1, np.int32))
        a.kf_pose, a.mp_pos = d_kf_pose.data_ptr(), d_mp_pos.data_ptr()
        a.max_kf_rows, a.max_pt_rows, a.max_obs = K, P, O
        for name, _, _ in self.ASSEMBLY_TABLES:
            setattr(a, name, t[name].data_ptr())
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_local_ba_assemble_device(graph._h, C.byref(a), s))
        return t

    def local_ba_assembled_device(self, tables: dict, d_kps, d_u_right, inv_level_sigma2, fx, fy, cx, cy, bf,
                                  out: dict | None = None, max_free_kf: int = 0, stream=None) -> dict:
        """local_ba_batch_device on the tables of assemble_batch_device (the capacities stand in
        for the sizes).  Returns kf_Tcw_opt, pt_pos_opt, erase, level1, n_erase, trace, status
        (device tensors; those passed in `out` are reused)."""
        import torch
        B = int(tables["kf_off"].shape[0]) - 1
        dev = tables["kf_off"].device
        o = dict(out or {})
        for name, like, dtype in (("kf_Tcw_opt", tables["kf_Tcw"].shape, torch.float32),
                                  ("pt_pos_opt", tables["pt_pos"].shape, torch.float32),
                                  ("erase", tables["obs_kf"].shape, torch.uint8),
                                  ("level1", tables["obs_kf"].shape, torch.uint8), ("n_erase", (B,), torch.int32),
                                  ("trace", (B, 2, 2), torch.int32), ("status", (B,), torch.int32)):
            if name not in o:
                o[name] = torch.zeros(tuple(like), dtype=dtype, device=dev)
        self.local_ba_batch_device(tables["kf_off"], tables["kf_Tcw"], tables["kf_fixed"], tables["kf_slot"],
                                   tables["pt_off"], tables["pt_pos"], tables["obs_off"], tables["obs_kf"],
                                   tables["obs_kp"], d_kps, d_u_right, inv_level_sigma2, fx, fy, cx, cy, bf,
                                   o["kf_Tcw_opt"], o["pt_pos_opt"], o["erase"], o["n_erase"], o["status"],
                                   d_level1=o["level1"], d_trace=o["trace"], max_free_kf=max_free_kf, stream=stream)
        return o

    def apply_batch_device(self, graph, tables: dict, d_kf_Tcw_opt, d_pt_pos_opt, d_erase, d_kf_pose, d_mp_pos,
                           d_kf_mp=None, stream=None) -> None:
        """orbx_local_ba_apply_device, the index part of Optimizer.cc:828-853: the optimised
        poses of the keyframes that are not fixed to d_kf_pose, the positions to d_mp_pos, and
        d_kf_mp[keyframe][keypoint] = -1 for every erase[o].  Asynchronous."""
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        a = L.LocalBaApply()
        a.batch = int(tables["kf_off"].shape[0]) - 1
        a.max_kf_rows, a.max_pt_rows = int(tables["kf_id"].shape[0]), int(tables["pt_id"].shape[0])
        for name in ("kf_off", "kf_id", "kf_fixed", "pt_off", "pt_id", "obs_off", "obs_kf", "obs_kp"):
            setattr(a, name, tables[name].data_ptr())
        a.kf_Tcw_opt, a.pt_pos_opt, a.erase = ptr(d_kf_Tcw_opt), ptr(d_pt_pos_opt), ptr(d_erase)
        a.n_keyframes, a.n_mappoints = int(d_kf_pose.shape[0]), int(d_mp_pos.shape[0])
        a.cap = 0 if d_kf_mp is None else int(d_kf_mp.shape[1])
        a.kf_pose, a.mp_pos, a.kf_mp = ptr(d_kf_pose), ptr(d_mp_pos), ptr(d_kf_mp)
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_local_ba_apply_device(graph._h, C.byref(a), s))


def global_ba_envelope(kf_fixed, obs_off, obs_kf) -> int:
    """orbx_global_ba_envelope: the 6 x 6 blocks of one problem's envelope (max_env_blocks)."""
    fixed = np.ascontiguousarray(kf_fixed, dtype=np.uint8)
    off = np.ascontiguousarray(obs_off, dtype=np.int32)
    okf = np.ascontiguousarray(obs_kf, dtype=np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None  # noqa: E731
    n = C.c_int64(0)
    L.check(L.lib().orbx_global_ba_envelope(len(fixed), ptr(fixed), max(len(off) - 1, 0), ptr(off), ptr(okf), len(okf),
                                            C.byref(n)))
    return int(n.value)


class GlobalBundleAdjuster(PoseOptimizer):
    """Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:41-281) on the GPU
    (csrc/orbx_globalba.hip): BundleAdjustment for one map on host arrays and
    global_ba_batch_device for B maps in HBM.  Which keyframes and points are good, where the
    results go (SetPose or mTcwGBA) and the propagation after a loop's GBA stay with the caller;
    the stop flag is not supported.  The handle, close() and last_call_us() are PoseOptimizer's."""

    global_ba_envelope = staticmethod(global_ba_envelope)

    def BundleAdjustment(self, kf_Tcw, kf_fixed, kf_slot, pt_pos, obs_off, obs_kf, obs_kp, keys_un, u_right,
                         inv_level_sigma2, fx, fy, cx, cy, bf, iterations: int = 5, robust: bool = True,
                         max_env_blocks: int | None = None, dense: bool = False) -> dict:
        """One map on host arrays, the tables of LocalBundleAdjuster.LocalBundleAdjustment;
        kf_fixed: mnId == 0.  iterations / robust: nIterations (the reference's default 5;
        0: 10) / bRobust.  max_env_blocks None: what the problem needs.  Returns Tcw (K, 12)
        and pos (P, 3) f32, pt_included (P,) u8, trace (2,) i32, chi2 (2,) f64 and status."""
        T = _f32(kf_Tcw).reshape(-1, 12)
        fixed = np.ascontiguousarray(kf_fixed, dtype=np.uint8)
        slot = np.ascontiguousarray(kf_slot, dtype=np.int32)
        pos = _f32(pt_pos).reshape(-1, 3)
        off = np.ascontiguousarray(obs_off, dtype=np.int32)
        okf = np.ascontiguousarray(obs_kf, dtype=np.int32)
        okp = np.ascontiguousarray(obs_kp, dtype=np.int32)
        keys = np.ascontiguousarray(keys_un, dtype=L.KEYPOINT_DTYPE)
        if keys.ndim != 2:
            raise ValueError("keys_un must be (n_slots, cap)")
        ur = None if u_right is None else _f32(u_right)
        K, P, no = len(T), len(pos), len(okf)
        if len(fixed) != K or len(slot) != K or len(off) != P + 1 or len(okp) != no or \
                (ur is not None and ur.shape != keys.shape):
            raise ValueError("table sizes differ")
        if max_env_blocks is None:
            max_env_blocks = K * (K + 1) // 2 if dense else global_ba_envelope(fixed, off, okf)
        sig = _f32(inv_level_sigma2)
        kf_off = np.array([0, K], np.int32)
        pt_off = np.array([0, P], np.int32)
        out = dict(Tcw=np.zeros((K, 12), np.float32), pos=np.zeros((P, 3), np.float32),
                   pt_included=np.zeros(P, np.uint8), trace=np.zeros(2, np.int32), chi2=np.zeros(2))
        status = np.zeros(1, np.int32)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        q = L.GlobalBaBatch()
        q.batch = 1
        q.kf_off, q.n_kf, q.kf_Tcw, q.kf_fixed, q.kf_slot = ptr(kf_off), K, ptr(T), ptr(fixed), ptr(slot)
        q.pt_off, q.n_pt, q.pt_pos = ptr(pt_off), P, ptr(pos)
        q.obs_off, q.n_obs, q.obs_kf, q.obs_kp = ptr(off), no, ptr(okf), ptr(okp)
        q.n_slots, q.cap, q.kps, q.u_right = keys.shape[0], keys.shape[1], ptr(keys), ptr(ur)
        q.inv_level_sigma2, q.nlevels = sig.ctypes.data_as(F32P), len(sig)
        q.fx, q.fy, q.cx, q.cy, q.bf = fx, fy, cx, cy, bf
        q.iterations, q.robust, q.max_env_blocks, q.dense = int(iterations), int(bool(robust)), int(max_env_blocks), int(dense)
        q.kf_Tcw_opt, q.pt_pos_opt, q.pt_included = ptr(out["Tcw"]), ptr(out["pos"]), ptr(out["pt_included"])
        q.trace, q.chi2, q.status = ptr(out["trace"]), ptr(out["chi2"]), ptr(status)
        L.check(L.lib().orbx_global_bundle_adjustment(self._h, C.byref(q)))
        out["status"] = int(status[0])
        return out

    def global_ba_batch_device(self, d_kf_off, d_kf_Tcw, d_kf_fixed, d_kf_slot, d_pt_off, d_pt_pos, d_obs_off, d_obs_kf,
                               d_obs_kp, d_kps, d_u_right, inv_level_sigma2, fx, fy, cx, cy, bf, iterations: int,
                               robust: bool, max_env_blocks: int, d_kf_Tcw_opt, d_pt_pos_opt, d_pt_included, d_status,
                               d_trace=None, d_chi2=None, dense: bool = False, stream=None) -> None:
        """orbx_global_bundle_adjustment_batch_device on device tensors: the tables of
        local_ba_batch_device, d_pt_included (n_pt,) u8, d_status (B,) i32, d_trace (B, 2) i32,
        d_chi2 (B, 2) f64.  Asynchronous on `stream` (or the handle's)."""
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        sig = _f32(inv_level_sigma2)
        q = L.GlobalBaBatch()
        q.batch = int(d_kf_off.shape[0]) - 1
        q.kf_off, q.n_kf, q.kf_Tcw = ptr(d_kf_off), int(d_kf_Tcw.shape[0]), ptr(d_kf_Tcw)
        q.kf_fixed, q.kf_slot = ptr(d_kf_fixed), ptr(d_kf_slot)
        q.pt_off, q.n_pt, q.pt_pos = ptr(d_pt_off), int(d_pt_pos.shape[0]), ptr(d_pt_pos)
        q.obs_off, q.n_obs, q.obs_kf, q.obs_kp = ptr(d_obs_off), int(d_obs_kf.shape[0]), ptr(d_obs_kf), ptr(d_obs_kp)
        q.n_slots, q.cap, q.kps, q.u_right = int(d_kps.shape[0]), int(d_kps.shape[1]), ptr(d_kps), ptr(d_u_right)
        q.inv_level_sigma2, q.nlevels = sig.ctypes.data_as(F32P), len(sig)
        q.fx, q.fy, q.cx, q.cy, q.bf = fx, fy, cx, cy, bf
        q.iterations, q.robust, q.max_env_blocks, q.dense = int(iterations), int(bool(robust)), int(max_env_blocks), int(dense)
        q.kf_Tcw_opt, q.pt_pos_opt, q.pt_included = ptr(d_kf_Tcw_opt), ptr(d_pt_pos_opt), ptr(d_pt_included)
        q.trace, q.chi2, q.status = ptr(d_trace), ptr(d_chi2), ptr(d_status)
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_global_bundle_adjustment_batch_device(self._h, C.byref(q), s))


def essential_graph_envelope(n_kf: int, fixed: int, edge_v) -> int:
    """orbx_essential_graph_envelope: the 7 x 7 blocks of one problem's envelope (max_env_blocks)."""
    ev = np.ascontiguousarray(edge_v, dtype=np.int32).reshape(-1, 2)
    n = C.c_int64(0)
    L.check(L.lib().orbx_essential_graph_envelope(int(n_kf), int(fixed), C.c_void_p(ev.ctypes.data), len(ev),
                                                  C.byref(n)))
    return int(n.value)


def essential_graph_edges(ids, parent, children, loop_edges, covisibles, loop_connections, cur_id, loop_id,
                          min_feat: int = 100):
    """The edges of Optimizer::OptimizeEssentialGraph as src/Optimizer.cc:954-1089 inserts them, on
    the host, with the keyframes walked in ascending mnId.  ids: the mnId of the good keyframes, ascending (row
    k of the tables is keyframe ids[k]); parent[k]: the mnId of GetParent() or -1; children[k]:
    the mnIds of its children (hasChild); loop_edges[k]: the mnIds of GetLoopEdges(), in the
    set's order; covisibles[k]: (mnId, weight) pairs in GetCovisiblesByWeight order -- every
    connected keyframe, the weights decide (a keyframe that is not in ids is bad and is skipped);
    loop_connections: an ORDERED list of (mnId, [(mnId, weight), ...]) -- the reference iterates a
    map<KeyFrame*, set<KeyFrame*>>, whose order is pointer order, so the order is taken as given,
    as is the order within each set.  The reference's walk over the keyframes (cc:989) is pointer
    order too (GetAllKeyFrames() copies a set<KeyFrame*>); here the keyframes are walked in
    ascending mnId, by choice: the order of `ids`.  Returns edge_v (E, 2) i32 (row indices: vertex 0, vertex 1)
    and edge_kind (E,) i32 (0: LoopConnections, 1: spanning tree, loop and covisibility edges)."""
    row = {int(m): k for k, m in enumerate(ids)}
    ev, kind, inserted = [], [], set()
    for mi, conns in loop_connections:                       # cc:954-986
        for mj, w in conns:
            if (mi != cur_id or mj != loop_id) and w < min_feat:
                continue
            ev.append((row[int(mi)], row[int(mj)]))
            kind.append(0)
            inserted.add((min(mi, mj), max(mi, mj)))
    for k, mi in enumerate(ids):                             # cc:989-1089
        par = int(parent[k])
        if par >= 0:
            ev.append((k, row[par]))
            kind.append(1)
        loops = [int(m) for m in loop_edges[k]]
        for ml in loops:
            if ml < mi:
                ev.append((k, row[ml]))
                kind.append(1)
        kids = set(int(m) for m in children[k])
        for mn, w in covisibles[k]:
            mn = int(mn)
            if w < min_feat or mn == par or mn in kids or mn in loops:
                continue
            if mn not in row or not mn < mi:
                continue
            if (min(mi, mn), max(mi, mn)) in inserted:
                continue
            ev.append((k, row[mn]))
            kind.append(1)
    return np.array(ev, np.int32).reshape(-1, 2), np.array(kind, np.int32)


class EssentialGraphOptimizer(PoseOptimizer):
    """Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:873-1150) on the GPU
    (csrc/orbx_essgraph.hip): OptimizeEssentialGraph for one map on host arrays and
    essential_graph_batch_device for B maps in HBM.  CorrectLoop's Sim3 propagation, the graph's
    assembly on the device and UpdateNormalAndDepth after it are LoopCorrector's (loopclosing.py);
    essential_graph_edges below is the host assembly.  The handle,
    close() and last_call_us() are PoseOptimizer's."""

    def OptimizeEssentialGraph(self, kf_Tcw, kf_corr, corr_S, loop_kf, edge_v, edge_kind, pt_pos, pt_ref,
                               fix_scale: bool, iterations: int = 0, max_env_blocks: int | None = None,
                               dense: bool = False) -> dict:
        """One map on host arrays: kf_Tcw (K, 12) f32 (the non-corrected poses, ascending mnId),
        kf_corr (K,) rows of corr_S or -1, corr_S (n_corr, 8) f64 (q xyzw, t, s), loop_kf the
        fixed keyframe's row, edge_v (E, 2) / edge_kind (E,), pt_pos (P, 3) f32, pt_ref (P,).
        max_env_blocks None: what the problem needs.  Returns Tcw (K, 12) and pos (P, 3) f32,
        Scw (K, 8) f64, trace (2,) i32, chi2 (2,) f64 and status."""
        T = _f32(kf_Tcw).reshape(-1, 12)
        corr = np.ascontiguousarray(kf_corr, dtype=np.int32)
        cS = np.ascontiguousarray(corr_S, dtype=np.float64).reshape(-1, 8)
        ev = np.ascontiguousarray(edge_v, dtype=np.int32).reshape(-1, 2)
        kind = np.ascontiguousarray(edge_kind, dtype=np.int32)
        pos = _f32(pt_pos).reshape(-1, 3)
        ref = np.ascontiguousarray(pt_ref, dtype=np.int32)
        K, E, P = len(T), len(ev), len(pos)
        if len(corr) != K or len(kind) != E or len(ref) != P:
            raise ValueError("table sizes differ")
        if max_env_blocks is None:
            max_env_blocks = K * (K + 1) // 2 if dense else essential_graph_envelope(K, loop_kf, ev)
        off = [np.array([0, n], np.int32) for n in (K, E, P)]
        loop = np.array([loop_kf], np.int32)
        out = dict(Tcw=np.zeros((K, 12), np.float32), pos=np.zeros((P, 3), np.float32), Scw=np.zeros((K, 8)),
                   trace=np.zeros(2, np.int32), chi2=np.zeros(2))
        status = np.zeros(1, np.int32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        q = L.EssentialGraphBatch()
        q.batch = 1
        q.kf_off, q.n_kf, q.kf_Tcw, q.kf_corr = ptr(off[0]), K, ptr(T), ptr(corr)
        q.corr_S, q.n_corr, q.loop_kf = ptr(cS), len(cS), ptr(loop)
        q.edge_off, q.n_edges, q.edge_v, q.edge_kind = ptr(off[1]), E, ptr(ev), ptr(kind)
        q.pt_off, q.n_pt, q.pt_pos, q.pt_ref = ptr(off[2]), P, ptr(pos), ptr(ref)
        q.fix_scale, q.iterations, q.max_env_blocks, q.dense = int(bool(fix_scale)), int(iterations), int(max_env_blocks), int(dense)
        q.kf_Tcw_opt, q.pt_pos_opt, q.Scw_opt = ptr(out["Tcw"]), ptr(out["pos"]), ptr(out["Scw"])
        q.trace, q.chi2, q.status = ptr(out["trace"]), ptr(out["chi2"]), ptr(status)
        L.check(L.lib().orbx_optimize_essential_graph(self._h, C.byref(q)))
        out["status"] = int(status[0])
        return out

    def essential_graph_batch_device(self, d_kf_off, d_kf_Tcw, d_kf_corr, d_corr_S, d_loop_kf, d_edge_off, d_edge_v,
                                     d_edge_kind, d_pt_off, d_pt_pos, d_pt_ref, fix_scale: bool, max_env_blocks: int,
                                     d_kf_Tcw_opt, d_pt_pos_opt, d_status, d_Scw_opt=None, d_trace=None, d_chi2=None,
                                     iterations: int = 0, dense: bool = False, stream=None) -> None:
        """orbx_optimize_essential_graph_batch_device on device tensors: d_kf_off / d_edge_off /
        d_pt_off (B + 1,) i32, d_kf_Tcw / d_kf_Tcw_opt (n_kf, 12) f32, d_kf_corr (n_kf,) i32,
        d_corr_S (n_corr, 8) f64, d_loop_kf (B,) i32, d_edge_v (n_edges, 2) / d_edge_kind
        (n_edges,) i32, d_pt_pos / d_pt_pos_opt (n_pt, 3) f32, d_pt_ref (n_pt,) i32, d_status
        (B,) i32, d_Scw_opt (n_kf, 8) f64, d_trace (B, 2) i32, d_chi2 (B, 2) f64.  Asynchronous
        on `stream` (or the handle's)."""
        ptr = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())  # noqa: E731
        q = L.EssentialGraphBatch()
        q.batch = int(d_kf_off.shape[0]) - 1
        q.kf_off, q.n_kf, q.kf_Tcw, q.kf_corr = ptr(d_kf_off), int(d_kf_Tcw.shape[0]), ptr(d_kf_Tcw), ptr(d_kf_corr)
        q.corr_S, q.n_corr, q.loop_kf = ptr(d_corr_S), int(d_corr_S.shape[0]), ptr(d_loop_kf)
        q.edge_off, q.n_edges, q.edge_v, q.edge_kind = ptr(d_edge_off), int(d_edge_v.shape[0]), ptr(d_edge_v), ptr(d_edge_kind)
        q.pt_off, q.n_pt, q.pt_pos, q.pt_ref = ptr(d_pt_off), int(d_pt_pos.shape[0]), ptr(d_pt_pos), ptr(d_pt_ref)
        q.fix_scale, q.iterations, q.max_env_blocks, q.dense = int(bool(fix_scale)), int(iterations), int(max_env_blocks), int(dense)
        q.kf_Tcw_opt, q.pt_pos_opt, q.Scw_opt = ptr(d_kf_Tcw_opt), ptr(d_pt_pos_opt), ptr(d_Scw_opt)
        q.trace, q.chi2, q.status = ptr(d_trace), ptr(d_chi2), ptr(d_status)
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_optimize_essential_graph_batch_device(self._h, C.byref(q), s))
