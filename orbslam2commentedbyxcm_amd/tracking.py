"""Tracking::UpdateLocalMap and TrackLocalMap's tally on the GPU (csrc/orbx_localmap.hip).

UpdateLocalKeyFrames + UpdateLocalPoints (src/Tracking.cc:1342-1500) for a batch of frames on a
CovisibilityGraph, writing the lists that ORBmatcher.search_local_points_offsets_device reads,
and the count of cc:1047-1081 after the second PoseOptimization.  Nothing is read back between
the steps.  All integer work: results are exact.
"""
from __future__ import annotations

import ctypes as C

from . import _lib as L
from .covisibility import CovisibilityGraph, _ptr, _stream

STATUS_CAPACITY = L.ORBX_LOCAL_MAP_STATUS_CAPACITY
STATUS_EMPTY = L.ORBX_LOCAL_MAP_STATUS_EMPTY


class LocalMapTracker:
    """The per-frame local map of a batch of frames over `graph`.  The in/out lists (local_kf,
    local_kf_n, ref_kf) live here from call to call, as mvpLocalKeyFrames and mpReferenceKF do
    in Tracking; they are (re)allocated, empty, when the batch or a capacity changes."""

    def __init__(self, graph: CovisibilityGraph):
        self.graph = graph
        self._t = {}

    def buffers(self, B: int, max_local_kf: int, max_total: int) -> dict:
        """The device tensors that update_local_map writes for these sizes; a caller may set the
        in/out ones (local_kf, local_kf_n, ref_kf) before the call."""
        import torch
        t = self._t
        if t and (t["local_kf"].shape != (B, max_local_kf) or t["local_ids"].shape[0] != max_total):
            t = self._t = {}
        if not t:
            dev = torch.device("cuda", self.graph.device)
            i32 = dict(dtype=torch.int32, device=dev)
            t.update(local_kf=torch.full((B, max_local_kf), -1, **i32), local_kf_n=torch.zeros((B,), **i32),
                     ref_kf=torch.full((B,), -1, **i32), local_off=torch.zeros((B + 1,), **i32),
                     local_ids=torch.full((max_total,), -1, **i32), counts=torch.zeros((B, 2), **i32),
                     status=torch.zeros((B,), **i32))
        return t

    def update_local_map(self, d_frame_mp, d_n, max_local_kf: int, max_local_points: int, max_total: int,
                         d_parent=None, stream=None) -> dict:
        """orbx_update_local_map_device: d_frame_mp (B, cap) i32 in/out (bad MapPoints become -1),
        d_n (B,) i32, d_parent (max_keyframes,) i32 or None (the graph's own mpParent).  Returns
        the device tensors local_kf (B, max_local_kf), local_kf_n, ref_kf, local_off (B + 1),
        local_ids (max_total,), counts (B, 2), status (B,); this object keeps them.  Asynchronous."""
        if d_frame_mp.dim() != 2 or not d_frame_mp.is_contiguous():
            raise ValueError("d_frame_mp must be a contiguous (batch, cap) table")
        B, cap = int(d_frame_mp.shape[0]), int(d_frame_mp.shape[1])
        t = self.buffers(B, int(max_local_kf), int(max_total))
        u = L.LocalMapUpdate()
        u.batch, u.cap = B, cap
        u.frame_mp, u.n, u.parent = _ptr(d_frame_mp), _ptr(d_n), _ptr(d_parent)
        u.max_local_kf, u.max_local_points, u.max_total = int(max_local_kf), int(max_local_points), int(max_total)
        for k in ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status"):
            setattr(u, k, _ptr(t[k]))
        self._keep = (d_frame_mp, d_n, d_parent)
        L.check(L.lib().orbx_update_local_map_device(self.graph._h, C.byref(u), _stream(stream)))
        return t

    def tally(self, d_frame_mp, d_n, d_outlier, d_observations, only_tracking: bool = False, stereo: bool = False,
              d_recently_relocalised=None, d_mp_found=None, stream=None):
        """orbx_track_local_map_tally_device: d_outlier (B, cap) u8 from PoseOptimization,
        d_observations (n_mappoints,) i32; optional d_recently_relocalised (B,) u8 and d_mp_found
        (n_mappoints,) i32 in/out.  Returns (matches_inliers (B,) i32, ok (B,) u8) device tensors.
        Asynchronous."""
        import torch
        B, cap = int(d_frame_mp.shape[0]), int(d_frame_mp.shape[1])
        dev = d_frame_mp.device
        inl = torch.zeros((B,), dtype=torch.int32, device=dev)
        ok = torch.zeros((B,), dtype=torch.uint8, device=dev)
        q = L.TrackLocalMapTally()
        q.batch, q.cap = B, cap
        q.frame_mp, q.n, q.outlier = _ptr(d_frame_mp), _ptr(d_n), _ptr(d_outlier)
        q.n_mappoints, q.observations = int(d_observations.shape[0]), _ptr(d_observations)
        q.only_tracking, q.stereo = int(bool(only_tracking)), int(bool(stereo))
        q.recently_relocalised, q.mp_found = _ptr(d_recently_relocalised), _ptr(d_mp_found)
        q.matches_inliers, q.ok = _ptr(inl), _ptr(ok)
        L.check(L.lib().orbx_track_local_map_tally_device(self.graph._h, C.byref(q), _stream(stream)))
        return inl, ok

    def state(self) -> dict:
        """The tensors of the last update_local_map on the host (tests).  Synchronises."""
        import torch
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self._t.items()}
