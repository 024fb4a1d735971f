"""The covisibility graph on the GPU (csrc/orbx_covis.hip).

MapPoint::GetObservations() as a CSR over MapPoint ids and KeyFrame::UpdateConnections
(src/KeyFrame.cc:324-415) with the per-keyframe lists that GetVectorCovisibleKeyFrames,
GetBestCovisibilityKeyFrames(N) and GetCovisiblesByWeight(w) read, for a map that lives in HBM:
the [K][cap] MapPoint id table that every search writes (frame_mp), the keyframes' and
MapPoints' bad flags.  The keyframe id stands in for the reference's KeyFrame* wherever its
order is a pointer order.  All integer work: results are exact.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L

STATUS_CAPACITY = L.ORBX_COVIS_STATUS_CAPACITY
STATUS_BAD_KEYFRAME = L.ORBX_COVIS_STATUS_BAD_KEYFRAME
STATUS_DUPLICATE = L.ORBX_COVIS_STATUS_DUPLICATE


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(stream):
    return None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))


class CovisibilityGraph:
    """Owns an orbx_covis handle (its own stream), or borrows another CovisibilityGraph's."""

    def __init__(self, max_keyframes: int = 0, cap: int = 0, max_mappoints: int = 0, max_conn: int = 256,
                 device: int = 0, graph: "CovisibilityGraph | None" = None):
        self._h = None
        self._own = graph is None
        self._graph = graph
        if graph is not None:
            self._h, self.device = graph._h, graph.device
            self.max_keyframes, self.cap, self.max_mappoints, self.max_conn = (
                graph.max_keyframes, graph.cap, graph.max_mappoints, graph.max_conn)
        else:
            self.device = int(device)
            self.max_keyframes, self.cap, self.max_mappoints, self.max_conn = (
                int(max_keyframes), int(cap), int(max_mappoints), int(max_conn))
            h = C.c_void_p()
            L.check(L.lib().orbx_covis_create(self.device, self.max_keyframes, self.cap, self.max_mappoints,
                                              self.max_conn, C.byref(h)))
            self._destroy = L.lib().orbx_covis_destroy  # held: module globals may be gone at exit
            self._h = h
        self._keep = ()
        L.track(self)

    def close(self) -> None:
        """Release the handle (waits for its streams); idempotent.  A borrowed one is left alone."""
        if getattr(self, "_h", None) and self._own:
            self._destroy(self._h)
        self._h = None

    def __del__(self, _finalizing=sys.is_finalizing):
        if not _finalizing():
            self.close()

    @property
    def stream(self) -> int:
        return int(L.lib().orbx_covis_stream(self._h) or 0)

    def refresh_observations(self, kf_mp, kf_n, kf_bad=None, mp_bad=None, n_mappoints: int | None = None,
                             stream=None) -> None:
        """orbx_covis_refresh_observations_device: kf_mp (k, cap) int32, kf_n (k,) int32, kf_bad
        (k,) / mp_bad (n,) uint8 device tensors or None.  The graph keeps kf_n and the bad flags
        (and this object the tensors) for the later calls.  Asynchronous."""
        k = int(kf_mp.shape[0])
        if kf_mp.dim() != 2 or int(kf_mp.shape[1]) != self.cap or not kf_mp.is_contiguous():
            raise ValueError("kf_mp must be a contiguous (keyframes, cap) table")
        n = int(n_mappoints if n_mappoints is not None else (len(mp_bad) if mp_bad is not None else self.max_mappoints))
        self._keep = (kf_mp, kf_n, kf_bad, mp_bad)
        L.check(L.lib().orbx_covis_refresh_observations_device(self._h, k, _ptr(kf_mp), _ptr(kf_n), _ptr(kf_bad), n,
                                                               _ptr(mp_bad), _stream(stream)))

    def update_connections(self, ids, stream=None) -> None:
        """KeyFrame::UpdateConnections of the keyframes `ids` (host ints), as if called one after
        the other in that order.  Asynchronous."""
        a = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        L.check(L.lib().orbx_covis_update_connections_device(self._h, L.i32ptr(a if len(a) else np.zeros(1, np.int32)),
                                                             len(a), _stream(stream)))

    def erase_keyframe(self, kf_id: int, stream=None) -> None:
        """The connection part of KeyFrame::SetBadFlag.  Asynchronous."""
        L.check(L.lib().orbx_covis_erase_keyframe_device(self._h, int(kf_id), _stream(stream)))

    def view(self) -> L.CovisView:
        v = L.CovisView()
        L.check(L.lib().orbx_covis_view_device(self._h, C.byref(v)))
        return v

    def best_covisibles(self, N: int, out=None, out_n=None, stream=None):
        """GetBestCovisibilityKeyFrames(N) of every keyframe: (out (K, N) int32, -1 behind the
        end; out_n (K,)) device tensors (allocated when not given).  Asynchronous."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((self.max_keyframes, int(N)), dtype=torch.int32, device=dev)
        if out_n is None:
            out_n = torch.empty((self.max_keyframes,), dtype=torch.int32, device=dev)
        L.check(L.lib().orbx_covis_best_covisibles_device(self._h, int(N), _ptr(out), _ptr(out_n), _stream(stream)))
        return out, out_n

    def covisibles_by_weight(self, w: int, out=None, out_n=None, stream=None, lists: bool = True):
        """GetCovisiblesByWeight(w) of every keyframe: a prefix of the ordered list; (out (K,
        max_conn) or None, out_n (K,)).  Asynchronous."""
        import torch
        dev = torch.device("cuda", self.device)
        if out is None and lists:
            out = torch.empty((self.max_keyframes, self.max_conn), dtype=torch.int32, device=dev)
        if out_n is None:
            out_n = torch.empty((self.max_keyframes,), dtype=torch.int32, device=dev)
        L.check(L.lib().orbx_covis_covisibles_by_weight_device(self._h, int(w), _ptr(out), _ptr(out_n),
                                                               _stream(stream)))
        return out, out_n

    def ordered(self, kf_id: int):
        """(keyframe ids, weights) of keyframe kf_id's ordered list on the host (what
        KeyFrameDatabase.set_covisibility takes).  Synchronises."""
        kf = np.zeros(self.max_conn, np.int32)
        w = np.zeros(self.max_conn, np.int32)
        n = C.c_int()
        L.check(L.lib().orbx_covis_ordered(self._h, int(kf_id), L.i32ptr(kf), L.i32ptr(w), self.max_conn, C.byref(n)))
        return kf[:n.value].copy(), w[:n.value].copy()

    def state(self) -> dict:
        """Every array of the graph on the host (tests, diagnostics).  Waits for the last call."""
        v = self.view()
        K, mc = v.max_keyframes, v.max_conn

        def get(ptr, shape, dtype=np.int32):
            a = np.zeros(shape, dtype)
            L.check(L.lib().orbx_covis_read(self._h, ptr, a.ctypes.data, a.nbytes))
            return a

        nobs_off = get(v.obs_off, (v.n_mappoints + 1,))
        nobs = int(nobs_off[-1])
        return {"obs_off": nobs_off, "obs_kf": get(v.obs_kf, (nobs,)), "obs_idx": get(v.obs_idx, (nobs,)),
                "mp": get(v.mp, (K, v.cap)), "row_kf": get(v.row_kf, (K, mc)), "row_w": get(v.row_w, (K, mc)),
                "row_n": get(v.row_n, (K,)), "ordered_kf": get(v.ordered_kf, (K, mc)),
                "ordered_w": get(v.ordered_w, (K, mc)), "ordered_n": get(v.ordered_n, (K,)),
                "parent": get(v.parent, (K,)), "first": get(v.first, (K,), np.uint8), "status": get(v.status, (K,))}
