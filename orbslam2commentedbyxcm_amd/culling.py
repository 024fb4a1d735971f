"""LocalMapping's two culls and the whole of KeyFrame::SetBadFlag on the GPU (csrc/orbx_culling.hip).

LocalMapping::KeyFrameCulling (src/LocalMapping.cc:708-775), KeyFrame::SetBadFlag
(src/KeyFrame.cc:492-598) with MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:152-212),
LocalMapping::MapPointCulling (src/LocalMapping.cc:185-220) and MapPoint::Observations() on a
CovisibilityGraph whose map lives in HBM.  Every mutating call ends with the observation
refresh's launches, so the graph's CSR, cleaned table and `parent` are right for the next
UpdateLocalMap.  Nothing is read back.  All integer work: results are exact.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .covisibility import CovisibilityGraph, _ptr, _stream

STATUS_NO_PARENT = L.ORBX_CULL_STATUS_NO_PARENT


class MapCuller:
    """The culls of LocalMapping over `graph`.  `tables` are the device tensors of
    orbx_map_tables by name: kf_mp, kf_bad, mp_bad (those of the graph's last
    refresh_observations), kf_keys_un ((K, cap, 7) int32 words or KEYPOINT records), and
    optionally kf_u_right, kf_depth, kf_th_depth, kf_not_erase, kf_to_be_erased.  The result
    tensors live here from call to call."""

    FIELDS = ("kf_mp", "kf_bad", "mp_bad", "kf_keys_un", "kf_u_right", "kf_depth", "kf_th_depth", "kf_not_erase",
              "kf_to_be_erased")

    def __init__(self, graph: CovisibilityGraph, tables: dict | None = None):
        self.graph = graph
        self.tables = dict(tables or {})
        self._t = {}

    def _tables(self) -> L.MapTables:
        m = L.MapTables()
        for k in self.FIELDS:
            setattr(m, k, _ptr(self.tables.get(k)))
        return m

    def _buffers(self) -> dict:
        import torch
        t = self._t
        if not t:
            i32 = dict(dtype=torch.int32, device=torch.device("cuda", self.graph.device))
            mc = self.graph.max_conn
            t.update(cand=torch.full((mc,), -1, **i32), cand_counts=torch.zeros((mc, 3), **i32),
                     n_cand=torch.zeros((1,), **i32), culled=torch.full((mc,), -1, **i32), n_culled=torch.zeros((1,), **i32),
                     n_new_bad_mp=torch.zeros((1,), **i32), status=torch.zeros((1,), **i32),
                     n_mp_culled=torch.zeros((1,), **i32))
        return t

    def keyframe_culling(self, cur_kf: int, monocular: bool = False, stream=None) -> dict:
        """orbx_keyframe_culling_device for the current keyframe: returns the device tensors cand
        (max_conn,), cand_counts (max_conn, 3), n_cand, culled (max_conn,), n_culled, n_new_bad_mp,
        status (1,).  Asynchronous."""
        t = self._buffers()
        m = self._tables()
        L.check(L.lib().orbx_keyframe_culling_device(
            self.graph._h, C.byref(m), int(cur_kf), int(bool(monocular)), _ptr(t["cand"]), _ptr(t["cand_counts"]),
            _ptr(t["n_cand"]), _ptr(t["culled"]), _ptr(t["n_culled"]), _ptr(t["n_new_bad_mp"]), _ptr(t["status"]),
            _stream(stream)))
        return t

    def set_bad_flag(self, ids, stream=None) -> dict:
        """KeyFrame::SetBadFlag on the keyframes `ids` (host ints) in order -- also what SetErase
        runs once kf_not_erase is cleared.  Returns the tensors n_new_bad_mp and status.
        Asynchronous."""
        t = self._buffers()
        m = self._tables()
        a = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        L.check(L.lib().orbx_covis_set_bad_flag_device(
            self.graph._h, C.byref(m), L.i32ptr(a if len(a) else np.zeros(1, np.int32)), len(a), _ptr(t["n_new_bad_mp"]),
            _ptr(t["status"]), _stream(stream)))
        return t

    def map_point_culling(self, cur_kf_id: int, monocular: bool, d_recent, d_n_recent, d_mp_first_kf, d_mp_found,
                          d_mp_visible, stream=None):
        """orbx_map_point_culling_device: d_recent (max_recent,) i32 and d_n_recent (1,) i32 are
        in/out (mlpRecentAddedMapPoints, compacted in order).  Returns the (1,) tensor of the
        points that SetBadFlag ran on.  Asynchronous."""
        t = self._buffers()
        m = self._tables()
        L.check(L.lib().orbx_map_point_culling_device(
            self.graph._h, C.byref(m), int(cur_kf_id), int(bool(monocular)), _ptr(d_recent), _ptr(d_n_recent),
            int(d_recent.shape[0]), _ptr(d_mp_first_kf), _ptr(d_mp_found), _ptr(d_mp_visible), _ptr(t["n_mp_culled"]),
            _stream(stream)))
        return t["n_mp_culled"]

    def observation_counts(self, out=None, stream=None):
        """Observations() of every MapPoint of the last refresh ((n_mappoints,) i32 device tensor;
        0 for a bad one), with the tables' kf_u_right weights.  Asynchronous."""
        import torch
        if out is None:
            n = self.graph.view().n_mappoints
            out = torch.zeros((n,), dtype=torch.int32, device=torch.device("cuda", self.graph.device))
        L.check(L.lib().orbx_covis_observation_counts_device(self.graph._h, _ptr(self.tables.get("kf_u_right")), _ptr(out),
                                                             _stream(stream)))
        return out

    def state(self) -> dict:
        """The result tensors on the host (tests).  Synchronises."""
        import torch
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self._t.items()}
