"""LoopClosing::CorrectLoop on the GPU (csrc/orbx_correctloop.hip).

The Sim3 propagation and first map-point correction (src/LoopClosing.cc:482-571), LoopConnections
and the tables of Optimizer::OptimizeEssentialGraph (LoopClosing.cc:595-618, src/Optimizer.cc:
913-1089, 1125-1133) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:386-439) on a
CovisibilityGraph whose map lives in HBM.  The chain is OptimizeSim3 -> propagate -> (the caller's
fusion on kf_mp and a refresh of the observations) -> assemble -> optimize ->
update_normal_and_depth; nothing is read back on the way except the one envelope count that sizes
the optimiser's workspace when the caller does not give it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .covisibility import CovisibilityGraph, _ptr, _stream

NORMAL_STATUS_REF_NOT_OBSERVER = L.ORBX_NORMAL_STATUS_REF_NOT_OBSERVER
NORMAL_STATUS_BAD_INDEX = L.ORBX_NORMAL_STATUS_BAD_INDEX
ASSEMBLY_STATUS_CAPACITY = L.ORBX_ASSEMBLY_STATUS_CAPACITY
ASSEMBLY_STATUS_BAD_KEYFRAME = L.ORBX_ASSEMBLY_STATUS_BAD_KEYFRAME


class LoopCorrector:
    """CorrectLoop over `graph`.  `tables` are device tensors by name: kf_Tcw (K, 12) f32, mp_pos
    (n, 3) f32, mp_corrected_by_kf / mp_corrected_ref / mp_ref_kf (n,) i32, kf_keys_un ((K, cap, 7)
    int32 words or KEYPOINT records), normal (n, 3), max_distance / min_distance (n,) f32.
    scale_factors is mvScaleFactors on the host.  The result tensors live here from call to call."""

    def __init__(self, graph: CovisibilityGraph, tables: dict, scale_factors):
        self.graph = graph
        self.tables = dict(tables)
        self.scale = np.ascontiguousarray(scale_factors, dtype=np.float32)
        self._p = {}
        self._a = {}
        self._o = {}

    def _dev(self):
        import torch
        return torch.device("cuda", self.graph.device)

    def _scale_ptr(self):
        return self.scale.ctypes.data_as(C.POINTER(C.c_float))

    def update_normal_and_depth(self, ids=None, stream=None, status=None, tables: dict | None = None):
        """orbx_update_normal_and_depth_device on the tables' normal / max_distance / min_distance:
        ids a device (m,) i32 tensor, or None for every MapPoint.  `tables` overrides entries of
        the object's (the optimised kf_Tcw and mp_pos, say).  Returns the (1,) status tensor.
        Asynchronous."""
        import torch
        t = dict(self.tables, **(tables or {}))
        if status is None:
            status = self._p.setdefault("nd_status", torch.zeros((1,), dtype=torch.int32, device=self._dev()))
        a = L.NormalDepth()
        for k in ("kf_Tcw", "kf_keys_un", "mp_ref_kf", "mp_pos", "normal", "max_distance", "min_distance"):
            setattr(a, k, _ptr(t.get(k)))
        a.scale_factors, a.nlevels = self._scale_ptr(), len(self.scale)
        L.check(L.lib().orbx_update_normal_and_depth_device(self.graph._h, C.byref(a), _ptr(ids),
                                                            0 if ids is None else int(ids.shape[0]), _ptr(status),
                                                            _stream(stream)))
        return status

    def propagate(self, cur_kf: int, Scw=None, sim3=None, matched_kf: int | None = None, stream=None) -> dict:
        """orbx_correct_loop_propagate_device for the current keyframe: Scw a device (8,) f64 tensor
        (q xyzw, t, s), or sim3 = (R (9,), t (3,), s (1,)) f32 device tensors of OptimizeSim3 with
        matched_kf.  Changes the tables' kf_Tcw, mp_pos, mp_corrected_*, normal and distances and
        the graph; returns the device tensors conn, n_conn, corr_S, kf_corr, kf_Tcw_nc, status.
        Asynchronous."""
        import torch
        g, t = self.graph, self._p
        if "conn" not in t:
            dev, m = self._dev(), g.max_conn + 1
            t.update(conn=torch.full((m,), -1, dtype=torch.int32, device=dev),
                     n_conn=torch.zeros((1,), dtype=torch.int32, device=dev),
                     corr_S=torch.zeros((m, 8), dtype=torch.float64, device=dev),
                     kf_corr=torch.full((g.max_keyframes,), -1, dtype=torch.int32, device=dev),
                     kf_Tcw_nc=torch.zeros((m, 12), dtype=torch.float32, device=dev),
                     status=torch.zeros((1,), dtype=torch.int32, device=dev))
        a = L.CorrectLoopPropagate()
        a.cur_kf = int(cur_kf)
        a.Scw = _ptr(Scw)
        if sim3 is not None:
            a.sim3_R, a.sim3_t, a.sim3_s = (_ptr(x) for x in sim3)
        a.matched_kf = -1 if matched_kf is None else int(matched_kf)
        for k in ("kf_Tcw", "mp_pos", "mp_corrected_by_kf", "mp_corrected_ref", "mp_ref_kf", "kf_keys_un", "normal",
                  "max_distance", "min_distance"):
            setattr(a, k, _ptr(self.tables.get(k)))
        a.scale_factors, a.nlevels = self._scale_ptr(), len(self.scale)
        for k in ("conn", "n_conn", "corr_S", "kf_corr", "kf_Tcw_nc", "status"):
            setattr(a, k, _ptr(t[k]))
        self._keep = (Scw, sim3)
        L.check(L.lib().orbx_correct_loop_propagate_device(g._h, C.byref(a), _stream(stream)))
        self.cur_kf = int(cur_kf)
        return t

    def assembly_tables(self, n_keyframes: int, max_edges: int | None = None, max_lc: int | None = None) -> dict:
        """The result tensors of assemble() for these sizes (kept until the sizes change).  lc_kf /
        lc_w and edge_v / edge_kind carry one guard element behind their capacity."""
        import torch
        g = self.graph
        k, n, m = int(n_keyframes), int(self.tables["mp_pos"].shape[0]), g.max_conn + 1
        max_lc = m * g.max_conn if max_lc is None else int(max_lc)
        max_edges = k * (g.max_conn + 2) + max_lc if max_edges is None else int(max_edges)
        key = (k, n, max_lc, max_edges)
        if self._a.get("key") != key:
            dev = self._dev()
            i32 = dict(dtype=torch.int32, device=dev)
            self._a = dict(key=key, lc_off=torch.zeros((m + 1,), **i32), lc_member=torch.full((m,), -1, **i32),
                           lc_kf=torch.zeros((max_lc + 1,), **i32), lc_w=torch.zeros((max_lc + 1,), **i32),
                           kf_ids=torch.zeros((k,), **i32), kf_row=torch.full((g.max_keyframes,), -1, **i32),
                           n_rows=torch.zeros((1,), **i32), kf_off=torch.zeros((2,), **i32), loop_row=torch.zeros((1,), **i32),
                           kf_corr_rows=torch.zeros((k,), **i32), kf_Tcw_rows=torch.zeros((k, 12), dtype=torch.float32, device=dev),
                           edge_v=torch.zeros((max_edges + 1, 2), **i32), edge_kind=torch.zeros((max_edges + 1,), **i32),
                           n_edges=torch.zeros((1,), **i32), edge_off=torch.zeros((2,), **i32), pt_ref=torch.zeros((n,), **i32),
                           pt_off=torch.zeros((2,), **i32), env_blocks=torch.zeros((1,), dtype=torch.int64, device=dev),
                           status=torch.zeros((1,), **i32))
        return self._a

    def assemble(self, loop_kf: int, d_loop_off, d_loop_kf_ids=None, min_feat: int = 100, max_edges: int | None = None,
                 max_lc: int | None = None, stream=None) -> dict:
        """orbx_essential_graph_assemble_device after propagate(), the caller's fusion and a refresh:
        d_loop_off (k + 1,) / d_loop_kf_ids i32 are GetLoopEdges() as a CSR over the keyframes.
        max_edges defaults to k * (max_conn + 2) + max_lc, max_lc to (max_conn + 1) * max_conn, which
        always fit.  Returns the device tensors of orbx_essential_graph_assembly's outputs by
        name.  Asynchronous."""
        g, p = self.graph, self._p
        t = self.assembly_tables(int(d_loop_off.shape[0]) - 1, max_edges, max_lc)
        max_lc, max_edges = t["key"][2], t["key"][3]
        a = L.EssentialGraphAssembly()
        a.cur_kf, a.loop_kf, a.min_feat = self.cur_kf, int(loop_kf), int(min_feat)
        for name in ("conn", "n_conn", "kf_corr", "kf_Tcw_nc"):
            setattr(a, name, _ptr(p[name]))
        a.kf_Tcw = _ptr(self.tables["kf_Tcw"])
        a.loop_off, a.loop_kf_ids = _ptr(d_loop_off), _ptr(d_loop_kf_ids)
        for name in ("mp_corrected_by_kf", "mp_corrected_ref", "mp_ref_kf"):
            setattr(a, name, _ptr(self.tables[name]))
        a.max_lc, a.max_edges = max_lc, max_edges
        for name in ("lc_off", "lc_member", "lc_kf", "lc_w", "kf_ids", "kf_row", "n_rows", "kf_off", "loop_row",
                     "kf_corr_rows", "kf_Tcw_rows", "edge_v", "edge_kind", "n_edges", "edge_off", "pt_ref", "pt_off",
                     "env_blocks", "status"):
            setattr(a, name, _ptr(t[name]))
        self._keep2 = (d_loop_off, d_loop_kf_ids)
        L.check(L.lib().orbx_essential_graph_assemble_device(g._h, C.byref(a), _stream(stream)))
        return t

    def optimize(self, optimizer, fix_scale: bool, max_env_blocks: int | None = None, iterations: int = 0,
                 stream=None) -> dict:
        """The assembled tables through optimizer.essential_graph_batch_device (an
        EssentialGraphOptimizer) as one problem.  max_env_blocks None: the assembly's env_blocks is
        read back (one synchronisation).  Returns the device tensors kf_Tcw_opt (k, 12), pt_pos_opt
        (n, 3), Scw_opt (k, 8), trace (1, 2), chi2 (1, 2), status (1,): rows [0, n_rows) are the
        keyframes kf_ids.  Asynchronous on `stream` (or the optimiser's: the caller orders it
        behind the assembly)."""
        import torch
        t, p = self._a, self._p
        if max_env_blocks is None:
            max_env_blocks = max(1, int(t["env_blocks"].cpu()[0]))
        k, n = int(t["kf_ids"].shape[0]), int(t["pt_ref"].shape[0])
        o = self._o
        if o.get("key") != (k, n):
            dev = self._dev()
            o.clear()
            o.update(key=(k, n), kf_Tcw_opt=torch.zeros((k, 12), dtype=torch.float32, device=dev),
                     pt_pos_opt=torch.zeros((n, 3), dtype=torch.float32, device=dev),
                     Scw_opt=torch.zeros((k, 8), dtype=torch.float64, device=dev),
                     trace=torch.zeros((1, 2), dtype=torch.int32, device=dev),
                     chi2=torch.zeros((1, 2), dtype=torch.float64, device=dev),
                     status=torch.zeros((1,), dtype=torch.int32, device=dev))
        max_edges = t["key"][3]
        optimizer.essential_graph_batch_device(
            t["kf_off"], t["kf_Tcw_rows"], t["kf_corr_rows"], p["corr_S"], t["loop_row"], t["edge_off"],
            t["edge_v"][:max_edges], t["edge_kind"][:max_edges], t["pt_off"], self.tables["mp_pos"], t["pt_ref"], fix_scale,
            int(max_env_blocks), o["kf_Tcw_opt"], o["pt_pos_opt"], o["status"], d_Scw_opt=o["Scw_opt"], d_trace=o["trace"],
            d_chi2=o["chi2"], iterations=iterations, stream=stream)
        return o

    def state(self) -> dict:
        """Every result tensor on the host (tests).  Synchronises."""
        import torch
        torch.cuda.synchronize()
        out = {}
        for d in (self._p, self._a, self._o):
            out.update({k: v.cpu().numpy() for k, v in d.items() if hasattr(v, "cpu")})
        return out
