"""LocalMapping::CreateNewMapPoints' triangulation on the GPU (csrc/orbx_triangulate.hip).

The second half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:307-501): for the
vMatchedPairs SearchForTriangulation produced, the linear triangulation or a stereo
back-projection chosen by the parallax test, the depth-sign, reprojection and scale-consistency
tests, and the new MapPoint's position, normal and distance range.  The keyframes, the matched
pairs and the results stay in HBM: the call reads what ORBmatcher.SearchForTriangulationBatchDevice
left and writes the columns of the MapPoint table that search_local_points_device and Fuse read.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L
from .matcher import I32P, FrameView, _f32

REASONS = L.ORBX_TRIANGULATE_REASONS
OUTPUTS = ("reason", "method", "pos", "normal", "max_distance", "min_distance", "nnew", "new_idx")


def keyframe_geom_device(keys_un, n, Tcw, u_right=None, depth=None, keys=None) -> L.KeyFrameGeomDevice:
    """One orbx_keyframe_geom_device record from device tensors (or raw device addresses):
    keys_un (cap, 7) int32 words (mvKeysUn), n a 1-element int32, u_right / depth (cap,) f32 or
    None, keys (mvKeys) or None for keys_un; Tcw a host 3x4 (or 4x4) pose.  depth None: the
    float mbf / (keys.x - u_right), how ComputeStereoMatches derived mvDepth."""
    def a(t):
        return None if t is None else (int(t) if isinstance(t, int) else t.data_ptr())

    r = L.KeyFrameGeomDevice()
    r.keys_un, r.keys, r.u_right, r.depth, r.n = a(keys_un), a(keys), a(u_right), a(depth), a(n)
    r.Tcw[:] = list(_f32(Tcw)[:3, :4].reshape(-1))
    return r


def keyframe_geom_table(records):
    """A ctypes array of keyframe_geom_device records (build once, pass to every call)."""
    return (L.KeyFrameGeomDevice * max(len(records), 1))(*records)


def new_mappoints_table(P: int, cap: int, device) -> dict:
    """Device tensors for every output of triangulate_pairs_batch_device."""
    import torch
    f32 = dict(dtype=torch.float32, device=device)
    return {"reason": torch.zeros((P, cap), dtype=torch.uint8, device=device),
            "method": torch.zeros((P, cap), dtype=torch.uint8, device=device),
            "pos": torch.zeros((P, cap, 3), **f32), "normal": torch.zeros((P, cap, 3), **f32),
            "max_distance": torch.zeros((P, cap), **f32), "min_distance": torch.zeros((P, cap), **f32),
            "nnew": torch.zeros((P,), dtype=torch.int32, device=device),
            "new_idx": torch.zeros((P, cap), dtype=torch.int32, device=device)}


class Triangulator:
    """triangulate_pairs for one keyframe pair on host arrays and triangulate_pairs_batch_device
    for the matched pairs of many keyframe pairs in HBM.  Borrows an ORBmatcher's library handle
    (the pipeline's triangulation matcher, so both calls share its stream) or owns one."""

    def __init__(self, matcher=None, device: int = 0):
        self._h = None
        self._own = matcher is None
        self._matcher = matcher
        if matcher is not None:
            self.device = matcher.device
            self._h = matcher._h
        else:
            self.device = int(device)
            h = C.c_void_p()
            L.check(L.lib().orbx_matcher_create(self.device, 0.6, 0, C.byref(h)))  # LocalMapping.cc:243
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

    def triangulate_pairs_batch_device(self, kfs, cam: FrameView, pairs, cap: int, d_pairs, d_npairs, out: dict,
                                       mb: float | None = None, mbf: float | None = None, stream=None) -> None:
        """orbx_triangulate_pairs_batch_device: kfs = keyframe_geom_device records (or a
        keyframe_geom_table), pairs (P, 2) (KF1, KF2) indices into kfs -- the table the search
        took --, d_pairs (P, cap, 2) / d_npairs (P,) int32 as SearchForTriangulationBatchDevice
        left them, cam the shared intrinsics + level tables (mb / mbf default to cam.b / cam.bf).
        out: device tensors by name (OUTPUTS; new_mappoints_table), any subset.  Asynchronous."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        tab = kfs if isinstance(kfs, C.Array) else keyframe_geom_table(kfs)
        cv = cam.c()
        o = L.NewMapPoints()
        for k in OUTPUTS:
            t = out.get(k)
            setattr(o, k, None if t is None else t.data_ptr())
        s = None if stream is None else C.c_void_p(getattr(stream, "cuda_stream", stream))
        L.check(L.lib().orbx_triangulate_pairs_batch_device(
            self._h, len(tab) if len(kfs) else 0, C.addressof(tab), C.addressof(cv), len(pr), pr.ctypes.data_as(I32P),
            int(cap), C.c_void_p(d_pairs.data_ptr()), C.c_void_p(d_npairs.data_ptr()),
            float(cam.b if mb is None else mb), float(cam.bf if mbf is None else mbf), C.byref(o), s))

    def triangulate_pairs(self, kf1: dict, kf2: dict, cam: FrameView, matched, mb: float | None = None,
                          mbf: float | None = None) -> dict:
        """orbx_triangulate_pairs on host arrays.  kf1 / kf2: dicts with keys_un (n,)
        KEYPOINT_DTYPE and Tcw, optional keys, u_right, depth (n,) f32; matched (k, 2) int32
        (idx1, idx2).  Returns reason, method (k,) u8, pos, normal (k, 3), max_distance,
        min_distance (k,) f32, nnew and new_idx (nnew,)."""
        keep = []

        def rec(kf):
            ku = np.ascontiguousarray(kf["keys_un"], dtype=L.KEYPOINT_DTYPE)
            n = np.array([len(ku)], np.int32)
            r = L.KeyFrameGeomDevice()

            def host(a, dtype):
                if a is None:
                    return None
                a = np.ascontiguousarray(a, dtype=dtype)
                if len(a) != len(ku):
                    raise ValueError("a keyframe's arrays must have one length")
                a = a if len(a) else np.zeros(1, dtype)
                keep.append(a)
                return a.ctypes.data

            r.keys_un = host(ku, L.KEYPOINT_DTYPE)
            r.keys = host(kf.get("keys"), L.KEYPOINT_DTYPE)
            r.u_right = host(kf.get("u_right"), np.float32)
            r.depth = host(kf.get("depth"), np.float32)
            keep.append(n)
            r.n = n.ctypes.data
            r.Tcw[:] = list(_f32(kf["Tcw"])[:3, :4].reshape(-1))
            return r

        r1, r2 = rec(kf1), rec(kf2)
        mt = np.ascontiguousarray(matched, dtype=np.int32).reshape(-1, 2)
        k = len(mt)
        c = max(k, 1)
        res = {"reason": np.zeros(c, np.uint8), "method": np.zeros(c, np.uint8), "pos": np.zeros((c, 3), np.float32),
               "normal": np.zeros((c, 3), np.float32), "max_distance": np.zeros(c, np.float32),
               "min_distance": np.zeros(c, np.float32), "nnew": np.zeros(1, np.int32), "new_idx": np.zeros(c, np.int32)}
        o = L.NewMapPoints()
        for name in OUTPUTS:
            setattr(o, name, res[name].ctypes.data)
        cv = cam.c()
        mtp = (mt if k else np.zeros((1, 2), np.int32)).ctypes.data_as(I32P)
        L.check(L.lib().orbx_triangulate_pairs(self._h, C.byref(r1), C.byref(r2), C.addressof(cv), k, mtp,
                                               float(cam.b if mb is None else mb),
                                               float(cam.bf if mbf is None else mbf), C.byref(o)))
        nnew = int(res["nnew"][0])
        out = {name: res[name][:k] for name in OUTPUTS if name not in ("nnew", "new_idx")}
        out["nnew"], out["new_idx"] = nnew, res["new_idx"][:nnew]
        return out
