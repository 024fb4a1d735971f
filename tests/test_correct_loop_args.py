"""The CorrectLoop entry points (include/orbx.h) reject their arguments before any
device call, and the Python mirror knows them.  Needs only the built library, no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

NAMES = ("orbx_update_normal_and_depth_device", "orbx_correct_loop_propagate_device", "orbx_essential_graph_assemble_device")


def test_symbols_are_exported(orbx_built):
    from orbslam2commentedbyxcm_amd import LoopCorrector  # noqa: F401  (exported)
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = C.CDLL(str(orbx_built))
    for name in NAMES:
        assert name in L.EXPORTED and hasattr(lib, name), name


def _filled(struct, fake, **kw):
    a = struct()
    for name, typ in struct._fields_:
        if typ is C.c_void_p:
            setattr(a, name, fake)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_errors_without_a_graph(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: every case fails first
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    sp = scale.ctypes.data_as(C.POINTER(C.c_float))
    nd = _filled(L.NormalDepth, fake, scale_factors=sp, nlevels=8)
    pr = _filled(L.CorrectLoopPropagate, fake, scale_factors=sp, nlevels=8, cur_kf=1, matched_kf=0)
    asm = _filled(L.EssentialGraphAssembly, fake, cur_kf=1, loop_kf=0, min_feat=100, max_lc=4, max_edges=4)
    nd_call, pr_call, asm_call = (getattr(lib, n) for n in NAMES)
    # a null graph
    assert nd_call(None, C.byref(nd), None, 0, fake, None) == L.ORBX_ERR_ARG
    assert pr_call(None, C.byref(pr), None) == L.ORBX_ERR_ARG
    assert asm_call(None, C.byref(asm), None) == L.ORBX_ERR_ARG
    assert b"null graph" in lib.orbx_last_error()
    # a null struct (with a handle that is never dereferenced)
    assert nd_call(fake, None, None, 0, fake, None) == L.ORBX_ERR_ARG
    assert pr_call(fake, None, None) == L.ORBX_ERR_ARG
    assert asm_call(fake, None, None) == L.ORBX_ERR_ARG
    assert b"null argument" in lib.orbx_last_error()
    # negative capacities
    assert nd_call(fake, C.byref(nd), fake, -1, fake, None) == L.ORBX_ERR_ARG
    assert b"n_ids" in lib.orbx_last_error()
    for kw in (dict(max_lc=-1), dict(max_edges=-1)):
        bad = _filled(L.EssentialGraphAssembly, fake, cur_kf=1, loop_kf=0, min_feat=100, **{"max_lc": 4, "max_edges": 4, **kw})
        assert asm_call(fake, C.byref(bad), None) == L.ORBX_ERR_ARG, kw
        assert b"negative capacity" in lib.orbx_last_error()
    # null pointers
    for name in ("kf_Tcw", "kf_keys_un", "mp_ref_kf", "mp_pos", "normal", "max_distance", "min_distance"):
        assert nd_call(fake, C.byref(_filled(L.NormalDepth, fake, scale_factors=sp, nlevels=8, **{name: None})), None, 0, fake,
                       None) == L.ORBX_ERR_ARG, name
    assert nd_call(fake, C.byref(nd), None, 0, None, None) == L.ORBX_ERR_ARG  # status
    assert nd_call(fake, C.byref(_filled(L.NormalDepth, fake, nlevels=8)), None, 0, fake, None) == L.ORBX_ERR_ARG  # scale_factors
    for name, typ in L.CorrectLoopPropagate._fields_:
        if typ is C.c_void_p and name not in ("Scw", "sim3_R", "sim3_t", "sim3_s"):
            bad = _filled(L.CorrectLoopPropagate, fake, scale_factors=sp, nlevels=8, cur_kf=1, **{name: None})
            assert pr_call(fake, C.byref(bad), None) == L.ORBX_ERR_ARG, name
    for name in ("sim3_R", "sim3_t", "sim3_s"):  # without Scw the three are required
        bad = _filled(L.CorrectLoopPropagate, fake, scale_factors=sp, nlevels=8, cur_kf=1, Scw=None, **{name: None})
        assert pr_call(fake, C.byref(bad), None) == L.ORBX_ERR_ARG, name
    for name, typ in L.EssentialGraphAssembly._fields_:
        if typ is C.c_void_p and name != "loop_kf_ids":
            bad = _filled(L.EssentialGraphAssembly, fake, cur_kf=1, loop_kf=0, min_feat=100, max_lc=4, max_edges=4, **{name: None})
            assert asm_call(fake, C.byref(bad), None) == L.ORBX_ERR_ARG, name
    # nlevels outside 1..32
    for nl in (0, 33):
        assert nd_call(fake, C.byref(_filled(L.NormalDepth, fake, scale_factors=sp, nlevels=nl)), None, 0, fake, None) == L.ORBX_ERR_ARG
        assert pr_call(fake, C.byref(_filled(L.CorrectLoopPropagate, fake, scale_factors=sp, nlevels=nl)), None) == L.ORBX_ERR_ARG
        assert b"nlevels" in lib.orbx_last_error()
