"""The culling entry points (include/orbx.h) reject their arguments before any
device call, and the Python mirror knows them.  Needs only the built library, no GPU."""
from __future__ import annotations

import ctypes as C


def test_symbols_are_exported(orbx_built):
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = C.CDLL(str(orbx_built))
    for name in ("orbx_keyframe_culling_device", "orbx_covis_set_bad_flag_device", "orbx_map_point_culling_device",
                 "orbx_covis_observation_counts_device"):
        assert name in L.EXPORTED and hasattr(lib, name), name


def test_argument_errors_without_a_graph(orbx_built):
    import numpy as np

    from orbslam2commentedbyxcm_amd import MapCuller  # noqa: F401  (exported)
    from orbslam2commentedbyxcm_amd import _lib as L
    lib = L.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: every case fails first
    m = L.MapTables(kf_mp=fake, kf_bad=fake, mp_bad=fake, kf_keys_un=fake)
    ids = np.array([1, 2], np.int32)
    # a null graph
    assert lib.orbx_keyframe_culling_device(None, C.byref(m), 1, 1, fake, fake, fake, fake, fake, fake, fake, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_set_bad_flag_device(None, C.byref(m), L.i32ptr(ids), 2, fake, fake, None) == L.ORBX_ERR_ARG
    assert lib.orbx_map_point_culling_device(None, C.byref(m), 5, 0, fake, fake, 8, fake, fake, fake, fake, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_observation_counts_device(None, None, fake, None) == L.ORBX_ERR_ARG
    assert b"null graph" in lib.orbx_last_error()
    # a null orbx_map_tables, a negative max_recent (with a handle that is never dereferenced)
    assert lib.orbx_keyframe_culling_device(fake, None, 1, 1, fake, fake, fake, fake, fake, fake, fake, None) == L.ORBX_ERR_ARG
    assert lib.orbx_covis_set_bad_flag_device(fake, None, L.i32ptr(ids), 2, fake, fake, None) == L.ORBX_ERR_ARG
    assert lib.orbx_map_point_culling_device(fake, None, 5, 0, fake, fake, 8, fake, fake, fake, fake, None) == L.ORBX_ERR_ARG
    assert b"null map tables" in lib.orbx_last_error()
    assert lib.orbx_map_point_culling_device(fake, C.byref(m), 5, 0, fake, fake, -1, fake, fake, fake, fake, None) == L.ORBX_ERR_ARG
    assert b"max_recent" in lib.orbx_last_error()
    # the switch of the alternative form is known without a GPU
    L.debug_set("cull_serial", 1)
    L.debug_set("cull_serial", -1)
