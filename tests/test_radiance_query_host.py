"""Radiance queries (rt_shade_rays*), the part that needs no GPU: the 16-byte record, the version
symbol and header macro, the exported and declared symbols, and the argument rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ceng795_amd
from ceng795_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "ceng795_rt.h")
SYMBOLS = ["rt_radiance_query_version", "rt_shade_rays_device", "rt_shade_rays",
           "rt_set_radiance_scratch_limit", "rt_stream_frame_scratch_bytes"]


def test_record_size_and_layout():
    assert C.sizeof(_lib.rt_radiance) == 16 and ceng795_amd.RADIANCE_DTYPE.itemsize == 16
    for name, _ in _lib.rt_radiance._fields_:
        assert ceng795_amd.RADIANCE_DTYPE.fields[name][1] == getattr(_lib.rt_radiance, name).offset
    assert ceng795_amd.RADIANCE_DTYPE["rgb"].shape == (3,)


def test_version_symbol_and_header_macro():
    assert _lib.lib().rt_radiance_query_version() == 1
    assert _lib.lib().rt_abi_version() == 7 == _lib.ABI_VERSION  # new symbols within ABI 7
    text = open(HEADER).read()
    assert re.search(r"^#define CENG795_RT_HAS_RADIANCE_QUERY 1$", text, re.M)
    assert re.search(r"enum \{ RT_QUERY_IN_MEDIUM = 2 \};", text)
    assert _lib.RT_QUERY_IN_MEDIUM == 2 and _lib.RT_QUERY_REORDER == 1
    assert re.search(r"typedef struct rt_radiance \{ float rgb\[3\]; float t; \} rt_radiance;", text)


def test_symbols_exported_and_declared():
    text = open(HEADER).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^(?:int|long long) " + name + r"\(", text, re.M), name
    for method in ("shade_rays", "shade_rays_device", "set_radiance_scratch_limit"):
        assert callable(getattr(ceng795_amd.Scene, method))


@pytest.mark.parametrize("fn", ["rt_shade_rays", "rt_shade_rays_device"])
def test_argument_errors_need_no_gpu(fn):
    """n < 0, an unknown flag bit, a NULL pointer with n > 0 and a misaligned pointer are
    RT_E_INVALID before anything touches HIP (no scene exists on a machine without a GPU, and a
    NULL scene is RT_E_INVALID too)."""
    L = _lib.lib()
    f = getattr(L, fn)
    rays = ceng795_amd.pack_rays(np.zeros((4, 3)), np.ones((4, 3)))
    out = np.zeros(4 * 16 + 16, np.uint8)
    out_p = out.ctypes.data + (-out.ctypes.data % 16)
    scene = C.c_void_p(None)
    known = _lib.RT_QUERY_REORDER | _lib.RT_QUERY_IN_MEDIUM

    def call(rp, n, op, flags, depth=-1):
        rc = f(scene, C.c_void_p(rp), n, depth, C.c_void_p(op), flags, None)
        return rc, L.rt_last_error().decode()

    rc, msg = call(rays.ctypes.data, -1, out_p, 0)
    assert rc == _lib.RT_E_INVALID and "n < 0" in msg
    for flags in (4, 8, ~known, known | 4):
        rc, msg = call(rays.ctypes.data, 4, out_p, flags)
        assert rc == _lib.RT_E_INVALID and "flag" in msg, flags
    rc, msg = call(None, 4, out_p, 0)
    assert rc == _lib.RT_E_INVALID and "NULL pointer" in msg
    rc, msg = call(rays.ctypes.data, 4, None, 0)
    assert rc == _lib.RT_E_INVALID and "NULL pointer" in msg
    rc, msg = call(rays.ctypes.data + 4, 4, out_p, 0)
    assert rc == _lib.RT_E_INVALID and "aligned" in msg
    rc, msg = call(rays.ctypes.data, 4, out_p + 8, 0)
    assert rc == _lib.RT_E_INVALID and "aligned" in msg
    # both known flags pass the flag rule: the next rule (the scene) is what refuses
    for flags in (0, _lib.RT_QUERY_REORDER, _lib.RT_QUERY_IN_MEDIUM, known):
        rc, msg = call(rays.ctypes.data, 4, out_p, flags)
        assert rc == _lib.RT_E_INVALID and "scene is NULL" in msg, flags


def test_in_medium_is_still_unknown_to_the_other_queries():
    L = _lib.lib()
    rays = ceng795_amd.pack_rays(np.zeros((4, 3)), np.ones((4, 3)))
    out = np.zeros(4 * 32 + 16, np.uint8)
    out_p = out.ctypes.data + (-out.ctypes.data % 16)
    for fn in ("rt_trace_rays", "rt_occluded"):
        rc = getattr(L, fn)(None, C.c_void_p(rays.ctypes.data), 4, C.c_void_p(out_p),
                            _lib.RT_QUERY_IN_MEDIUM)
        assert rc == _lib.RT_E_INVALID and "flag" in L.rt_last_error().decode(), fn


def test_scratch_limit_and_probe_refuse_a_null_scene():
    L = _lib.lib()
    assert L.rt_set_radiance_scratch_limit(None, 1 << 20) == _lib.RT_E_INVALID
    assert L.rt_stream_frame_scratch_bytes(None, None) == _lib.RT_E_INVALID
