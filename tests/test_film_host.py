"""Films, CPU only (no HIP call is made): the checker the GPU tests use is pinned to the oracle's
MSAA frame, the C ABI announces and exports the film entries, and the refusals that need no film."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import film_util as FU
import scenes
from ceng795_amd import _lib
from oracle.cpu_ref import OracleScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ceng795_rt.h")

FILM_FUNCTIONS = [
    "rt_film_version", "rt_film_create", "rt_film_destroy", "rt_film_clear_device",
    "rt_film_splat_device", "rt_film_shade_rays_device", "rt_film_resolve_device", "rt_film_clear",
    "rt_film_splat", "rt_film_shade_rays", "rt_film_resolve", "rt_film_read", "rt_film_counts"]


@pytest.mark.parametrize("name", list(scenes.MSAA))
def test_restatement_reproduces_the_oracle_msaa_frame(scene_dir, name):
    """Every MSAA sample rebuilt from cpuref_msaa_seed + minstd_uniform, shaded by
    OracleScene.shade_rays, splatted one at a time by the restatement and divided by the weight
    is OracleScene.render_msaa bit for bit: 0 differing channels."""
    xml = scenes.write(name, scene_dir)
    o = OracleScene(xml)
    for seed in (0, 7):
        org, d, xy, (w, h, _) = FU.msaa_samples(xml, 0, seed)
        rad, _ = o.shade_rays(org, d)
        acc = FU.new_film(w, h)
        added, dropped = FU.splat(acc, xy, rad[:, :3])
        assert (added, dropped) == (len(xy), 0)
        ref, _ = o.render_msaa(0, seed=seed, threads=min(16, os.cpu_count() or 1))
        differing = int((FU.bits(FU.resolve(acc)) != FU.bits(ref)).sum())
        assert differing == 0, (name, seed, differing)


def test_header_announces_films_and_library_exports_them():
    text = open(HEADER).read()
    assert re.search(r"^#define CENG795_RT_HAS_FILM 1\b", text, re.M)
    assert re.search(r"enum \{ RT_FILM_GAUSSIAN = 0, RT_FILM_BOX = 1 \}", text)
    L = _lib.lib()
    assert L.rt_film_version() == 1
    for n in FILM_FUNCTIONS:
        assert re.search(r"^\s*(?:int|void)\s+" + n + r"\s*\(", text, re.M), f"{n} not declared"
        assert hasattr(L, n), f"{n} not exported"
        assert n in _lib.SIGNATURES, f"{n} missing from the ctypes table"
    assert (_lib.RT_FILM_GAUSSIAN, _lib.RT_FILM_BOX) == (0, 1)


def test_null_arguments_are_invalid_before_any_hip_call():
    L = _lib.lib()
    h = C.c_void_p()
    scene = C.c_void_p(0)
    assert L.rt_film_create(scene, 8, 8, 0, 0.0, C.byref(h)) == _lib.RT_E_INVALID
    assert not h.value and b"NULL" in L.rt_last_error()
    # (a non-NULL scene is never reached: the out pointer is checked with it)
    assert L.rt_film_create(scene, 8, 8, 0, 0.0, None) == _lib.RT_E_INVALID
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data + (-buf.ctypes.data % 16))
    null = C.c_void_p(0)
    two = (C.c_longlong * 2)()
    calls = [lambda: L.rt_film_clear_device(null, null),
             lambda: L.rt_film_splat_device(null, p, p, 1, null),
             lambda: L.rt_film_shade_rays_device(null, p, p, 1, -1, 0, null),
             lambda: L.rt_film_resolve_device(null, p, null),
             lambda: L.rt_film_clear(null),
             lambda: L.rt_film_splat(null, p, p, 1),
             lambda: L.rt_film_shade_rays(null, p, p, 1, -1, 0, None),
             lambda: L.rt_film_resolve(null, p),
             lambda: L.rt_film_read(null, p),
             lambda: L.rt_film_counts(null, two)]
    for k, call in enumerate(calls):
        assert call() == _lib.RT_E_INVALID, k
    L.rt_film_destroy(null)  # NULL ok


def test_python_film_is_exported():
    import ceng795_amd
    assert ceng795_amd.Film.__name__ == "Film" and "Film" in ceng795_amd.__all__
    with pytest.raises(ValueError):
        ceng795_amd.Film(None, 4, 4, filter="tent")
