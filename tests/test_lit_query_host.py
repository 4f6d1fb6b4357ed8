"""Light samples (rt_shade_rays_lit*, rt_film_shade_rays_lit*), the part that needs no GPU: the
restatement of the depth-0 shading the emitter tests judge by (tests/lit_util.py) against the
CPU oracle, the 48-byte record, the version symbol and header macro, the exported and declared
symbols, and the argument rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ceng795_amd
import desc_xml
import lit_util
import rq_util
import scenes
from ceng795_amd import _lib
from oracle.cpu_ref import OracleScene

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "ceng795_rt.h")
SYMBOLS = ["rt_light_samples_version", "rt_shade_rays_lit_device", "rt_shade_rays_lit",
           "rt_film_shade_rays_lit_device", "rt_film_shade_rays_lit"]


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["soup1", "single_sphere", "c1"])
def test_restatement_equals_the_oracle(scene_dir, name):
    """Fed the scene's own point lights as records, the restatement is OracleScene.shade_rays
    at depth 0 bit for bit — rgb, t and the shadow-ray count — on camera 0's pixel rays."""
    xml = scenes.write(name, scene_dir)
    desc = desc_xml.Desc(xml)
    if name == "c1":
        # a pow that is not the identity
        assert 10 in [desc.mats[m].phong_exponent for m in range(desc.d.num_materials)]
    b = rq_util.oracle_batch(xml, cameras=[0])
    assert b.hit.sum() >= 100 and (~b.hit).sum() >= 100
    orc = OracleScene(xml)
    want, st = orc.shade_rays(b.o, b.d, depth=0)
    orc.close()
    own = np.broadcast_to(lit_util.scene_records(desc)[None, :], (len(b), desc.d.num_lights))
    got, shadow = lit_util.restate(xml, b.o, b.d, own)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert shadow == st.shadow_rays == b.hit.sum() * desc.d.num_lights
    assert (got[b.hit, :3] != 0).any(axis=1).sum() >= 100


def test_restatement_skips_inactive_records(scene_dir):
    """A NaN position is no light: the scene's lights with NaN records between them."""
    xml = scenes.write("single_sphere", scene_dir)
    desc = desc_xml.Desc(xml)
    b = rq_util.oracle_batch(xml, cameras=[0])
    base = lit_util.scene_records(desc)
    own = np.zeros((len(b), 3), ceng795_amd.LIGHT_SAMPLE_DTYPE)
    own["position"] = np.nan
    own[:, 1] = base[0]
    plain, n0 = lit_util.restate(xml, b.o, b.d, np.broadcast_to(base[None, :], (len(b), 1)))
    padded, n1 = lit_util.restate(xml, b.o, b.d, own)
    assert np.array_equal(plain.view(np.uint32), padded.view(np.uint32)) and n0 == n1


# ---------------------------------------------------------------- the record and the symbols
def test_record_size_and_layout():
    assert C.sizeof(_lib.rt_light_sample) == 48 and ceng795_amd.LIGHT_SAMPLE_DTYPE.itemsize == 48
    for name, _ in _lib.rt_light_sample._fields_:
        assert ceng795_amd.LIGHT_SAMPLE_DTYPE.fields[name][1] == \
            getattr(_lib.rt_light_sample, name).offset, name
    assert [getattr(_lib.rt_light_sample, f).offset for f in ("position", "intensity", "normal")] \
        == [0, 16, 32]
    for f in ("position", "intensity", "normal"):
        assert ceng795_amd.LIGHT_SAMPLE_DTYPE[f].shape == (3,)


def test_version_symbol_and_header_macro():
    assert _lib.lib().rt_light_samples_version() == 1
    assert _lib.lib().rt_abi_version() == 7 == _lib.ABI_VERSION  # new symbols within ABI 7
    text = open(HEADER).read()
    assert re.search(r"^#define CENG795_RT_HAS_LIGHT_SAMPLES 1$", text, re.M)
    assert re.search(r"enum \{ RT_QUERY_LIGHTS_SHARED = 4, RT_QUERY_NO_SCENE_LIGHTS = 8 \};", text)
    assert _lib.RT_QUERY_LIGHTS_SHARED == 4 and _lib.RT_QUERY_NO_SCENE_LIGHTS == 8
    assert re.search(r"typedef struct rt_light_sample \{", text)


def test_symbols_exported_and_declared():
    text = open(HEADER).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    for cls in (ceng795_amd.Scene, ceng795_amd.Film):
        for method in ("shade_rays_lit", "shade_rays_lit_device"):
            assert callable(getattr(cls, method)), (cls, method)
    assert "LIGHT_SAMPLE_DTYPE" in ceng795_amd.__all__


# ---------------------------------------------------------------- refusals
def _aligned_bytes(n):
    raw = np.zeros(n + 16, np.uint8)
    return raw, raw.ctypes.data + (-raw.ctypes.data % 16)


@pytest.mark.parametrize("fn", ["rt_shade_rays_lit", "rt_shade_rays_lit_device",
                                "rt_film_shade_rays_lit", "rt_film_shade_rays_lit_device"])
def test_argument_errors_need_no_gpu(fn):
    """NULL lights with k > 0, a misaligned lights pointer and k out of range are RT_E_INVALID
    before anything touches HIP, as are the query entries' own rules; the two new flags pass the
    flag rule (no scene or film exists without a GPU: NULL is what refuses them)."""
    L = _lib.lib()
    f = getattr(L, fn)
    film = "film" in fn
    rays = ceng795_amd.pack_rays(np.zeros((4, 3)), np.ones((4, 3)))
    _out, out_p = _aligned_bytes(4 * 16)
    _xy, xy_p = _aligned_bytes(4 * 8)
    _lt, lt_p = _aligned_bytes(4 * 2 * 48)
    SHARED, DARK = _lib.RT_QUERY_LIGHTS_SHARED, _lib.RT_QUERY_NO_SCENE_LIGHTS
    known = _lib.RT_QUERY_REORDER | _lib.RT_QUERY_IN_MEDIUM | SHARED | DARK

    def call(lp, k, flags, n=4, rp=rays.ctypes.data):
        if film:
            rc = f(None, C.c_void_p(rp), C.c_void_p(xy_p), n, -1, C.c_void_p(lp), k, flags, None)
        else:
            rc = f(None, C.c_void_p(rp), n, -1, C.c_void_p(lp), k, C.c_void_p(out_p), flags, None)
        return rc, L.rt_last_error().decode()

    rc, msg = call(None, 2, 0)
    assert rc == _lib.RT_E_INVALID and "NULL pointer" in msg
    rc, msg = call(lt_p + 8, 2, 0)
    assert rc == _lib.RT_E_INVALID and "aligned" in msg
    for k, flags in ((-1, 0), (257, 0), (65535, 0), (-1, SHARED), (65536, SHARED)):
        rc, msg = call(lt_p, k, flags)
        assert rc == _lib.RT_E_INVALID and "k must be" in msg, (k, flags)
    if not film:
        rc, msg = call(lt_p, 2, 0, n=-1)
        assert rc == _lib.RT_E_INVALID and "n < 0" in msg
        rc, msg = call(lt_p, 2, 0, rp=rays.ctypes.data + 4)
        assert rc == _lib.RT_E_INVALID and "aligned" in msg
    # what passes the light rules is refused by the next rule that needs no GPU: the NULL scene / film
    what = "film is NULL" if film else "scene is NULL"
    for k, flags in ((0, 0), (2, 0), (256, DARK), (65535, SHARED), (0, known), (2, known)):
        rc, msg = call(None if k == 0 else lt_p, k, flags)
        assert rc == _lib.RT_E_INVALID and (what in msg or "NULL" in msg), (k, flags, msg)
        assert "k must be" not in msg and "lights" not in msg, (k, flags, msg)
    if not film:
        rc, msg = call(lt_p, 2, 16)
        assert rc == _lib.RT_E_INVALID and "flag" in msg


def test_new_flags_are_still_unknown_to_the_existing_entries():
    L = _lib.lib()
    rays = ceng795_amd.pack_rays(np.zeros((4, 3)), np.ones((4, 3)))
    _out, out_p = _aligned_bytes(4 * 32)
    for bit in (_lib.RT_QUERY_LIGHTS_SHARED, _lib.RT_QUERY_NO_SCENE_LIGHTS):
        for fn in ("rt_trace_rays", "rt_occluded"):
            rc = getattr(L, fn)(None, C.c_void_p(rays.ctypes.data), 4, C.c_void_p(out_p), bit)
            assert rc == _lib.RT_E_INVALID and "flag" in L.rt_last_error().decode(), (fn, bit)
        rc = L.rt_shade_rays(None, C.c_void_p(rays.ctypes.data), 4, -1, C.c_void_p(out_p), bit, None)
        assert rc == _lib.RT_E_INVALID and "flag" in L.rt_last_error().decode(), bit


def test_bench_tool_dry_run(tmp_path):
    """tools/ray_query_bench.py --radiance --lights --dry-run writes the four cases' list."""
    import json
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HEADER), "..", "tools"))
    import ray_query_bench
    out = tmp_path / "lights.json"
    assert ray_query_bench.main(["--radiance", "--lights", "--dry-run", "--out", str(out)]) == 0
    got = json.loads(out.read_text())
    assert got["dry_run"] is True and got["rays"] == 1920 * 1080 and got["order"] == "tile_8x8"
    cases = got["case_list"]
    assert list(cases) == ["a_plain", "b_shared", "c_per_ray", "d_per_ray_k4"]
    assert [c["records_per_ray"] for c in cases.values()] == [0, 1, 1, 4]
    assert [c["shared"] for c in cases.values()] == [False, True, False, False]
    assert [c["scene_lights"] for c in cases.values()] == [True, False, False, False]
    assert cases["c_per_ray"]["light_bytes"] == 48 * 1920 * 1080


def test_python_light_shapes():
    """(n, k) per ray, (k,) shared; anything else is a ValueError before the library is called."""
    from ceng795_amd.scene import pack_lights
    rec = np.zeros((4, 3), ceng795_amd.LIGHT_SAMPLE_DTYPE)
    lit, k = pack_lights(rec, 4, False)
    assert k == 3 and lit.shape == (12,) and lit.ctypes.data % 16 == 0
    lit, k = pack_lights(rec[0], 4, True)
    assert k == 3 and lit.shape == (3,)
    for bad, n, shared in ((rec, 5, False), (rec[0], 4, False), (rec, 4, True),
                           (np.zeros((4, 3)), 4, False)):
        with pytest.raises(ValueError):
            pack_lights(bad, n, shared)
