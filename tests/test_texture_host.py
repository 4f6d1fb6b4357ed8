"""Image textures without a GPU: the lookup restatement of tests/texture_util.py
pinned by hand-derived values and the library's host lookup pinned to it bit for bit; the tracer
of texture_util pinned to smooth_util's where nothing is textured; what the test scene holds;
descriptor validation, which happens before any HIP call."""
import ctypes as C
import itertools

import numpy as np
import pytest

import desc_xml
import rq_util
import smooth_util as su
import texture_util as tu
from rq_util import bits
from texture_util import MODES, SIZES, grid_queries, lit_records, replace_all_rays


def rt():
    import ceng795_amd
    return ceng795_amd


def host_lookup(textures, texture, u, v):
    from ceng795_amd.scene import host_texture_lookup
    return host_texture_lookup(textures, texture, u, v)


def grey(values, w, h, **kw):
    """A w x h texture whose three channels hold `values` in row-major order."""
    img = np.repeat(np.array(values, np.uint8).reshape(h, w, 1), 3, axis=2)
    return tu.texture(img, **kw)


# ---------------------------------------------------------------- hand-derived values
def test_hand_derived_lookups():
    """2 x 2 clamp bilinear, channel values 0 40 80 120.  (0.25, 0.25): u = v = 0.5, p = q = 0,
    dx = dy = 0.5, all four terms: 0 + 40/4 + 120/4 + 80/4 = 60.  (0.75, 0.25): u = 1.5, p = 1,
    pn = 2 == w, dx = dy = 0.5: the first term 40 * 0.5 * 0.5 = 10; pn < w fails; qn = 1 < h but the
    linear index w*qn+pn = 4 = w*h is past the end and skipped; the last term is guarded out.
    2 wide, 3 high, (0.75, 1/6): v = 0.5, the same, but index 4 is the first texel of row 2 (the
    kept wrap): 10 + T[4] * 0.25."""
    t22 = grey([0, 40, 80, 120], 2, 2)
    t23 = grey([0, 40, 80, 120, 200, 16], 2, 3)
    sixth = np.float32(1) / np.float32(6)
    assert np.float32(sixth * np.float32(3)) == np.float32(0.5)
    cases = [(t22, 0.25, 0.25, 60.0), (t22, 0.75, 0.25, 10.0), (t23, 0.75, sixth, 10.0 + 200 * 0.25)]
    for tex, u, v, want in cases:
        assert (tu.lookup(tex, u, v) == np.float32(want)).all(), (u, v)
        got = host_lookup([tex], 0, [u], [v])
        assert got.shape == (1, 3) and (got == np.float32(want)).all(), (u, v)
    assert tu.pn_equals_w(t22, 0.75) and not tu.pn_equals_w(t22, 0.25)


# ---------------------------------------------------------------- the grid
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_lookup_equals_restatement_on_the_grid(size):
    w, h = size
    u, v = grid_queries(w, h)
    for k, (interpolation, appearance) in enumerate(MODES):
        tex = tu.random_texture(w, h, 100 * w + 10 * h + k, interpolation=interpolation,
                                appearance=appearance)
        want = tu.lookups(tex, u, v)
        got = host_lookup([tex], 0, u, v)
        assert np.array_equal(bits(got), bits(want)), (size, interpolation, appearance)
        assert np.isfinite(want).all() and (want >= 0).all() and (want <= 255).all()
    # an id out of range gives zeros
    assert (host_lookup([tex], [-1, 1, 7], [0.5] * 3, [0.5] * 3) == 0).all()


# ---------------------------------------------------------------- the tracer with nothing textured
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_tracer_without_textures_is_smooth_utils(scene_dir, depth):
    xml, _, _ = tu.mixed_scene(scene_dir)
    b = rq_util.oracle_batch(xml, cameras=[0])
    want = su.trace(xml, b.o, b.d, depth, False, tu.MIXED_SMOOTH)
    rgb, t, counts, flag, _ = tu.trace(xml, b.o, b.d, depth, False, smooth=tu.MIXED_SMOOTH)
    assert np.array_equal(bits(rgb), bits(want[0])) and np.array_equal(bits(t), bits(want[1]))
    assert counts == want[2] and not flag.any()


def test_lit_restatement_without_textures_is_lit_utils(scene_dir):
    xml, _, _ = tu.mixed_scene(scene_dir)
    b = rq_util.oracle_batch(xml, cameras=[1])
    own = lit_records(b)
    want, shadow = su.restate_lit(xml, b.o, b.d, own, tu.MIXED_SMOOTH)
    got, n = tu.restate_lit(xml, b.o, b.d, own, smooth=tu.MIXED_SMOOTH)
    assert np.array_equal(bits(got), bits(want)) and n == shadow


# ---------------------------------------------------------------- the test scene holds its cases
def test_mixed_scene_holds_its_cases(scene_dir):
    b, rgb, t, counts, flag, seen = tu.reference(scene_dir)
    primary = {k for k, via in seen if via == "primary"}
    assert {tu.REPLACE_KD, tu.BLEND_KD, tu.REPLACE_ALL, "sphere", "untextured", "miss",
            "pn==w"} <= primary, primary
    deeper = {via for k, via in seen if k in (tu.REPLACE_KD, tu.BLEND_KD, tu.REPLACE_ALL)}
    assert "mirror" in deeper or "reflection" in deeper, deeper
    assert "transmission" in deeper, deeper
    assert counts["secondary_rays"] > 100 and counts["shadow_rays"] > 1000
    # no sphere lookup of these inputs sits near a rounding boundary: the GPU test's exemption
    # leaves nothing out unless the GPU disagrees
    for depth, medium in itertools.product((0, 1, 3), (False, True)):
        assert not tu.reference(scene_dir, depth, medium)[4].any(), (depth, medium)
    assert not tu.reference(scene_dir, camera=1)[4].any()
    # textures matter: the same rays on the untextured scene give other colours
    xml, _, _ = tu.mixed_scene(scene_dir)
    plain = su.trace(xml, b.o, b.d, -1, False, tu.MIXED_SMOOTH)[0]
    assert (bits(plain) != bits(rgb)).any(axis=1).sum() >= 300


def test_replace_all_rays(scene_dir):
    """Rays aimed at the loose triangle: the raw texel, no shadow ray, no secondary ray although
    the triangle's material is a mirror."""
    xml, desc, scene = tu.mixed_scene(scene_dir)
    o, d = replace_all_rays(desc)
    rgb, t, counts, flag, seen = tu.trace(xml, o, d, **scene)
    assert {k for k, _ in seen} - {"pn==w"} == {tu.REPLACE_ALL}
    assert counts["shadow_rays"] == 0 and counts["secondary_rays"] == 0
    assert counts["primary_hits"] == len(o) and np.isfinite(t).all()
    assert (rgb.max(axis=1) > 1).all()


# ---------------------------------------------------------------- descriptor validation
def create(desc, **kw):
    """Scene.create on a machine that may have no GPU: only RT_E_INVALID may come back from the
    cases below, and it comes before any HIP call."""
    return rt().Scene.create(desc.d, **kw)


def test_descriptor_validation(scene_dir):
    from ceng795_amd import _lib
    from ceng795_amd.scene import texture_desc
    xml, desc, scene = tu.mixed_scene(scene_dir)
    good = tu.create_kwargs(desc, scene)

    def refused(**change):
        with pytest.raises(rt().RTError) as e:
            create(desc, **{**good, **change})
        assert e.value.code == _lib.RT_E_INVALID, (change.keys(), str(e.value))

    tex = scene["textures"]
    refused(mesh_texture=[-1, -1, 0, 4])                       # id >= num_textures
    refused(triangle_texture=[-2])                             # id < -1
    refused(sphere_texture=[17])
    refused(vertex_uv=None)                                    # a textured mesh without uv
    refused(vertex_uv=None, mesh_texture=None)                 # ... a loose triangle without uv
    for field, value in (("interpolation", 2), ("decal", 3), ("appearance", -1),
                         ("normalizer", 0.0), ("normalizer", float("nan")),
                         ("normalizer", float("inf"))):
        refused(textures=[{**tex[0], field: value}] + tex[1:])
    refused(textures=[{**tex[0], "rgb8": np.zeros((1, 16385, 3), np.uint8)}] + tex[1:])
    # a short struct_size, a NULL rgb8 and a zero size: through the C entry itself
    for breakage in ("struct_size", "rgb8", "width"):
        td, keep = texture_desc(tex, good["mesh_texture"], good["triangle_texture"],
                                good["sphere_texture"])
        if breakage == "struct_size":
            td.struct_size = C.sizeof(_lib.rt_texture_desc) - 8
        elif breakage == "rgb8":
            td.textures[1].rgb8 = None
        else:
            td.textures[2].width = 0
        uv = np.ascontiguousarray(scene["uv"], np.float32)
        surf = _lib.rt_surface_desc(C.sizeof(_lib.rt_surface_desc), None, None,
                                    uv.ctypes.data_as(C.POINTER(C.c_float)))
        h = C.c_void_p()
        rc = _lib.lib().rt_scene_create_textured(C.byref(desc.d), C.byref(surf), C.byref(td), -1,
                                                 C.byref(h))
        assert rc == _lib.RT_E_INVALID and not h.value, breakage
        q = np.zeros(1, rt().scene.TEX_QUERY_DTYPE)
        out = np.zeros(3, np.float32)
        assert _lib.lib().rt_host_texture_lookup_desc(C.byref(td), q.ctypes.data, 1,
                                                      out.ctypes.data) == _lib.RT_E_INVALID
    assert _lib.lib().rt_textures_version() == 1
    # the lookup entries' argument rules need no GPU either
    q = np.zeros(2, rt().scene.TEX_QUERY_DTYPE)
    assert _lib.lib().rt_texture_lookup(None, q.ctypes.data, 2, out.ctypes.data) == _lib.RT_E_INVALID
    assert _lib.lib().rt_texture_lookup_device(None, None, -1, None, None) == _lib.RT_E_INVALID


def test_python_refuses_textures_with_instances(scene_dir):
    from ceng795_amd import _lib
    xml, desc, scene = tu.mixed_scene(scene_dir)
    with pytest.raises(rt().RTError) as e:
        rt().Scene.create(desc.d, textures=scene["textures"], sphere_texture=[0],
                          instance_mesh=[0], instance_material=[0], instance_transform=np.eye(4))
    assert e.value.code == _lib.RT_E_UNSUPPORTED


# ---------------------------------------------------------------- scene files
def test_textures_xml_report(scene_dir):
    """rt_host_textures_xml returns the modes, defaults, ids and uv written into the file."""
    from ceng795_amd import host_textures_xml
    # texture 1 (bilinear, blend_kd, clamp) with its tags left out: the reference's defaults, but
    # for the normalizer, which is then 255
    path, images, scene = tu.textured_xml(scene_dir, "tx_report", defaults=(1,))
    got = host_textures_xml(path)
    assert len(got["textures"]) == 4
    for k, (have, want) in enumerate(zip(got["textures"], scene["textures"])):
        assert have["name"] == f"tex{k}.png"
        assert (have["interpolation"], have["decal"], have["appearance"]) == \
            (want["interpolation"], want["decal"], want["appearance"]), k
        assert np.float32(have["normalizer"]) == np.float32(want["normalizer"]), k
    assert got["textures"][1]["normalizer"] == 255.0
    assert got["mesh_texture"].tolist() == [-1, -1, 0, 1]
    assert got["triangle_texture"].tolist() == [2] and got["sphere_texture"].tolist() == [3]
    assert np.array_equal(bits(got["uv"]), bits(scene["uv"]))
    # unknown words: anything but nearest is bilinear, anything but replace_kd / blend_kd is
    # replace_all, anything but repeat is clamp
    odd = lambda text: (text.replace("<Interpolation>nearest", "<Interpolation>Nearest")  # noqa: E731
                        .replace("<DecalMode>replace_kd", "<DecalMode>replace")
                        .replace("<Appearance>repeat", "<Appearance>mirror"))
    got = host_textures_xml(tu.textured_xml(scene_dir, "tx_odd", change=odd)[0])
    assert (got["textures"][0]["interpolation"], got["textures"][0]["decal"],
            got["textures"][0]["appearance"]) == (tu.BILINEAR, tu.REPLACE_ALL, tu.CLAMP)
    # the other loaders read such a file exactly as before
    xml, desc, _ = tu.mixed_scene(scene_dir)
    other = desc_xml.Desc(path)
    assert other.d.num_vertices == desc.d.num_vertices and other.d.num_meshes == desc.d.num_meshes
    a, b = (tmp_dump(p) for p in (xml, path))
    assert a == b


def tmp_dump(xml):
    import os
    import tempfile
    from ceng795_amd.scene import host_dump_bvh
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "bvh.txt")
        host_dump_bvh(xml, out)
        return open(out).read()


REFUSED = {
    "perlin": lambda t: t.replace("<ImageName>tex1.png", "<ImageName>perlin"),
    "bumpmap": lambda t: t.replace('<Texture id="2">', '<Texture id="2" bumpmap="true">'),
    "background": lambda t: t.replace("  <Textures>", "  <BackgroundTexture>1</BackgroundTexture>\n  <Textures>"),
    "offset": lambda t: t.replace("<Faces>", '<Faces textureOffset="2">'),
    "pairs": lambda t: t[:t.index("<TexCoordData>")] + "<TexCoordData>\n0 0\n1 1\n  </TexCoordData>" +
        t[t.index("</TexCoordData>") + len("</TexCoordData>"):],
    "ply": lambda t: t.replace("<Faces>", '<Faces plyFile="mesh.ply">'),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_textured_xml_refusals(scene_dir, case):
    """Each unsupported construct is refused by name with RT_E_UNSUPPORTED, a missing image with
    RT_E_IO: by the host report where it parses the construct, else by the loader, before any HIP
    call (the images are matched and the uv checked on the host)."""
    from ceng795_amd import _lib, host_textures_xml
    path, images, _ = tu.textured_xml(scene_dir, "tx_refused_" + case, change=REFUSED[case])
    words = {"perlin": "perlin", "bumpmap": "bumpmap", "background": "BackgroundTexture",
             "offset": "textureOffset", "pairs": "TexCoordData", "ply": "plyFile"}
    with pytest.raises(rt().RTError) as e:
        if case == "pairs":  # needs the faces: the loader's check
            rt().Scene(path, textured=True, images=images)
        else:
            host_textures_xml(path)
    assert e.value.code == _lib.RT_E_UNSUPPORTED and words[case] in str(e.value), str(e.value)
    with pytest.raises(rt().RTError) as e:
        rt().Scene(path, textured=True, images=images)
    assert e.value.code == _lib.RT_E_UNSUPPORTED and words[case] in str(e.value), str(e.value)


def test_textured_xml_missing_image_and_switches(scene_dir):
    from ceng795_amd import _lib
    path, images, _ = tu.textured_xml(scene_dir, "tx_missing")
    fewer = {k: v for k, v in images.items() if k != "tex2.png"}
    with pytest.raises(rt().RTError) as e:
        rt().Scene(path, textured=True, images=fewer)
    assert e.value.code == _lib.RT_E_IO and "tex2.png" in str(e.value)
    for other in (dict(instanced=True), dict(instanced=True, motion=True), dict(devices=[0])):
        with pytest.raises(rt().RTError) as e:
            rt().Scene(path, textured=True, images=images, **other)
        assert e.value.code == _lib.RT_E_UNSUPPORTED


# ---------------------------------------------------------------- the records and the symbols
SYMBOLS = ["rt_textures_version", "rt_scene_create_textured", "rt_scene_num_textures",
           "rt_texture_lookup_device", "rt_texture_lookup", "rt_host_texture_lookup_desc",
           "rt_scene_load_xml_textured", "rt_host_textures_xml"]


def test_records_symbols_and_header_macro():
    import os
    import re
    import ceng795_amd
    from ceng795_amd import _lib
    assert C.sizeof(_lib.rt_tex_query) == 16 and ceng795_amd.TEX_QUERY_DTYPE.itemsize == 16
    for name, _ in _lib.rt_tex_query._fields_:
        assert ceng795_amd.TEX_QUERY_DTYPE.fields[name][1] == getattr(_lib.rt_tex_query, name).offset
    assert C.sizeof(_lib.rt_texture) == 32 and C.sizeof(_lib.rt_texture_desc) == 48
    assert C.sizeof(_lib.rt_texture_image) == 24
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                          "ceng795_rt.h")
    text = open(header).read()
    assert re.search(r"^#define CENG795_RT_HAS_TEXTURES 1$", text, re.M)
    assert re.search(r"^#define CENG795_RT_ABI_VERSION 7 ", text, re.M)  # new symbols within ABI 7
    assert _lib.lib().rt_textures_version() == 1 and _lib.lib().rt_abi_version() == 7
    assert re.search(r"enum \{ RT_TEX_NEAREST = 0, RT_TEX_BILINEAR = 1 \};", text)
    assert re.search(r"enum \{ RT_TEX_REPLACE_KD = 0, RT_TEX_BLEND_KD = 1, RT_TEX_REPLACE_ALL = 2 \};", text)
    assert re.search(r"enum \{ RT_TEX_REPEAT = 0, RT_TEX_CLAMP = 1 \};", text)
    assert (tu.NEAREST, tu.BILINEAR, tu.REPLACE_KD, tu.BLEND_KD, tu.REPLACE_ALL, tu.REPEAT, tu.CLAMP) == \
        (_lib.RT_TEX_NEAREST, _lib.RT_TEX_BILINEAR, _lib.RT_TEX_REPLACE_KD, _lib.RT_TEX_BLEND_KD,
         _lib.RT_TEX_REPLACE_ALL, _lib.RT_TEX_REPEAT, _lib.RT_TEX_CLAMP)
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    for name in ("TEX_QUERY_DTYPE", "host_texture_lookup", "host_textures_xml"):
        assert name in ceng795_amd.__all__, name
    assert isinstance(ceng795_amd.Scene.num_textures, property)
    assert callable(ceng795_amd.Scene.texture_lookup)
