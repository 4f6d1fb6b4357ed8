"""Smooth shading and hit attributes (rt_scene_create_surface, rt_hit_attributes*; DESIGN.md
§4.15), the part that needs no GPU: the restatement the GPU tests judge by (tests/smooth_util.py)
against the CPU oracle, the host vertex normals, the XML's shadingMode, the 48-byte record, the
version symbol and header macro, the exported and declared symbols, the argument rules, the bench
tool's case list, and — from the oracle alone — that every test scene holds the cases it is for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ceng795_amd
import desc_xml
import rq_util
import scenes
import smooth_util as su
from ceng795_amd import _lib
from oracle.cpu_ref import OracleScene

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "ceng795_rt.h")
SYMBOLS = ["rt_surface_version", "rt_scene_create_surface", "rt_scene_load_xml_surface",
           "rt_scene_has_smooth", "rt_host_vertex_normals_desc", "rt_host_mesh_smooth_xml",
           "rt_hit_attributes_device", "rt_hit_attributes"]
bits = rq_util.bits


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["soup1", "soup_depth3", "soup_depth6", "mirror_only"])
def test_restatement_equals_the_oracle(scene_dir, name):
    """With nothing smooth, `trace` is OracleScene.shade_rays bit for bit — rgb, t and the ray
    counters — at depth 0, 1 and the maximum, with and without in_medium, on camera 0's rays."""
    xml = scenes.write(name, scene_dir)
    b = rq_util.oracle_batch(xml, cameras=[0])
    sel = np.arange(0, len(b), max(1, len(b) // 1500))
    o, d = b.o[sel], b.d[sel]
    assert b.hit[sel].sum() >= 100 and (~b.hit[sel]).sum() >= 100
    top = desc_xml.Desc(xml).d.max_recursion_depth
    orc = OracleScene(xml)
    spawned = 0
    for depth in sorted({0, min(1, top), top}):
        for medium in (False, True):
            want, st = orc.shade_rays(o, d, depth=depth, in_medium=medium)
            rgb, t, counts = su.trace(xml, o, d, depth, medium)
            what = (name, depth, medium)
            assert np.array_equal(bits(rgb), bits(want[:, :3])), what
            assert np.array_equal(bits(t), bits(want[:, 3])), what
            assert counts == {k: getattr(st, k) for k in counts}, what
            spawned += counts["secondary_rays"]
    orc.close()
    assert (spawned >= 100) == (top > 0)


# ---------------------------------------------------------------- host entries
@pytest.mark.parametrize("name", ["sm_hf", "sm_mixed", "sm_glass", "sm_single", "sm_deep"])
def test_host_vertex_normals(scene_dir, name):
    """rt_host_vertex_normals_desc equals the sequential loop bit for bit; every vertex a mesh
    uses has a unit normal (or NaN where its faces have no area), the others keep 0."""
    xml, _ = su.case_xml(name, scene_dir)
    desc = desc_xml.Desc(xml)
    want = su.vertex_normals(desc)
    got = ceng795_amd.host_vertex_normals(desc.d)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    used = np.zeros(len(want), bool)
    used[desc.arrays["mesh_faces"][:3 * int(desc.arrays["mesh_face_count"][:desc.d.num_meshes].sum())]] = True
    # (sm_deep's triangles shrink to 2^-99: past the first thirty or so their areas are subnormal
    # or 0 in fp32, the lengths lose their bits, and 0 / 0 stays NaN: no special cases)
    normal_range = used & (np.arange(len(want)) < 90) if name == "sm_deep" else used
    assert normal_range.sum() >= 3
    assert np.allclose(np.linalg.norm(want[normal_range], axis=1), 1, atol=1e-6)
    assert (bits(want[~used]) == 0).all()


def test_flat_faces_move_the_shared_normals(scene_dir):
    """sm_mixed: the flat mesh's faces count in the normals of the vertex row it shares with the
    smooth mesh (HW3 adds every mesh's faces), and loose triangles do not."""
    xml, smooth = su.case_xml("sm_mixed", scene_dir)
    desc = desc_xml.Desc(xml)
    assert tuple(smooth) == (0,) and desc.d.num_meshes == 2 and desc.d.num_triangles == 1
    full = su.vertex_normals(desc)
    keep = desc.d.num_meshes
    desc.d.num_meshes = 1  # the smooth mesh alone
    alone = su.vertex_normals(desc)
    desc.d.num_meshes = keep
    shared, top = slice(4, 8), slice(0, 4)
    assert (np.abs(full[shared] - alone[shared]).max(axis=1) > 1e-3).all()
    assert np.array_equal(bits(full[top]), bits(alone[top]))
    assert (bits(full[12:16]) == 0).all()  # the loose triangle's and the sphere's vertices


def test_host_mesh_smooth_xml(scene_dir):
    for name in su.CASES:
        xml, smooth = su.case_xml(name, scene_dir)
        flags = ceng795_amd.host_mesh_smooth(xml)
        assert flags.tolist() == su.mesh_flags(desc_xml.Desc(xml), smooth).tolist(), name
    assert ceng795_amd.host_mesh_smooth(scenes.write("soup1", scene_dir)).tolist() == [0, 0]
    L = _lib.lib()
    assert L.rt_host_mesh_smooth_xml(None, None, 0) == _lib.RT_E_INVALID
    assert L.rt_host_mesh_smooth_xml(b"/nonexistent/scene.xml", None, 0) == _lib.RT_E_IO


# ---------------------------------------------------------------- the record and the symbols
def test_record_size_and_layout():
    assert C.sizeof(_lib.rt_hit_attr) == 48 and ceng795_amd.HIT_ATTR_DTYPE.itemsize == 48
    for name, _ in _lib.rt_hit_attr._fields_:
        assert ceng795_amd.HIT_ATTR_DTYPE.fields[name][1] == getattr(_lib.rt_hit_attr, name).offset, name
    offs = [getattr(_lib.rt_hit_attr, f).offset for f in
            ("beta", "gamma", "uv", "shading_normal", "flags", "geometric_normal", "pad")]
    assert offs == [0, 4, 8, 16, 28, 32, 44]
    assert C.sizeof(_lib.rt_surface_desc) == 4 * C.sizeof(C.c_void_p)


def test_version_symbol_and_header_macro():
    assert _lib.lib().rt_surface_version() == 1
    assert _lib.lib().rt_abi_version() == 7 == _lib.ABI_VERSION  # new symbols within ABI 7
    text = open(HEADER).read()
    assert re.search(r"^#define CENG795_RT_HAS_SURFACE 1$", text, re.M)
    assert re.search(r"enum \{ RT_ATTR_HIT = 1, RT_ATTR_TRIANGLE = 2, RT_ATTR_SMOOTH = 4 \};", text)
    assert (_lib.RT_ATTR_HIT, _lib.RT_ATTR_TRIANGLE, _lib.RT_ATTR_SMOOTH) == (1, 2, 4)
    assert re.search(r"typedef struct rt_hit_attr \{", text)
    assert re.search(r"typedef struct rt_surface_desc \{", text)


def test_symbols_exported_and_declared():
    text = open(HEADER).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    for method in ("create", "hit_attributes", "hit_attributes_device"):
        assert callable(getattr(ceng795_amd.Scene, method)), method
    assert isinstance(ceng795_amd.Scene.has_smooth, property)
    assert "HIT_ATTR_DTYPE" in ceng795_amd.__all__


# ---------------------------------------------------------------- refusals
def _aligned_bytes(n):
    raw = np.zeros(n + 16, np.uint8)
    return raw, raw.ctypes.data + (-raw.ctypes.data % 16)


@pytest.mark.parametrize("fn", ["rt_hit_attributes", "rt_hit_attributes_device"])
def test_argument_errors_need_no_gpu(fn):
    """n < 0, a NULL pointer with n > 0 and a misaligned pointer are RT_E_INVALID before anything
    touches HIP; what passes them is refused by the NULL scene (none exists without a GPU)."""
    L = _lib.lib()
    f = getattr(L, fn)
    _r, rp = _aligned_bytes(4 * 32)
    _h, hp = _aligned_bytes(4 * 32)
    _a, ap = _aligned_bytes(4 * 48)

    def call(r, h, a, n):
        args = [None, C.c_void_p(r), C.c_void_p(h), n, C.c_void_p(a)]
        rc = f(*args, None) if fn.endswith("_device") else f(*args)
        return rc, L.rt_last_error().decode()

    rc, msg = call(rp, hp, ap, -1)
    assert rc == _lib.RT_E_INVALID and "n < 0" in msg
    for r, h, a in ((None, hp, ap), (rp, None, ap), (rp, hp, None)):
        rc, msg = call(r, h, a, 4)
        assert rc == _lib.RT_E_INVALID and "NULL pointer" in msg
    for r, h, a in ((rp + 4, hp, ap), (rp, hp + 8, ap), (rp, hp, ap + 4)):
        rc, msg = call(r, h, a, 4)
        assert rc == _lib.RT_E_INVALID and "aligned" in msg
    for n in (0, 4):
        rc, msg = call(rp, hp, ap, n)
        assert rc == _lib.RT_E_INVALID and "scene is NULL" in msg


def test_creator_argument_errors_need_no_gpu(scene_dir):
    L = _lib.lib()
    h = C.c_void_p()
    assert L.rt_scene_create_surface(None, None, 0, C.byref(h)) == _lib.RT_E_INVALID
    assert L.rt_scene_load_xml_surface(None, 0, C.byref(h)) == _lib.RT_E_INVALID
    desc = desc_xml.Desc(su.case_xml("sm_single", scene_dir)[0])
    assert L.rt_scene_create_surface(C.byref(desc.d), None, 0, None) == _lib.RT_E_INVALID
    surf = _lib.rt_surface_desc()  # struct_size 0
    assert L.rt_scene_create_surface(C.byref(desc.d), C.byref(surf), 0, C.byref(h)) == _lib.RT_E_INVALID
    assert "struct_size" in L.rt_last_error().decode() and not h.value
    assert L.rt_host_vertex_normals_desc(None, None) == _lib.RT_E_INVALID
    assert L.rt_scene_has_smooth(None) == 0
    with pytest.raises(ValueError):
        ceng795_amd.Scene.create(desc.d, mesh_smooth=[1, 0])
    with pytest.raises(ceng795_amd.RTError):
        ceng795_amd.Scene("unused.xml", devices=[0, 0], smooth=True)


def test_host_vertex_normals_refuses_bad_descriptions(scene_dir):
    """NULL mesh arrays, a mesh without faces and a vertex index out of range are RT_E_INVALID."""
    L = _lib.lib()
    desc = desc_xml.Desc(su.case_xml("sm_mixed", scene_dir)[0])
    out = np.zeros((desc.d.num_vertices, 3), np.float32)
    call = lambda: L.rt_host_vertex_normals_desc(C.byref(desc.d), out.ctypes.data_as(C.POINTER(C.c_float)))  # noqa: E731
    assert call() == _lib.RT_OK
    ints = lambda name: desc.arrays[name].ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    desc.d.mesh_faces = None
    assert call() == _lib.RT_E_INVALID and "NULL" in L.rt_last_error().decode()
    desc.d.mesh_faces, desc.d.mesh_face_count = ints("mesh_faces"), None
    assert call() == _lib.RT_E_INVALID and "NULL" in L.rt_last_error().decode()
    desc.d.mesh_face_count = ints("mesh_face_count")
    assert call() == _lib.RT_OK
    for bad in (0, -3):
        desc.arrays["mesh_face_count"][1] = bad
        assert call() == _lib.RT_E_INVALID and "without faces" in L.rt_last_error().decode(), bad
    desc.arrays["mesh_face_count"][1] = 6
    desc.arrays["mesh_faces"][4] = desc.d.num_vertices
    assert call() == _lib.RT_E_INVALID and "out of range" in L.rt_last_error().decode()
    desc.d.num_meshes = -1
    assert call() == _lib.RT_E_INVALID


def test_lit_restatement_with_nothing_smooth(scene_dir):
    """smooth_util.restate_lit sees the primary rays' query exactly once, and with nothing smooth
    it is lit_util.restate; with the mesh smooth it differs on at least 100 channels."""
    import lit_util
    xml, smooth = su.case_xml("sm_hf", scene_dir)
    b = rq_util.oracle_batch(xml, cameras=[0])
    own = np.broadcast_to(lit_util.scene_records(desc_xml.Desc(xml))[None, :], (len(b), 1))
    plain, n0 = lit_util.restate(xml, b.o, b.d, own)
    same, n1 = su.restate_lit(xml, b.o, b.d, own)
    assert np.array_equal(bits(same), bits(plain)) and n0 == n1 == b.hit.sum()
    smoothed, n2 = su.restate_lit(xml, b.o, b.d, own, smooth)
    assert n2 == n0 and (bits(smoothed[:, :3]) != bits(plain[:, :3])).sum() >= 100
    assert np.array_equal(bits(smoothed[:, 3]), bits(plain[:, 3]))
    # ... which is `trace` at depth 0, the scene's own light being the record
    rgb, t, _ = su.trace(xml, b.o, b.d, smooth=smooth)
    assert np.array_equal(bits(smoothed[:, :3]), bits(rgb)) and np.array_equal(bits(smoothed[:, 3]), bits(t))


def test_bench_tool_dry_run(tmp_path):
    """tools/ray_query_bench.py --smooth --dry-run (with and without --radiance) lists the cases."""
    import json
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HEADER), "..", "tools"))
    import ray_query_bench
    for extra in ([], ["--radiance"]):
        out = tmp_path / "smooth.json"
        assert ray_query_bench.main(extra + ["--smooth", "--dry-run", "--out", str(out)]) == 0
        got = json.loads(out.read_text())
        assert got["dry_run"] is True and got["rays"] == 1920 * 1080 and got["order"] == "tile_8x8"
        cases = got["case_list"]
        assert list(cases) == ["flat/closest", "smooth/closest", "flat/radiance", "smooth/radiance",
                               "flat/attributes", "smooth/attributes"]
        assert [c["scene"] for c in cases.values()] == ["flat", "smooth"] * 3
        assert cases["smooth/attributes"]["entry"] == "rt_hit_attributes_device"


# ---------------------------------------------------------------- the scenes hold their cases
def _flat_normals(b):
    return b.normal[b.hit]


def test_sm_hf_conditions(scene_dir):
    """At least 100 hits whose smooth and flat normals differ by more than 1e-3, and at least 100
    channels of camera 0's frame that differ from the flat scene's."""
    xml, smooth = su.case_xml("sm_hf", scene_dir)
    b, rgb, t, _ = su.reference("sm_hf", scene_dir)
    tr = su.Tracer(xml, smooth)
    rec, shape = tr.orc.intersect_rays(b.o, b.d)
    idx = np.flatnonzero(rec[:, 7] == 1.0)
    nrm = tr.hit_normals(b.o, b.d, rec, shape, idx)
    tr.close()
    assert len(idx) == b.hit.sum() >= 1000 and (~b.hit).sum() >= 100
    assert (np.abs(nrm - rec[idx, 4:7]).max(axis=1) > 1e-3).sum() >= 100
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-5)
    cam0 = b.cam == 0
    flat, _ = OracleScene(xml).render(0, threads=4)
    assert (bits(rgb[cam0]) != bits(flat.reshape(-1, 3))).sum() >= 100
    assert np.array_equal(bits(t[b.hit]), bits(b.t[b.hit]))


def test_sm_mixed_conditions(scene_dir):
    """The frame's first tile (pixels 0..7 x 0..7 of 17 x 9) holds smooth, flat-mesh, loose-triangle
    and sphere hits and misses; the frame's other tiles hold lanes outside the image."""
    xml, smooth = su.case_xml("sm_mixed", scene_dir)
    b, rgb, _, _ = su.reference("sm_mixed", scene_dir)
    desc = desc_xml.Desc(xml)
    assert (desc.cams[0].width, desc.cams[0].height) == (17, 9) and desc.d.num_lights == 4
    orc = OracleScene(xml)
    _, shape = orc.intersect_rays(b.o, b.d)
    orc.close()
    kinds = su.hit_kinds(desc, shape, smooth).reshape(9, 17)
    assert set(kinds[:8, :8].reshape(-1)) == {"smooth", "flat", "loose", "sphere", "miss"}
    assert 17 % 8 and 9 % 8  # tiles 1..5 have pixels outside the image


def test_sm_glass_conditions(scene_dir):
    """At least 100 rays with secondary rays whose colour differs from the flat scene's."""
    xml, smooth = su.case_xml("sm_glass", scene_dir)
    b, rgb, _, counts = su.reference("sm_glass", scene_dir)
    desc = desc_xml.Desc(xml)
    assert desc.d.max_recursion_depth == 3 and tuple(smooth) == (0, 1)
    assert [int(x) for x in desc.arrays["mesh_face_count"][:3]] == [80, 80, 2]
    orc = OracleScene(xml)
    flat, st = orc.shade_rays(b.o, b.d)
    _, shape = orc.intersect_rays(b.o, b.d)
    orc.close()
    ob = su.Objects(desc, smooth)
    mats = ob.mat[np.where(shape >= 0, shape, 0)]
    spawns = (shape >= 0) & (mats <= 1)  # the mirror and the glass material
    differs = (bits(rgb) != bits(flat[:, :3])).any(axis=1)
    assert (spawns & differs).sum() >= 100
    assert counts["secondary_rays"] >= 300 and st.secondary_rays >= 300
    assert ((shape >= 0) & (mats == 0)).sum() >= 50 and ((shape >= 0) & (mats == 1)).sum() >= 50
