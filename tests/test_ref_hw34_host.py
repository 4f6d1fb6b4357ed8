"""The numpy restatements of the later features before the reference's own compiled HW3 / HW4 code
(DESIGN.md §4.19): tests/golden/golden_hw3.npz and golden_hw4.npz hold what oracle/_ref/hw3_harness
and hw4_harness — the unmodified sources — answer for the scenes of tests/ref34_util.py.

Judged here, bit for bit: smooth_util.Tracer and vertex_normals, instance_util.trace and
Composite.intersect, motion_util.trace_at and MotionComposite, smooth_util.restate_lit (lit_util's
terms, with a tiny area light's deterministic sample), texture_util.TexTracer, lookup, sphere_uv and
triangle_uv, and the library's host functions host_texture_lookup and host_vertex_normals.

Hits are compared on every ray; colours on every ray outside the departure classes of
ref34_util.CLASSES, whose membership comes from the restated tree.  Restated as the homework has
it (ref34_util.homework) the helpers equal the goldens on the rays of the classes too — all but
the trees in which the reference reads past a texture's image — so the classes are the whole
difference.  Where the harness exists the stored records are regenerated and compared."""
import os

import numpy as np
import pytest

import desc_xml
import ref34_util as R
import smooth_util as su
import texture_util as tu
from ref34_util import bits

CASES = [(3, n) for n in R.HW3_CASES] + [(4, n) for n in R.HW4_CASES]
IDS = [f"hw{hw}-{n}" for hw, n in CASES]
_GOLDEN = {}


def golden(hw):
    if hw not in _GOLDEN:
        _GOLDEN[hw] = R.load(hw)
    return _GOLDEN[hw]


@pytest.mark.parametrize("hw,name", CASES, ids=IDS)
def test_writers_still_write_the_golden_scenes(scene_dir, hw, name):
    """The SHA-256 of every scene file, and the rays, are the goldens'."""
    z, summary = golden(hw)
    case = R.build(hw, name, scene_dir)
    want = summary["scenes"][name]["sha256"]
    assert R.sha256_file(case.xml) == want["xml"]
    if "plain_xml" in want:
        assert R.sha256_file(case.plain_xml) == want["plain_xml"]
    g = R.golden_case(z, name)
    for k, a in (("o", case.o), ("d", case.d), ("time", case.time)):
        assert np.array_equal(bits(g[k]), bits(a)), k
    assert len(case.o) <= 1500


@pytest.mark.parametrize("hw,name", CASES, ids=IDS)
def test_restatements_equal_the_reference(scene_dir, hw, name):
    """ref34_util.check_restatement; the classes re-derived from the restated trees are the stored
    ones, they leave at least four fifths of the rays in the colour comparison, and the counts of
    the .json are the arrays'."""
    z, summary = golden(hw)
    case = R.build(hw, name, scene_dir)
    g = R.golden_case(z, name)
    cls = R.tree_classes(case)
    assert np.array_equal(cls, g["cls"])
    n = len(case.o)
    assert (cls != 0).sum() <= R.MAX_EXCLUDED * n
    info = summary["scenes"][name]
    assert info["rays"] == info["rays_compared_in_hits"] == n
    assert info["rays_compared_in_colour"] == int((cls == 0).sum())
    assert info["excluded"] == R.class_counts(cls)
    mine = R.check_restatement(case, g)
    assert np.array_equal(mine["near"], g["near"].astype(bool))
    assert g["near"].sum() * 1000 <= n
    if case.kind in ("instanced", "moving"):
        assert not cls.any()
    if name in ("sm_glass", "tx_mixed"):  # the present glass: a recorded departure
        assert (cls & R.BEER).sum() >= 100
    if name in ("sm_clear", "xml_shiny", "tx_clear"):  # Transparency 1 1 1: judged whole
        assert not (cls & R.BEER).any()
    if case.kind == "moving":
        t = case.time
        assert (t == 0).any() and (t < 0).any() and ((t > 0) & (t < 1)).any()


def test_the_clear_glass_is_met():
    """The scenes with Transparency 1 1 1 put the dielectric path before the reference: their
    colours differ from the same rays' in the scene with the present glass wherever a tree leaves
    the glass again — on >= 60 rays (the glass mesh takes 85 of the camera's first hits)."""
    for hw, clear, old in ((3, "sm_clear", "sm_glass"), (4, "tx_clear", "tx_mixed")):
        z, _ = golden(hw)
        assert np.array_equal(bits(z[clear + "__d"]), bits(z[old + "__d"]))
        assert (bits(z[clear + "__rgb"]) != bits(z[old + "__rgb"])).any(axis=1).sum() >= 60
    z, _ = golden(3)
    assert (z["xml_shiny__material"] == 4).sum() >= 20  # first hits on the glass instance


def test_area_light_sample_is_in_the_golden():
    """sm_area is sm_mixed with the tiny area light: same hits, other colours."""
    z, _ = golden(3)
    assert np.array_equal(bits(z["sm_area__t"]), bits(z["sm_mixed__t"]))
    lit = (bits(z["sm_area__rgb"]) != bits(z["sm_mixed__rgb"])).any(axis=1)
    assert lit.sum() >= 60 and not lit[z["sm_area__hit"] == 0].any()


@pytest.mark.parametrize("hw,name", [c for c in CASES if c[1][:2] in ("sm", "tx")],
                         ids=[i for i, c in zip(IDS, CASES) if c[1][:2] in ("sm", "tx")])
def test_vertex_normals(scene_dir, hw, name):
    """smooth_util.vertex_normals and the library's host_vertex_normals against the loader's
    (HW3/src/Scene.cpp:690-695, 870-876) on every vertex some mesh uses."""
    import ceng795_amd
    z, _ = golden(hw)
    case = R.build(hw, name, scene_dir)
    has, vn = z[name + "__vn_has"].astype(bool), z[name + "__vn"]
    desc = desc_xml.Desc(case.plain_xml)
    assert has.sum() >= 12
    for what, got in (("restatement", su.vertex_normals(desc)),
                      ("library", ceng795_amd.host_vertex_normals(desc.d))):
        assert np.array_equal(bits(got[has]), bits(vn[has])), what
        assert not got[~has].any(), what


def test_lookup_grids():
    """texture_util.lookup and host_texture_lookup against Texture::get_color_at on the edge grids
    of every size and mode.  The queries the generator dropped are exactly those whose index
    arithmetic reaches 3 w h: recomputed here from the formula."""
    import ceng795_amd
    z, summary = golden(4)
    textures = R.texel_textures()
    k, u, v, past = R.texel_queries(textures)
    info = summary["texels"]
    assert info["dropped_past_the_image"] == int(past.sum()) > 0
    assert info["queries"] == int((~past).sum()) == len(z["texels__k"])
    assert np.array_equal(z["texels__k"], k[~past])
    assert np.array_equal(bits(z["texels__u"]), bits(u[~past]))
    assert np.array_equal(bits(z["texels__v"]), bits(v[~past]))
    for t, tex in enumerate(textures):
        rows = z["texels__k"] == t
        uu, vv, want = z["texels__u"][rows], z["texels__v"][rows], z["texels__rgb"][rows]
        assert np.array_equal(bits(tu.lookups(tex, uu, vv)), bits(want)), t
        got = ceng795_amd.host_texture_lookup(textures, t, uu, vv)
        assert np.array_equal(bits(got), bits(want)), t
    # only the clamped bilinear form is ever dropped, and never for a 1 x 1 image's ... row q < h - 1
    for t, tex in enumerate(textures):
        if past[k == t].any():
            assert tex["interpolation"] == tu.BILINEAR and tex["appearance"] == tu.CLAMP


@pytest.mark.parametrize("name", list(R.HW4_CASES))
def test_lookup_at_the_golden_hits(scene_dir, name):
    """The lookup at the uv of every textured golden hit (floor, wall, sphere)."""
    import ceng795_amd
    z, summary = golden(4)
    case = R.build(4, name, scene_dir)
    g = R.golden_case(z, name)
    rows = z[name + "__texel_ray"]
    want = z[name + "__texel"]
    tex = g["texture"][rows].astype(np.int32)
    assert set(tex.tolist()) == {0, 1, 3} and len(rows) >= 700
    textures = case.scene["textures"]
    mine = np.stack([tu.lookup(textures[t], a, b) for t, a, b in zip(tex, g["u"][rows], g["v"][rows])])
    assert np.array_equal(bits(mine), bits(want))
    got = ceng795_amd.host_texture_lookup(textures, tex, g["u"][rows], g["v"][rows])
    assert np.array_equal(bits(got), bits(want))
    # the hits left out are the wall's lookups past the image, and rays of that class
    textured = np.flatnonzero(g["texture"] >= 0)
    gone = np.setdiff1d(textured, rows)
    assert len(gone) == summary["scenes"][name]["hit_texels_dropped_past_the_image"] > 0
    assert (g["texture"][gone] == 1).all() and ((g["cls"][gone] & R.PAST_IMAGE) != 0).all()


@pytest.mark.parametrize("hw,name", CASES, ids=IDS)
def test_stored_records_are_the_harness(scene_dir, hw, name):
    """Where the harness is built, its records for the case are the stored bytes."""
    if not os.path.exists(R.HARNESS[hw]):
        pytest.skip("no reference harness here")
    z, _ = golden(hw)
    case = R.build(hw, name, scene_dir)
    g = R.golden_case(z, name)
    rec = R.reference_records(case)
    for k, a in rec.items():
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                              np.ascontiguousarray(g[k]).view(np.uint8)), k
    if case.kind in ("smooth", "textured"):
        has, vn = R.ref_normals(case)
        assert np.array_equal(has, z[name + "__vn_has"].astype(bool))
        assert np.array_equal(bits(vn), bits(z[name + "__vn"]))
