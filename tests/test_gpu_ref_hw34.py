"""The GPU queries of the later features before the reference's own compiled HW3 / HW4 code
(DESIGN.md §4.19): the records of tests/golden/golden_hw3.npz and golden_hw4.npz — what the
unmodified sources answer for the scenes of tests/ref34_util.py — against Scene.trace_rays,
occluded, hit_attributes, shade_rays (with time=, and in a medium), shade_rays_lit with the tiny
area light's record, and texture_lookup, in both traversal modes.  Bit for bit.

Hits are compared on every ray; a hit normal only where normalising it once more would not move
it on a ray of a renormalisation class (ref34_util.normal_rows_excluded).  Colours on every ray
outside the departure classes stored with the goldens (membership comes from the restated tree,
test_ref_hw34_host.py re-derives it), less the rays texture_util flags for a sphere lookup near an
fp32 rounding boundary: at most 1 in 1,000, as test_gpu_textures.assert_radiance has it."""
import numpy as np
import pytest

import ref34_util as R
import texture_util as tu
from ref34_util import bits

pytestmark = pytest.mark.gpu

MODES = ["fast", "reference"]
CASES = [(3, n) for n in R.HW3_CASES] + [(4, n) for n in R.HW4_CASES]
IDS = [f"hw{hw}-{n}" for hw, n in CASES]
_GOLDEN = {}


def rt():
    import ceng795_amd
    return ceng795_amd


def golden(hw, name):
    if hw not in _GOLDEN:
        _GOLDEN[hw] = R.load(hw)
    z, summary = _GOLDEN[hw]
    return R.golden_case(z, name), z, summary


def open_case(case, traversal):
    if case.kind == "smooth":  # (the plain file: the library takes an area light's samples as records)
        s = rt().Scene(case.plain_xml, smooth=True)
    elif case.kind == "textured":
        s = rt().Scene(case.xml, textured=True, images=case.images)
    else:
        s = rt().Scene(case.xml, instanced=True, motion=case.kind == "moving")
    s.set_traversal(traversal)
    return s


def times(case):
    return case.time if case.kind == "moving" else None


def assert_colours(rad, g, key, what):
    n = len(g["t"])
    near = g["near"].astype(bool)
    assert near.sum() * 1000 <= n, what
    keep = R.colour_rows(g) & ~near
    assert keep.sum() >= (1 - R.MAX_EXCLUDED) * n - near.sum(), what
    differing = int((bits(rad["rgb"]) != bits(g[key])).any(axis=1).sum())
    print(f"{what} {key}: {differing} of {n} rays differ from the reference, {int((~keep).sum())} "
          f"outside the comparison")
    assert np.array_equal(bits(rad["rgb"][keep]), bits(g[key][keep])), what
    hit = g["hit"].astype(bool)
    assert np.array_equal(bits(rad["t"][hit]), bits(g["t"][hit])), what
    assert (bits(rad["t"][~hit]) == bits(np.float32(np.inf))).all(), what


@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("hw,name", CASES, ids=IDS)
def test_hits(scene_dir, hw, name, traversal):
    """trace_rays, hit_attributes and occluded against the `hits` records."""
    g, z, summary = golden(hw, name)
    case = R.build(hw, name, scene_dir)
    assert R.sha256_file(case.xml) == summary["scenes"][name]["sha256"]["xml"]
    hit = g["hit"].astype(bool)
    with open_case(case, traversal) as s:
        hits = s.trace_rays(case.o, case.d, time=times(case))
        again = s.trace_rays(case.o, case.d, time=times(case), reorder=True)
        attr = None if case.kind in ("instanced", "moving") else s.hit_attributes(case.o, case.d, hits)
        # occlusion from the closest hit: half of it is in front of nothing, twice it is behind
        tmax = np.where(hit, g["t"] * np.where(np.arange(len(hit)) % 2, 0.5, 2.0), 1e30).astype(np.float32)
        occ = s.occluded(case.o, case.d, tmax, time=times(case))
    assert np.array_equal(hits.view(np.uint8), again.view(np.uint8))
    assert np.array_equal(hits["object"] >= 0, hit)
    assert np.array_equal(bits(hits["t"][hit]), bits(g["t"][hit]))
    assert (bits(hits["t"][~hit]) == bits(np.float32(np.inf))).all()
    assert np.array_equal(hits["material"], g["material"].astype(np.int32))
    normal = hits["normal"] if attr is None else attr["shading_normal"]
    keep = hit & ~R.normal_rows_excluded(normal, g["cls"])
    assert keep.sum() >= 0.8 * hit.sum()
    assert np.array_equal(bits(normal[keep]), bits(g["normal"][keep]))
    if case.kind in ("instanced", "moving"):
        assert keep[hit].all()
    assert np.array_equal(occ.astype(bool), hit & (g["t"] < tmax))
    # (rt_hit_attr::uv is §4.15's own ((uv0 w) + (uv1 beta)) + (uv2 gamma), by its contract not
    # HW4's (uva + beta (uvb - uva)) + gamma (uvc - uva): HW4's u, v are inside the ray trees only,
    # where test_radiance and test_lookup_at_the_golden_hits meet them)


@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("medium", [False, True])
@pytest.mark.parametrize("hw,name", [c for c in CASES if c[1] != "sm_area"],
                         ids=[i for i, c in zip(IDS, CASES) if c[1] != "sm_area"])
def test_radiance(scene_dir, hw, name, medium, traversal):
    """shade_rays at the scene's depth against Scene::trace_ray."""
    g, _, _ = golden(hw, name)
    case = R.build(hw, name, scene_dir)
    with open_case(case, traversal) as s:
        rad = s.shade_rays(case.o, case.d, in_medium=medium, time=times(case))
    assert_colours(rad, g, "rgb_medium" if medium else "rgb", (name, medium, traversal))


@pytest.mark.parametrize("traversal", MODES)
def test_area_light_record(scene_dir, traversal):
    """shade_rays_lit with the scene's lights and one shared emitter record — the position,
    intensity and normal of the area light whose every sample is its position — against HW3's
    trace_ray on the scene with that <AreaLight>."""
    g, _, _ = golden(3, "sm_area")
    case = R.build(3, "sm_area", scene_dir)
    with open_case(case, traversal) as s:
        rad = s.shade_rays_lit(case.o, case.d, R.area_record(case), shared=True, scene_lights=True)
        plain = s.shade_rays(case.o, case.d)
    assert_colours(rad, g, "rgb", ("sm_area", traversal))
    assert (bits(rad["rgb"]) != bits(plain["rgb"])).any(axis=1).sum() >= 60


def test_lookup_grids(scene_dir):
    """texture_lookup against Texture::get_color_at on the edge grids of every size and mode."""
    _, z, _ = golden(4, "tx_mixed")
    textures = R.texel_textures()
    _, desc, _ = tu.mixed_scene(scene_dir)
    with rt().Scene.create(desc.d, textures=textures, sphere_texture=[0]) as s:
        assert s.num_textures == len(textures) == 24
        got = s.texture_lookup(z["texels__k"], z["texels__u"], z["texels__v"])
    assert len(got) >= 12000
    assert np.array_equal(bits(got), bits(z["texels__rgb"]))


@pytest.mark.parametrize("name", list(R.HW4_CASES))
def test_lookup_at_the_golden_hits(scene_dir, name):
    g, z, _ = golden(4, name)
    case = R.build(4, name, scene_dir)
    rows = z[name + "__texel_ray"]
    with open_case(case, "fast") as s:
        got = s.texture_lookup(g["texture"][rows].astype(np.int32), g["u"][rows], g["v"][rows])
    assert len(rows) >= 700
    assert np.array_equal(bits(got), bits(z[name + "__texel"]))
