"""Image textures on the GPU (rt_scene_create_textured, rt_texture_lookup*), bit
for bit against the restatement of tests/texture_util.py (which test_texture_host.py pins: its
lookup by hand-derived values, its tracer to smooth_util's where nothing is textured; that the
scene holds its cases is asserted there).

Trees that touch a textured sphere go through the fp64 acos / atan2, ocml's on the device and
glibc's in the restatement.  A ray may be left out of the bit comparison only if the restatement
found an fp64 value of such a hit within 4 fp64 ulps of an fp32 rounding boundary; the host test
asserts there is no such ray for these inputs, so nothing is left out unless the GPU disagrees."""
import ctypes as C

import numpy as np
import pytest

import desc_xml
import film_util as FU
import rq_util
import scenes
import smooth_util as su
import texture_util as tu
from oracle.cpu_ref import OracleScene
from rq_util import bits, same_records, shade_device
from texture_util import MODES as TEX_MODES, SIZES, grid_queries, lit_records, replace_all_rays

pytestmark = pytest.mark.gpu

MODES = ["fast", "reference"]
COUNTERS = ("primary_rays", "primary_hits", "shadow_rays", "secondary_rays")


def rt():
    import ceng795_amd
    return ceng795_amd


def open_mixed(scene_dir, traversal="fast"):
    xml, desc, scene = tu.mixed_scene(scene_dir)
    s = rt().Scene.create(desc.d, **tu.create_kwargs(desc, scene))
    s.set_traversal(traversal)
    assert s.num_textures == 4 and s.has_smooth
    return s


def assert_radiance(rad, rgb, t, near, what):
    """Bit for bit, but for the rays whose restated tree has a sphere lookup near a rounding
    boundary: at most 1 in 1,000 of them."""
    assert near.sum() * 1000 <= len(near), (what, int(near.sum()))
    keep = ~near
    assert np.array_equal(bits(rad["rgb"][keep]), bits(rgb[keep])), what
    assert np.array_equal(bits(rad["t"]), bits(t)), what


# ---------------------------------------------------------------- the device lookup
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_lookup(scene_dir, size):
    """rt_texture_lookup on the edge grid and 4,096 seeded random queries per texture, four mode
    pairs as four textures of one scene; ids out of range give zeros."""
    w, h = size
    xml, desc, _ = tu.mixed_scene(scene_dir)
    textures = [tu.random_texture(w, h, 100 * w + 10 * h + k, interpolation=i, appearance=a)
                for k, (i, a) in enumerate(TEX_MODES)]
    gu, gv = grid_queries(w, h)
    rng = np.random.default_rng(w * 31 + h)
    u = np.concatenate([gu, rng.uniform(-1.5, 2.5, 4096).astype(np.float32)])
    v = np.concatenate([gv, rng.uniform(-1.5, 2.5, 4096).astype(np.float32)])
    with rt().Scene.create(desc.d, textures=textures, sphere_texture=[0]) as s:
        assert s.num_textures == 4 and not s.has_smooth
        for k, tex in enumerate(textures):
            got = s.texture_lookup(k, u, v)
            want = tu.lookups(tex, u, v)
            assert np.array_equal(bits(got), bits(want)), (size, k)
        ids = np.array([-1, 4, 2 ** 31 - 1, -2 ** 31, 0], np.int32)
        got = s.texture_lookup(ids, np.full(5, 0.5, np.float32), np.full(5, 0.5, np.float32))
        assert (got[:4] == 0).all() and np.array_equal(bits(got[4]), bits(tu.lookup(textures[0], 0.5, 0.5)))
        assert s.texture_lookup(0, [], []).shape == (0, 3)


def test_device_lookup_entry(scene_dir):
    """The device entry on a stream: a prefix, an untouched tail, n = 0, a misaligned pointer."""
    import torch
    from ceng795_amd import _lib
    with open_mixed(scene_dir) as s:
        n = 300
        rng = np.random.default_rng(4)
        q = np.zeros(n, rt().scene.TEX_QUERY_DTYPE)
        q["texture"] = rng.integers(-1, 5, n)
        q["u"], q["v"] = rng.uniform(-1, 2, n), rng.uniform(-1, 2, n)
        want = s.texture_lookup(q["texture"], q["u"], q["v"])
        dq = rq_util.to_device(q)
        out = torch.full((3 * n + 8,), -7.0, dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        call = _lib.lib().rt_texture_lookup_device
        for k in (0, 1, 65, n):
            out.fill_(-7.0)
            torch.cuda.synchronize()
            assert call(s.handle, dq.data_ptr(), k, out.data_ptr(), st.cuda_stream) == 0
            st.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(bits(got[:3 * k]), bits(want[:k].reshape(-1))), k
            assert (got[3 * k:] == -7.0).all(), k
        assert call(s.handle, dq.data_ptr() + 4, 1, out.data_ptr(), None) == _lib.RT_E_INVALID
        assert call(s.handle, None, 1, out.data_ptr(), None) == _lib.RT_E_INVALID


# ---------------------------------------------------------------- radiance on tx_mixed
@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("medium", [False, True])
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_mixed_radiance(scene_dir, depth, medium, traversal):
    b, rgb, t, counts, near, _ = tu.reference(scene_dir, depth, medium)
    with open_mixed(scene_dir, traversal) as s:
        rad, st = s.shade_rays(b.o, b.d, depth=depth, in_medium=medium, stats=True)
        again = s.shade_rays(b.o, b.d, depth=depth, in_medium=medium, reorder=True)
    differing = int((bits(rad["rgb"]) != bits(rgb)).any(axis=1).sum())
    print(f"tx_mixed depth {depth} medium {medium} {traversal}: {differing} of {len(b)} rays "
          f"differ from the restatement, {int(near.sum())} near a rounding boundary")
    assert_radiance(rad, rgb, t, near, (depth, medium, traversal))
    assert same_records(again, rad)
    got = {k: getattr(st, k) for k in COUNTERS}
    # (the library counts every first hit; the restatement only those at the scene's depth)
    got["primary_hits"] = got["primary_hits"] if depth == 3 else 0
    assert got == counts, (depth, medium)


# ---------------------------------------------------------------- frames
@pytest.mark.parametrize("traversal", MODES)
def test_mixed_frame_with_partial_tiles(scene_dir, traversal):
    """The 17 x 9 frame = shade_rays of its pixel rays = the restatement, counters included."""
    b, rgb, t, counts, near, _ = tu.reference(scene_dir, camera=1)
    with open_mixed(scene_dir, traversal) as s:
        assert not s.records_ok(1)
        frame, st = s.render_image(1)
        rad = s.shade_rays(b.o, b.d)
    assert frame.shape == (9, 17, 3)
    assert np.array_equal(bits(frame.reshape(-1, 3)), bits(rad["rgb"]))
    assert_radiance(rad, rgb, t, near, traversal)
    assert {k: getattr(st, k) for k in COUNTERS} == counts


def test_mixed_msaa_frame_equals_film(scene_dir):
    """Camera 2 (17 x 9, NumSamples 4): the MSAA frame equals a Gaussian film fed the same samples
    through the fused entry, bit for bit."""
    xml, _, _ = tu.mixed_scene(scene_dir)
    seed = 5
    o, d, xy, (w, h, S) = FU.msaa_samples(xml, 2, seed)
    assert (w, h, S) == (17, 9, 4)
    with open_mixed(scene_dir) as s:
        s.set_msaa_seed(seed)
        frame, _ = s.render_image(2)
        with rt().Film(s, w, h) as film:
            film.shade_rays(o, d, xy)
            got = film.resolve()
    assert FU.same_bits(frame, got)
    with rt().Scene(xml, smooth=True) as plain:  # the textures are in it
        plain.set_msaa_seed(seed)
        assert (bits(plain.render_image(2)[0]) != bits(frame)).sum() >= 100


# ---------------------------------------------------------------- light samples
@pytest.mark.parametrize("traversal", MODES)
def test_mixed_light_samples(scene_dir, traversal):
    """One emitter record per ray: kd' is in the own-light term."""
    xml, _, scene = tu.mixed_scene(scene_dir)
    b = rq_util.oracle_batch(xml, cameras=[1])
    own = lit_records(b)
    want, shadow = tu.restate_lit(xml, b.o, b.d, own, **scene)
    plain, _ = tu.restate_lit(xml, b.o, b.d, own, smooth=tu.MIXED_SMOOTH)
    assert (bits(want[:, :3]) != bits(plain[:, :3])).any(axis=1).sum() >= 30
    with open_mixed(scene_dir, traversal) as s:
        rad, st = s.shade_rays_lit(b.o, b.d, own, scene_lights=False, depth=0, stats=True)
    assert np.array_equal(bits(rad["rgb"]), bits(want[:, :3]))
    assert np.array_equal(bits(rad["t"]), bits(want[:, 3]))
    assert st.shadow_rays == shadow


# ---------------------------------------------------------------- REPLACE_ALL
def test_replace_all(scene_dir):
    """A batch that only hits the loose triangle, whose material is a mirror: the raw texel, no
    shadow ray, no secondary ray; the frame scratch is what the scene takes for any other batch of
    that size."""
    import torch
    xml, desc, scene = tu.mixed_scene(scene_dir)
    o, d = replace_all_rays(desc)
    rgb, t, counts, near, _ = tu.trace(xml, o, d, **scene)
    other = tu.reference(scene_dir)[0]
    stream = torch.cuda.current_stream().cuda_stream
    for medium in (False, True):
        with open_mixed(scene_dir) as s:
            rad, st = s.shade_rays(o, d, in_medium=medium, stats=True)
            assert np.array_equal(bits(rad["rgb"]), bits(rgb)) and np.array_equal(bits(rad["t"]), bits(t))
            assert st.shadow_rays == 0 and st.secondary_rays == 0 and st.primary_hits == len(o)
            assert s.stream_frame_scratch_bytes(stream) == 0
            shade_device(s, o, d)
            here = s.stream_frame_scratch_bytes(stream)
            s.release_stream(stream)
            shade_device(s, other.o[:len(o)], other.d[:len(o)])
            assert here == s.stream_frame_scratch_bytes(stream) > 0
            shade_device(s, o, d, depth=0)  # depth 0 cannot recurse: no more scratch
            assert s.stream_frame_scratch_bytes(stream) == here


# ---------------------------------------------------------------- independence
@pytest.mark.parametrize("traversal", MODES)
def test_independence(scene_dir, traversal):
    b, rgb, t, _, near, _ = tu.reference(scene_dir)
    with open_mixed(scene_dir, traversal) as s:
        whole = s.shade_rays(b.o, b.d)
        first, tail = shade_device(s, b.o[:50], b.d[:50], pad=64)
        assert same_records(first, whole[:50]) and (tail == 0xA5).all()
        pick = np.random.default_rng(7).permutation(len(b))[:200]
        assert same_records(s.shade_rays(b.o[pick], b.d[pick]), whole[pick])
        assert same_records(s.shade_rays(b.o[pick], b.d[pick], reorder=True), whole[pick])
    assert_radiance(whole, rgb, t, near, traversal)


# ---------------------------------------------------------------- unchanged scenes
@pytest.mark.parametrize("name", ["soup1", "soup_depth3", "msaa4"])
def test_untextured_scenes_are_unchanged(scene_dir, name):
    """rt_scene_create_textured with a NULL texture descriptor, and with one that names no object,
    gives rt_scene_create_surface's scene: frames, counters and queries byte for byte; and the
    flat scene made the old way still equals the oracle."""
    from ceng795_amd import _lib
    xml = scenes.write(name, scene_dir)
    desc = desc_xml.Desc(xml)
    b = rq_util.oracle_batch(xml, cameras=[0])

    def results(s):
        s.set_msaa_seed(3)
        out = [s.render_image(c)[0] for c in range(s.num_cameras)]
        st = [s.render_image(c)[1] for c in range(s.num_cameras)]
        hits = s.trace_rays(b.o, b.d)
        out += [hits, s.shade_rays(b.o, b.d), s.occluded(b.o, b.d, 5.0),
                s.hit_attributes(b.o, b.d, hits)]
        return out, [[getattr(x, k) for k in COUNTERS] for x in st], s.records_ok(0)

    with rt().Scene.create(desc.d) as s:
        want = results(s)
    if name != "msaa4":  # ... and the old way's frame is the oracle's
        ref, _ = OracleScene(xml).render(0, threads=4)
        assert np.array_equal(bits(want[0][0]), bits(ref))
    h = C.c_void_p()
    _lib.check(_lib.lib().rt_scene_create_textured(C.byref(desc.d), None, None, -1, C.byref(h)))
    tex = [tu.random_texture(3, 2, 1)]
    made = [rt().Scene._from_handle(h), rt().Scene.create(desc.d, textures=tex),
            rt().Scene.create(desc.d, textures=tex,
                              mesh_texture=np.full(desc.d.num_meshes, -1, np.int32),
                              triangle_texture=np.full(desc.d.num_triangles, -1, np.int32),
                              sphere_texture=np.full(desc.d.num_spheres, -1, np.int32))]
    for k, s in enumerate(made):
        with s:
            assert s.num_textures == 0 and not s.has_smooth
            got = results(s)
        assert got[1:] == want[1:], k
        for x, y in zip(got[0], want[0]):
            assert same_records(np.ascontiguousarray(x), np.ascontiguousarray(y)), k


# ---------------------------------------------------------------- refusals, queries, lifetime
def test_textured_scene_refusals_queries_and_lifetime(scene_dir):
    """A textured scene behaves to records like a scene that recurses; trace_rays and
    hit_attributes work on it and agree with the restatement's hits; twelve create / destroy
    cycles."""
    import torch
    from ceng795_amd import _lib
    xml, desc, scene = tu.mixed_scene(scene_dir)
    b, rgb, t, _, near, _ = tu.reference(scene_dir, camera=1)
    orc = OracleScene(xml)
    rec, shape = orc.intersect_rays(b.o, b.d)
    orc.close()
    stream = torch.cuda.current_stream().cuda_stream
    for cycle in range(12):
        with open_mixed(scene_dir) as s:
            assert not any(s.records_ok(c) for c in range(s.num_cameras))
            if cycle % 4 == 0:
                assert_radiance(s.shade_rays(b.o, b.d), rgb, t, near, cycle)
            if cycle:
                continue
            out = torch.zeros((s.num_tiles(1), 64), dtype=torch.float32, device="cuda")
            with pytest.raises(rt().RTError) as e:
                s.render_device(1, out.data_ptr(), tile_major=True, records=True, stream=stream)
            assert e.value.code == _lib.RT_E_UNSUPPORTED
            with pytest.raises(rt().RTError):
                s.tile_costs(stream, s.num_tiles(1))
            hits = s.trace_rays(b.o, b.d)
            assert np.array_equal(hits["object"], shape)
            assert np.array_equal(bits(hits["t"][b.hit]), bits(b.t[b.hit]))
            attr = s.hit_attributes(b.o, b.d, hits)
            tr = su.Tracer(xml, tu.MIXED_SMOOTH)
            idx = np.flatnonzero(b.hit)
            assert np.array_equal(bits(attr["shading_normal"][idx]),
                                  bits(tr.hit_normals(b.o, b.d, rec, shape, idx)))
            tr.close()
            occ = s.occluded(b.o, b.d, 1e30)
            assert np.array_equal(occ.astype(bool), b.hit)
    # only spheres textured: no uv needed
    with rt().Scene.create(desc.d, textures=scene["textures"], sphere_texture=[3]) as s:
        assert s.num_textures == 4 and not s.has_smooth
        want = tu.trace(xml, b.o, b.d, textures=scene["textures"], sphere_texture=[3])
        rad = s.shade_rays(b.o, b.d)
        assert_radiance(rad, want[0], want[1], want[3], "spheres only")


# ---------------------------------------------------------------- scene files
def test_textured_scene_file(scene_dir):
    """rt_scene_load_xml_textured of tx_mixed written with HW4's tags equals the scene made from
    the descriptors: frames, queries and the lookup."""
    path, images, scene = tu.textured_xml(scene_dir)
    b, rgb, t, counts, near, _ = tu.reference(scene_dir, camera=1)
    with rt().Scene(path, textured=True, images=images) as s, open_mixed(scene_dir) as made:
        assert s.num_textures == 4 and s.has_smooth
        for cam in range(3):
            assert FU.same_bits(s.render_image(cam)[0], made.render_image(cam)[0]), cam
        rad = s.shade_rays(b.o, b.d)
        u = np.linspace(-0.5, 1.5, 64, dtype=np.float32)
        for k in range(4):
            assert FU.same_bits(s.texture_lookup(k, u, u[::-1]), made.texture_lookup(k, u, u[::-1]))
    assert_radiance(rad, rgb, t, near, "the scene file")
    with rt().Scene(path, smooth=True) as plain:  # the other loaders ignore the tags
        assert plain.num_textures == 0
