"""Smooth shading and hit attributes on the GPU (rt_scene_create_surface, rt_scene_load_xml_surface,
rt_hit_attributes*), bit for bit against the restatement of tests/smooth_util.py
(which test_smooth_host.py pins to the CPU oracle, and which takes every hit and shadow decision
from it).  That each scene holds the cases it is for is asserted there, from the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import desc_xml
import film_util as FU
import lit_util
import rq_util
import scenes
import smooth_util as su
from oracle.cpu_ref import OracleScene
from rq_util import INF, bits, same_records, shade_device, to_device

pytestmark = pytest.mark.gpu

MODES = ["fast", "reference"]
HIT, TRIANGLE, SMOOTH = 1, 2, 4
COUNTERS = ("primary_rays", "primary_hits", "shadow_rays", "secondary_rays")


def rt():
    import ceng795_amd
    return ceng795_amd


def open_scene(name, scene_dir, traversal="fast"):
    xml, _ = su.case_xml(name, scene_dir)
    s = rt().Scene(xml, traversal=traversal, smooth=True)
    assert s.has_smooth
    return s


def frames_and_counts(s):
    """render_image of every camera as (n, 3) in ray order, and the summed ray counts."""
    total = dict.fromkeys(COUNTERS, 0)
    frames = []
    for c in range(s.num_cameras):
        img, st = s.render_image(c)
        frames.append(img.reshape(-1, 3))
        for k in COUNTERS:
            total[k] += getattr(st, k)
    return np.concatenate(frames), total


def assert_radiance(rad, rgb, t, what):
    assert np.array_equal(bits(rad["rgb"]), bits(rgb)), what
    assert np.array_equal(bits(rad["t"]), bits(t)), what


_ATTR = {}


def restated_attributes(name, scene_dir, vn=None, uv=None):
    """The scene's camera rays and what rt_trace_rays / rt_hit_attributes must give for them:
    (batch, oracle shape, HIT_ATTR_DTYPE records), computed once per (scene, normals, uv)."""
    key = (name, None if vn is None else vn.tobytes(), None if uv is None else uv.tobytes())
    if key not in _ATTR:
        xml, smooth = su.case_xml(name, scene_dir)
        b = rq_util.oracle_batch(xml)
        tr = su.Tracer(xml, smooth, vn)
        rec, shape = tr.orc.intersect_rays(b.o, b.d)
        idx = np.flatnonzero(rec[:, 7] == 1.0)
        want = np.zeros(len(b), rt().HIT_ATTR_DTYPE)
        want["geometric_normal"][idx] = rec[idx, 4:7]
        want["shading_normal"][idx] = tr.hit_normals(b.o, b.d, rec, shape, idx)
        tri = idx[tr.ob.tri[shape[idx]]]
        beta, gamma = su.barycentrics(tr.desc, b.o[tri], b.d[tri], shape[tri], rec[tri, 3], tr.ob)
        want["beta"][tri], want["gamma"][tri] = beta, gamma
        want["flags"][idx] = HIT
        want["flags"][tri] |= TRIANGLE
        want["flags"][tri[tr.ob.smooth[shape[tri]]]] |= SMOOTH
        if uv is not None:
            vi = tr.ob.idx[shape[tri]]
            want["uv"][tri] = su.interpolate(uv[vi[:, 0]], uv[vi[:, 1]], uv[vi[:, 2]], beta, gamma)
        tr.close()
        _ATTR[key] = (b, shape, want)
    return _ATTR[key]


def assert_hits(hits, b, shape, want, what):
    """rt_ray_hit records: the oracle's t and object, the restated (smooth) normal."""
    assert np.array_equal(hits["object"], shape), what
    assert np.array_equal(bits(hits["t"][b.hit]), bits(b.t[b.hit])), what
    assert (bits(hits["t"][~b.hit]) == bits(INF)).all(), what
    assert np.array_equal(bits(hits["normal"]), bits(want["shading_normal"])), what


def attributes_device(s, o, d, hits, *, n=None, pad=0, stream=None):
    """rt_hit_attributes_device over the first n rays; the output holds `pad` more slots of 0xA5
    bytes.  Returns (attr[n], the pad slots' bytes)."""
    import torch
    rays = rt().pack_rays(o, d)
    n = len(rays) if n is None else n
    dr, dh = to_device(rays), to_device(np.ascontiguousarray(hits))
    out = torch.full(((n + pad) * 48 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s.hit_attributes_device(dr.data_ptr(), dh.data_ptr(), n, out.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    raw = out.cpu().numpy()
    return raw[:n * 48].view(rt().HIT_ATTR_DTYPE).copy(), raw[n * 48:(n + pad) * 48]


# ---------------------------------------------------------------- sm_hf
@pytest.mark.parametrize("traversal", MODES)
def test_sm_hf(scene_dir, traversal):
    """Every camera's frame with its ray counts, rt_trace_rays' normals, rt_shade_rays and
    rt_hit_attributes on the smooth height field."""
    b, rgb, t, counts = su.reference("sm_hf", scene_dir)
    _, shape, want = restated_attributes("sm_hf", scene_dir)
    with open_scene("sm_hf", scene_dir, traversal) as s:
        assert not s.records_ok(0)
        frames, total = frames_and_counts(s)
        hits = s.trace_rays(b.o, b.d)
        rad, st = s.shade_rays(b.o, b.d, stats=True)
        attr = s.hit_attributes(b.o, b.d, hits)
        reordered = s.trace_rays(b.o, b.d, reorder=True)
    assert np.array_equal(bits(frames), bits(rgb))
    assert total == counts
    assert_hits(hits, b, shape, want, "sm_hf")
    assert same_records(hits, reordered)
    assert_radiance(rad, rgb, t, "sm_hf")
    assert {k: getattr(st, k) for k in COUNTERS} == counts
    assert same_records(attr, want)
    assert (attr["flags"][b.hit] == HIT | TRIANGLE | SMOOTH).all() and (attr["flags"][~b.hit] == 0).all()


# ---------------------------------------------------------------- sm_mixed
@pytest.mark.parametrize("traversal", MODES)
def test_sm_mixed(scene_dir, traversal):
    """Smooth, flat-mesh, loose-triangle and sphere hits and misses in one wave: the 17 x 9 frame
    (its first tile holds them all; the other tiles have lanes outside the image), and the first
    50 rays of that tile as a batch of their own (a wave with 14 idle lanes)."""
    b, rgb, t, counts = su.reference("sm_mixed", scene_dir)
    _, shape, want = restated_attributes("sm_mixed", scene_dir)
    tile0 = (np.arange(8)[:, None] * 17 + np.arange(8)[None, :]).reshape(-1)[:50]
    xml, smooth = su.case_xml("sm_mixed", scene_dir)
    kinds = su.hit_kinds(desc_xml.Desc(xml), shape, smooth)
    assert set(kinds[tile0]) == {"smooth", "flat", "loose", "sphere", "miss"}
    with open_scene("sm_mixed", scene_dir, traversal) as s:
        frames, total = frames_and_counts(s)
        hits = s.trace_rays(b.o, b.d)
        attr = s.hit_attributes(b.o, b.d, hits)
        rad, tail = shade_device(s, b.o[tile0], b.d[tile0], pad=64)
        few = s.trace_rays(b.o[tile0], b.d[tile0])
    assert np.array_equal(bits(frames), bits(rgb)) and total == counts
    assert_hits(hits, b, shape, want, "sm_mixed")
    assert same_records(attr, want)
    for kind, flags in (("smooth", HIT | TRIANGLE | SMOOTH), ("flat", HIT | TRIANGLE),
                        ("loose", HIT | TRIANGLE), ("sphere", HIT), ("miss", 0)):
        assert (attr["flags"][kinds == kind] == flags).all(), kind
    assert_radiance(rad, rgb[tile0], t[tile0], "sm_mixed wave 0")
    assert (tail == 0xA5).all()
    assert same_records(few, hits[tile0])


# ---------------------------------------------------------------- sm_glass
@pytest.mark.parametrize("traversal", MODES)
def test_sm_glass_frames(scene_dir, traversal):
    b, rgb, t, counts = su.reference("sm_glass", scene_dir)
    with open_scene("sm_glass", scene_dir, traversal) as s:
        frames, total = frames_and_counts(s)
        rad, st = s.shade_rays(b.o, b.d, stats=True)
    differing = int((bits(frames) != bits(rgb)).sum())
    print(f"sm_glass/{traversal}: {differing} frame channels differ from the restatement")
    assert differing == 0
    assert total == counts
    assert_radiance(rad, rgb, t, "sm_glass")
    assert {k: getattr(st, k) for k in COUNTERS} == counts


@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("medium", [False, True])
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_sm_glass_depths(scene_dir, depth, medium, traversal):
    b, rgb, t, counts = su.reference("sm_glass", scene_dir, depth, medium)
    with open_scene("sm_glass", scene_dir, traversal) as s:
        rad, st = s.shade_rays(b.o, b.d, depth=depth, in_medium=medium, stats=True)
    assert_radiance(rad, rgb, t, (depth, medium))
    got = {k: getattr(st, k) for k in COUNTERS}
    # (the library counts every first hit; the oracle's trace only those at the scene's depth)
    got["primary_hits"] = got["primary_hits"] if depth == 3 else 0
    assert got == counts, (depth, medium)


@pytest.mark.parametrize("traversal", MODES)
def test_sm_glass_independence_and_chunks(scene_dir, traversal):
    """RT_QUERY_REORDER, a permuted batch, prefixes 1 .. 257 with an untouched tail, and three
    chunks under a scratch limit give the whole batch's records."""
    b, rgb, t, _ = su.reference("sm_glass", scene_dir)
    n = len(b)
    with open_scene("sm_glass", scene_dir, traversal) as s:
        whole = s.shade_rays(b.o, b.d)
        assert_radiance(whole, rgb, t, "whole")
        perm = np.random.default_rng(795).permutation(n)
        assert same_records(s.shade_rays(b.o[perm], b.d[perm]), whole[perm])
        assert same_records(s.shade_rays(b.o, b.d, reorder=True), whole)
        assert same_records(s.shade_rays(b.o[perm], b.d[perm], reorder=True), whole[perm])
        lo = (n // 2) // 64 * 64
        part = slice(lo, lo + 300)
        assert b.hit[part].sum() >= 50 and (~b.hit[part]).sum() >= 50
        for reorder in (False, True):
            for k in (1, 63, 64, 65, 257):
                rad, tail = shade_device(s, b.o[part], b.d[part], n=k, pad=64, reorder=reorder)
                assert same_records(rad, whole[lo:lo + k]), (k, reorder)
                assert len(tail) == 64 * 16 and (tail == 0xA5).all(), (k, reorder)
        per_ray = 4 * 28 * (3 + 1)
        chunk = 384
        assert -(-n // chunk) == 3 and n % chunk != 0 and (n % chunk) % 64 != 0
        s.set_radiance_scratch_limit(chunk * per_ray)
        for reorder in (False, True):
            assert same_records(s.shade_rays(b.o, b.d, reorder=reorder), whole), reorder
        s.set_radiance_scratch_limit(0)


# ---------------------------------------------------------------- sm_single
def test_sm_single(scene_dir):
    """One smooth triangle as the root, the caller's own vertex normals (length 1.5, used as given)
    and texture coordinates through Scene.create."""
    xml, smooth = su.case_xml("sm_single", scene_dir)
    desc = desc_xml.Desc(xml)
    vn = np.array([[0.9, 0.0, 1.2], [-0.9, 0.6, 1.0392305], [0.0, -0.9, 1.2]], np.float32)
    vn = vn * (np.float32(1.5) / np.sqrt((vn * vn).sum(axis=1, dtype=np.float32)))[:, None]
    assert np.allclose(np.linalg.norm(vn, axis=1), 1.5, atol=1e-6)
    uv = np.array([[0.0, 0.0], [1.0, 0.125], [0.25, 1.0]], np.float32)
    b, shape, want = restated_attributes("sm_single", scene_dir, vn, uv)
    assert b.hit.sum() >= 50 and (~b.hit).sum() >= 50
    rgb, t, counts = su.trace(xml, b.o, b.d, smooth=smooth, vn=vn)
    unit, _, _ = su.trace(xml, b.o, b.d, smooth=smooth)
    assert (bits(rgb) != bits(unit)).any(axis=1).sum() >= 50  # the caller's normals are in use
    for traversal in MODES:
        s = rt().Scene.create(desc.d, mesh_smooth=[1], vertex_normals=vn, vertex_uv=uv)
        with s:
            s.set_traversal(traversal)
            assert s.has_smooth and s.bvh_depth == 0
            frames, total = frames_and_counts(s)
            hits = s.trace_rays(b.o, b.d)
            attr = s.hit_attributes(b.o, b.d, hits)
        assert np.array_equal(bits(frames), bits(rgb)) and total == counts, traversal
        assert_hits(hits, b, shape, want, traversal)
        assert same_records(attr, want), traversal
    assert (want["uv"][b.hit] != 0).any(axis=1).sum() >= 50
    # uv without a smooth mesh: the flat scene's results, and the same uv
    with rt().Scene.create(desc.d, vertex_uv=uv) as s, rt().Scene(xml) as plain:
        assert not s.has_smooth
        assert np.array_equal(bits(s.render_image(0)[0]), bits(plain.render_image(0)[0]))
        hits = s.trace_rays(b.o, b.d)
        assert same_records(hits, plain.trace_rays(b.o, b.d))
        attr = s.hit_attributes(b.o, b.d, hits)
    assert np.array_equal(bits(attr["uv"]), bits(want["uv"]))
    assert np.array_equal(bits(attr["shading_normal"]), bits(want["geometric_normal"]))
    assert (attr["flags"][b.hit] == HIT | TRIANGLE).all()


# ---------------------------------------------------------------- sm_deep
def test_sm_deep(scene_dir):
    """A tree deeper than the per-lane stack: the DEEP instantiations with SMOOTH."""
    b, rgb, t, counts = su.reference("sm_deep", scene_dir)
    _, shape, want = restated_attributes("sm_deep", scene_dir)
    assert b.hit.sum() >= 100 and (~b.hit).sum() >= 100
    assert np.isfinite(want["shading_normal"]).all()
    for traversal in MODES:
        with open_scene("sm_deep", scene_dir, traversal) as s:
            assert s.bvh_depth > 64
            frames, total = frames_and_counts(s)
            hits = s.trace_rays(b.o, b.d)
            rad = s.shade_rays(b.o, b.d)
        assert np.array_equal(bits(frames), bits(rgb)) and total == counts, traversal
        assert_hits(hits, b, shape, want, traversal)
        assert_radiance(rad, rgb, t, traversal)


# ---------------------------------------------------------------- sm_msaa
_MSAA = {}  # the samples and the restated film, computed once


@pytest.mark.parametrize("traversal", MODES)
def test_sm_msaa(scene_dir, traversal):
    """NumSamples 4 at 16 x 16: the MSAA frame and a Gaussian film of the same samples against the
    film restatement fed by `trace`."""
    xml, smooth = su.case_xml("sm_msaa", scene_dir)
    seed = 5
    if xml not in _MSAA:
        o, d, xy, (w, h, S) = FU.msaa_samples(xml, 0, seed)
        assert (w, h, S) == (16, 16, 4)
        rgb, _, counts = su.trace(xml, o, d, smooth=smooth)
        acc = FU.new_film(w, h)
        FU.splat(acc, xy, rgb)
        flat, _ = OracleScene(xml).render_msaa(0, seed=seed, threads=4)
        assert (bits(FU.resolve(acc)) != bits(flat)).sum() >= 100
        _MSAA[xml] = (o, d, xy, w, h, counts, acc)
    o, d, xy, w, h, counts, acc = _MSAA[xml]
    want = FU.resolve(acc)
    with open_scene("sm_msaa", scene_dir, traversal) as s:
        s.set_msaa_seed(seed)
        frame, st = s.render_image(0)
        with rt().Film(s, w, h) as film:
            film.shade_rays(o, d, xy)
            got = film.resolve()
            assert FU.same_bits(film.accumulators(), acc)
    assert FU.same_bits(frame, want), "the MSAA frame"
    assert FU.same_bits(got, want), "the Gaussian film"
    assert {k: getattr(st, k) for k in COUNTERS} == counts


# ---------------------------------------------------------------- lit queries
_LIT = {}  # the lit query's records and the restated answer, computed once


@pytest.mark.parametrize("traversal", MODES)
def test_lit_query(scene_dir, traversal):
    """One lit query with per-ray records on sm_hf: the scene's lights dark, each ray's own point
    light and emitter sample, against lit_util.restate with the smooth normals in place of the
    oracle's (smooth_util.restate_lit)."""
    xml, smooth = su.case_xml("sm_hf", scene_dir)
    if xml not in _LIT:
        b = rq_util.oracle_batch(xml, cameras=[0])
        n = len(b)
        rng = np.random.default_rng(3)
        pos = np.stack([lit_util.eighths(rng, -3, 3, n), lit_util.eighths(rng, 1, 4, n),
                        lit_util.eighths(rng, -8, -2, n)], axis=1)
        own = np.zeros((n, 2), rt().LIGHT_SAMPLE_DTYPE)
        own["position"][:, 0], own["intensity"][:, 0] = pos, (400, 300, 200)
        own["position"][:, 1], own["intensity"][:, 1] = pos[::-1], (100, 200, 300)
        own["normal"][:, 1] = (0, -1, 0)
        want, shadow = su.restate_lit(xml, b.o, b.d, own, smooth)
        flat, _ = lit_util.restate(xml, b.o, b.d, own)
        assert (bits(want[:, :3]) != bits(flat[:, :3])).sum() >= 100
        _LIT[xml] = (b, own, want, shadow)
    b, own, want, shadow = _LIT[xml]
    with open_scene("sm_hf", scene_dir, traversal) as s:
        rad, st = s.shade_rays_lit(b.o, b.d, own, scene_lights=False, stats=True)
    assert np.array_equal(bits(rad["rgb"]), bits(want[:, :3]))
    assert np.array_equal(bits(rad["t"]), bits(want[:, 3]))
    assert st.shadow_rays == shadow == 2 * b.hit.sum()


# ---------------------------------------------------------------- hit attributes
def bad_lanes(hits, o, d, leaves):
    """Lanes 0 and 63 of the first two waves and lanes around them: leaf -1, `leaves`, INT_MAX and
    INT_MIN, and invalid rays.  Returns the lanes changed."""
    hits["leaf"][0], hits["leaf"][63] = -1, leaves
    hits["leaf"][64], hits["leaf"][127] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    d[1], d[62], d[65] = (np.nan, 0, 1), (np.inf, 0, 0), (1e-7, -1e-7, 9e-7)
    o[126], d[128] = (0, np.inf, 0), (0, 0, 0)
    return [0, 63, 64, 127, 1, 62, 65, 126, 128]


@pytest.mark.parametrize("name", ["soup1", "single_sphere"])
def test_hit_attributes_on_flat_scenes(scene_dir, name):
    """On scenes made by the plain creator: beta and gamma of the oracle's hits, both normals the
    hit record's, spheres by their t (single_sphere: negative roots); out-of-range leaves and
    invalid rays give all-zero records and leave their neighbours alone; n = 0; host = device;
    two streams."""
    import torch
    xml = rq_util.write_rigged(name, scene_dir)
    b = rq_util.oracle_batch(xml)
    desc = desc_xml.Desc(xml)
    orc = OracleScene(xml)
    rec, shape = orc.intersect_rays(b.o, b.d)
    orc.close()
    ob = su.Objects(desc)
    tri = np.flatnonzero((shape >= 0) & ob.tri[np.where(shape >= 0, shape, 0)])
    sph = np.flatnonzero((shape >= 0) & ~ob.tri[np.where(shape >= 0, shape, 0)])
    if name == "single_sphere":
        assert len(tri) == 0 and (b.t[sph] < 0).sum() >= 50
    else:
        assert len(tri) >= 1000 and len(sph) >= 100
    want = np.zeros(len(b), rt().HIT_ATTR_DTYPE)
    want["shading_normal"][b.hit] = want["geometric_normal"][b.hit] = b.normal[b.hit]
    want["flags"][b.hit] = HIT
    want["flags"][tri] |= TRIANGLE
    if len(tri):
        want["beta"][tri], want["gamma"][tri] = su.barycentrics(desc, b.o[tri], b.d[tri], shape[tri],
                                                                rec[tri, 3], ob)
    leaves = len(rq_util.object_list(desc))
    with rt().Scene(xml) as s:
        hits = s.trace_rays(b.o, b.d)
        attr = s.hit_attributes(b.o, b.d, hits)
        assert same_records(attr, want)
        dev, tail = attributes_device(s, b.o, b.d, hits, pad=64)
        assert same_records(dev, attr) and (tail == 0xA5).all()
        # n = 0 launches nothing; a prefix leaves the tail untouched
        none, tail = attributes_device(s, b.o, b.d, hits, n=0, pad=4)
        assert len(none) == 0 and (tail == 0xA5).all()
        part, tail = attributes_device(s, b.o, b.d, hits, n=65, pad=64)
        assert same_records(part, attr[:65]) and (tail == 0xA5).all()
        assert len(s.hit_attributes(b.o[:0], b.d[:0], hits[:0])) == 0
        # records that point nowhere, rays that are no rays
        lo = int(np.flatnonzero(b.hit)[0]) // 64 * 64
        h2, o2, d2 = hits[lo:lo + 256].copy(), b.o[lo:lo + 256].copy(), b.d[lo:lo + 256].copy()
        bad = bad_lanes(h2, o2, d2, leaves)
        got = s.hit_attributes(o2, d2, h2)
        dev, _ = attributes_device(s, o2, d2, h2)
        good = np.ones(256, bool)
        good[bad] = False
        assert (got[bad].view(np.uint8) == 0).all()
        assert same_records(got[good], attr[lo:lo + 256][good]) and same_records(dev, got)
        # two streams
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a1, _ = attributes_device(s, b.o, b.d, hits, stream=s1)
        a2, _ = attributes_device(s, b.o[::-1], b.d[::-1], hits[::-1], stream=s2)
        assert same_records(a1, attr) and same_records(a2, np.ascontiguousarray(attr[::-1]))


# ---------------------------------------------------------------- flat scenes and refusals
@pytest.mark.parametrize("name", ["soup1", "soup_depth3", "msaa4"])
def test_flat_scenes_are_unchanged(scene_dir, name):
    """A flat scene through rt_scene_create_surface(NULL surface), through a surface without a
    smooth mesh or uv, and through rt_scene_load_xml_surface: every frame and query equals the
    plain creators' results byte for byte."""
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

    with rt().Scene(xml) as s:
        want = results(s)
    h = C.c_void_p()
    _lib.check(_lib.lib().rt_scene_create_surface(C.byref(desc.d), None, -1, C.byref(h)))
    made = [rt().Scene._from_handle(h), rt().Scene.create(desc.d),
            rt().Scene.create(desc.d, mesh_smooth=np.zeros(desc.d.num_meshes, np.uint8)),
            rt().Scene(xml, smooth=True)]
    for k, s in enumerate(made):
        with s:
            assert not s.has_smooth
            got = results(s)
        assert got[1:] == want[1:], k
        for x, y in zip(got[0], want[0]):
            assert same_records(np.ascontiguousarray(x), np.ascontiguousarray(y)), k


def test_smooth_scene_refusals_and_lifetime(scene_dir):
    """A smooth scene behaves to records and tile costs like a scene that recurses; there is no
    multi-device smooth scene; twelve create / destroy cycles."""
    import torch
    from ceng795_amd import _lib
    xml, _ = su.case_xml("sm_hf", scene_dir)
    b, rgb, _, _ = su.reference("sm_hf", scene_dir)
    cam0 = b.cam == 0
    stream = torch.cuda.current_stream().cuda_stream
    for cycle in range(12):
        with rt().Scene(xml, smooth=True) as s:
            assert s.has_smooth and not any(s.records_ok(c) for c in range(s.num_cameras))
            if cycle % 4 == 0:
                assert np.array_equal(bits(s.render_image(0)[0].reshape(-1, 3)), bits(rgb[cam0]))
            if cycle:
                continue
            out = torch.zeros((s.num_tiles(0), 64), dtype=torch.float32, device="cuda")
            with pytest.raises(rt().RTError):
                s.render_device(0, out.data_ptr(), tile_major=True, records=True, stream=stream)
            frame = torch.zeros((24, 24, 3), dtype=torch.float32, device="cuda")
            s.render_device(0, frame.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            assert np.array_equal(bits(frame.cpu().numpy().reshape(-1, 3)), bits(rgb[cam0]))
            with pytest.raises(rt().RTError):  # as a scene that recurses: no ordered frame
                s.tile_costs(stream, s.num_tiles(0))
    with pytest.raises(rt().RTError) as e:
        rt().Scene(xml, devices=[0, 0], smooth=True)
    assert e.value.code == _lib.RT_E_UNSUPPORTED
    with rt().Scene(xml, devices=[0, 0]) as multi:  # the plain multi-device scene: flat, refused
        assert not multi.has_smooth
        hits = np.zeros(4, rt().HIT_DTYPE)
        with pytest.raises(rt().RTError) as e:
            multi.hit_attributes(b.o[:4], b.d[:4], hits)
        assert e.value.code == _lib.RT_E_UNSUPPORTED
