"""Light samples on the GPU (rt_shade_rays_lit*, rt_film_shade_rays_lit*).

Point records are judged by the CPU oracle: ray i's result must be OracleScene.shade_rays on a
variant of the scene whose light list is L_i (tools/gen_scene.py's SceneSpec with `lights`
replaced; every light coordinate and intensity a multiple of 1/8 below 1024, so the variant's
text parses to exactly the fp32 the test uploads — lit_util.write_with_lights reads it back).
Per-ray lists come in G distinct sets, ray i using set i % G: every wave holds all G sets in
neighbouring lanes, and the rays of a set are compared with that set's variant.  Emitter records
are judged by lit_util.restate (tests/test_lit_query_host.py pins it to the oracle).

All comparisons are bit for bit on rgb and t, and the host variant's rt_stats equal the oracle's
Stats summed over the sets.  (The oracle counts primary_hits only for rays traced at the scene's
MaxRecursionDepth, the library for every query's first rays: below the maximum that one field is
left out.)"""
import functools

import numpy as np
import pytest

import desc_xml
import film_util
import lit_util
import rq_util
import scenes
from lit_util import NAN, eighths, records, shade_lit_device
from oracle.cpu_ref import OracleScene
from rq_util import INF, bits

pytestmark = pytest.mark.gpu

MODES = ["fast", "reference"]
COUNTS = ("primary_rays", "primary_hits", "shadow_rays", "secondary_rays")


# ---------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def batch_of(xml, cameras=(0,)):
    b = rq_util.oracle_batch(xml, cameras=None if cameras is None else list(cameras))
    for a in (b.o, b.d, b.t, b.hit):
        a.setflags(write=False)
    return b


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                          np.ascontiguousarray(b).view(np.uint8))


def scene_batch(name, xml):
    """Camera 0's pixel rays; for the lone sphere every camera's, the rig's included: the one
    that looks away from the sphere hits it with a negative root."""
    if name != "single_sphere":
        return batch_of(xml)
    b = batch_of(xml, None)
    assert (b.hit & (b.t < 0)).sum() >= 50
    return b


def add_rig(spec):
    spec.cameras = list(spec.cameras) + rq_util.rig(rq_util.RIG_AT["single_sphere"])


def base_xml(name, directory):
    """The scene the GPU loads: the catalogue scene with its own lights (the lone sphere with
    rq_util's camera rig)."""
    return lit_util.write_with_lights(name, directory, "own", lit_util.spec_lights(name),
                                      add_rig if name == "single_sphere" else None)


def light_box(name):
    """Where the test's lights go: around the scene's own first light."""
    p = lit_util.spec_lights(name)[0][0]
    c = np.round(p.astype(np.float64) * 8) / 8
    return c - 2.0, c + 2.0


def draw_lights(name, rng, count):
    lo, hi = light_box(name)
    pos = np.stack([eighths(rng, lo[a], hi[a], count) for a in range(3)], axis=1)
    inten = eighths(rng, 100, 900, (count, 3))
    return [(pos[k], inten[k]) for k in range(count)]


def oracle_sets(name, directory, tag, lists, o, d, depth=-1, in_medium=False, change=None):
    """Ray i against the variant whose light list is lists[i % G]: ((n, 4), summed stats)."""
    G = len(lists)
    want = np.zeros((len(o), 4), np.float32)
    total = dict.fromkeys(COUNTS, 0)
    for g, L in enumerate(lists):
        xml = lit_util.write_with_lights(name, directory, f"{tag}{g}", L, change)
        idx = np.arange(g, len(o), G)
        orc = OracleScene(xml)
        out, st = orc.shade_rays(o[idx], d[idx], depth, in_medium)
        orc.close()
        want[idx] = out
        for k in COUNTS:
            total[k] += getattr(st, k)
    return want, total


def set_records(sets, n, k, seed=0):
    """(n, k) records: ray i holds the lights of sets[i % G] in their order, at slots that vary
    from set to set; the other slots are inactive (a NaN position, in a component that varies,
    in front of a loud intensity)."""
    G = len(sets)
    rng = np.random.default_rng(seed)
    rec = records(np.zeros((n, k, 3)), np.full((n, k, 3), 99999.0))
    nan_at = np.arange(n * k).reshape(n, k) % 3
    pos = np.zeros((n, k, 3), np.float32)
    np.put_along_axis(pos, nan_at[..., None], NAN, axis=2)
    pos[::5][np.arange(len(pos[::5])) % 2 == 0] = np.inf  # (an infinite one is inactive too)
    rec["position"] = pos
    for g, L in enumerate(sets):
        slots = np.sort(rng.choice(k, len(L), replace=False))
        for s, (p, i) in zip(slots, L):
            rec["position"][g::G, s] = p
            rec["intensity"][g::G, s] = i
    return rec


def assert_same(rad, want, what):
    diff = int((bits(rad["rgb"]) != bits(want[:, :3])).sum())
    tdiff = int((bits(rad["t"]) != bits(want[:, 3])).sum())
    print(f"{what}: {len(want)} rays, {diff} channels and {tdiff} t differ in bits")
    assert diff == 0 and tdiff == 0, what


def assert_counts(st, total, what, at_max=True):
    for k in COUNTS:
        if k == "primary_hits" and not at_max:
            continue
        assert getattr(st, k) == total[k], (what, k, getattr(st, k), total[k])


# ---------------------------------------------------------------- 1. shared lists
def test_shared_lists(scene_dir):
    import ceng795_amd
    name = "soup1"
    xml = base_xml(name, scene_dir)
    b = batch_of(xml)
    assert len(b) == 96 * 96 and b.hit.sum() >= 1000 and (~b.hit).sum() >= 1000
    own = lit_util.spec_lights(name)
    assert len(own) == 4
    extra = draw_lights(name, np.random.default_rng(41), 2)
    own_rec = records([p for p, _ in own], [i for _, i in own])
    extra_rec = records([p for p, _ in extra], [i for _, i in extra])
    six, six_counts = oracle_sets(name, scene_dir, "six", [own + extra], b.o, b.d)
    first, first_counts = oracle_sets(name, scene_dir, "xfirst", [extra + own], b.o, b.d)
    assert (bits(six[:, :3]) != bits(first[:, :3])).sum() >= 100  # the order shows in the bits
    with ceng795_amd.Scene(xml) as s:
        plain = s.shade_rays(b.o, b.d)
        assert same_bytes(s.shade_rays_lit(b.o, b.d, own_rec, shared=True, scene_lights=False), plain)
        rad, st = s.shade_rays_lit(b.o, b.d, extra_rec, shared=True, stats=True)
        assert_same(rad, six, "scene + 2 shared")
        assert_counts(st, six_counts, "scene + 2 shared")
        rad2, st2 = s.shade_rays_lit(b.o, b.d, np.concatenate([extra_rec, own_rec]), shared=True,
                                     scene_lights=False, stats=True)
        assert_same(rad2, first, "2 shared first")
        assert_counts(st2, first_counts, "2 shared first")
        assert (bits(rad["rgb"]) != bits(rad2["rgb"])).sum() >= 100
        dev, tail = shade_lit_device(s, b.o, b.d, extra_rec, shared=True, pad=64, reorder=True)
        assert same_bytes(dev, rad) and (tail == 0xA5).all()


# ---------------------------------------------------------------- 2. per-ray lists
@pytest.mark.parametrize("name", ["soup1", "hf_small", "single_sphere"])
def test_per_ray_lists(scene_dir, name):
    """k = 3, G = 8: set g has g % 4 active records, the rest NaN at varying slots."""
    import ceng795_amd
    K, G = 3, 8
    xml = base_xml(name, scene_dir)
    b = scene_batch(name, xml)
    assert b.hit.sum() >= 500
    rng = np.random.default_rng(42)
    sets = [draw_lights(name, rng, g % 4) for g in range(G)]
    rec = set_records(sets, len(b), K)
    assert [int(np.isfinite(rec["position"][g]).all(axis=1).sum()) for g in range(G)] == \
        [g % 4 for g in range(G)]
    own = lit_util.spec_lights(name)
    ambient = np.array(list(desc_xml.Desc(xml).d.ambient_light), np.float32)
    with ceng795_amd.Scene(xml) as s:
        for scene_lights in (True, False):
            lists = [(own if scene_lights else []) + L for L in sets]
            want, counts = oracle_sets(name, scene_dir, f"k3{'s' if scene_lights else 'n'}", lists,
                                       b.o, b.d)
            what = f"{name}/scene_lights={scene_lights}"
            rad, st = s.shade_rays_lit(b.o, b.d, rec, scene_lights=scene_lights, stats=True)
            assert_same(rad, want, what)
            assert_counts(st, counts, what)
            assert same_bytes(s.shade_rays_lit(b.o, b.d, rec, scene_lights=scene_lights,
                                               reorder=True), rad), what
            if not scene_lights:  # no active record and no scene light: ambient only on hits
                dark = np.zeros(len(b), bool)
                dark[0::G] = dark[4::G] = True
                dark &= b.hit
                assert dark.sum() >= 100
                desc = desc_xml.Desc(xml)
                hits = s.trace_rays(b.o, b.d)
                ka = np.array([list(desc.mats[m].ambient) for m in range(desc.d.num_materials)],
                              np.float32)[hits["material"][dark]]
                assert np.array_equal(bits(rad["rgb"][dark]), bits(np.float32(0) + ka * ambient))


# ---------------------------------------------------------------- 3. recursion
def recursion_case(name, scene_dir):
    K, G = 2, 4
    xml = base_xml(name, scene_dir)
    b = batch_of(xml, None)
    rng = np.random.default_rng(43)
    sets = [draw_lights(name, rng, 1 + g % 2) for g in range(G)]
    rec = set_records(sets, len(b), K, seed=3)
    lists = [lit_util.spec_lights(name) + L for L in sets]
    return xml, b, rec, lists


@functools.lru_cache(maxsize=None)
def recursion_oracle(name, scene_dir, depth, in_medium):
    _, b, _, lists = recursion_case(name, scene_dir)
    return oracle_sets(name, scene_dir, "k2", lists, b.o, b.d, depth, in_medium)


@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("name", ["soup_depth3", "soup_depth6"])
def test_recursion_depths(scene_dir, name, traversal):
    """The whole ray tree uses L_i: depth 0, 1 and the maximum, with and without
    RT_QUERY_IN_MEDIUM, in both traversals."""
    import ceng795_amd
    xml, b, rec, _ = recursion_case(name, scene_dir)
    D = desc_xml.Desc(xml).d.max_recursion_depth
    assert D in (3, 6) and b.hit.sum() >= 1000 and (~b.hit).sum() >= 1000
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        for depth in (0, 1, D):
            for in_medium in (False, True):
                want, counts = recursion_oracle(name, scene_dir, depth, in_medium)
                what = f"{name}/{traversal}/depth{depth}/medium{in_medium}"
                rad, st = s.shade_rays_lit(b.o, b.d, rec, depth=depth, in_medium=in_medium,
                                           stats=True)
                assert_same(rad, want, what)
                assert_counts(st, counts, what, at_max=depth == D)
                if depth == D and not in_medium:
                    assert counts["secondary_rays"] >= 100
                    plain = s.shade_rays(b.o, b.d)
                    assert (bits(plain["rgb"]) != bits(rad["rgb"])).any(axis=1).sum() >= 1000


@pytest.mark.parametrize("name", ["soup_depth3", "soup_depth6"])
def test_recursion_independence(scene_dir, name):
    """Where a light index taken from the chunk or the sorted order would show: reorder, a
    permuted batch, prefixes with an untouched tail, and chunks under the scratch limit."""
    import ceng795_amd
    xml, b, rec, _ = recursion_case(name, scene_dir)
    D = desc_xml.Desc(xml).d.max_recursion_depth
    want, _ = recursion_oracle(name, scene_dir, D, False)
    n = len(b)
    with ceng795_amd.Scene(xml) as s:
        whole = s.shade_rays_lit(b.o, b.d, rec)
        assert_same(whole, want, name)
        assert same_bytes(s.shade_rays_lit(b.o, b.d, rec, reorder=True), whole)
        perm = np.random.default_rng(799).permutation(n)
        assert same_bytes(s.shade_rays_lit(b.o[perm], b.d[perm], rec[perm]), whole[perm])
        assert same_bytes(s.shade_rays_lit(b.o[perm], b.d[perm], rec[perm], reorder=True),
                          whole[perm])
        # the lights permuted differently from the rays are other lights: the index matters
        assert not same_bytes(s.shade_rays_lit(b.o[perm], b.d[perm], rec), whole[perm])
        lo = (n // 6) // 64 * 64
        part = slice(lo, lo + 300)
        assert b.hit[part].sum() >= 50 and (~b.hit[part]).sum() >= 50
        for reorder in (False, True):
            for k in (1, 63, 64, 65, 257):
                rad, tail = shade_lit_device(s, b.o[part], b.d[part], rec[part], n=k, pad=64,
                                             reorder=reorder)
                assert same_bytes(rad, whole[lo:lo + k]), (k, reorder)
                assert len(tail) == 64 * 16 and (tail == 0xA5).all(), (k, reorder)
        # three chunks with a partial last one
        m = min(n, 5700)
        per_ray = 4 * 28 * (D + 1)
        limit = 2048 * per_ray
        chunk = limit // per_ray // 64 * 64
        assert -(-m // chunk) >= 3 and (m % chunk) % 64 != 0
        s.set_radiance_scratch_limit(limit)
        for reorder in (False, True):
            assert same_bytes(s.shade_rays_lit(b.o[:m], b.d[:m], rec[:m], reorder=reorder),
                              whole[:m]), reorder
            rad, tail = shade_lit_device(s, b.o[:m], b.d[:m], rec[:m], pad=64, reorder=reorder)
            assert same_bytes(rad, whole[:m]) and (tail == 0xA5).all(), reorder
        s.set_radiance_scratch_limit(0)


# ---------------------------------------------------------------- 4. a tree deeper than 64
def mirror_floor(spec):
    spec.max_depth = 2
    spec.materials[0].mirror = (0.5, 0.4, 0.3)


@pytest.mark.parametrize("variant", ["flat", "mirror"])
def test_deep_tree(scene_dir, variant):
    """rq_util.deep_scene (99 levels: the LDS spill stack of the DEEP variants), per-ray lists."""
    import ceng795_amd
    K, G = 2, 4
    change = mirror_floor if variant == "mirror" else None
    own = lit_util.spec_lights("deep")
    xml = lit_util.write_with_lights("deep", scene_dir, f"own_{variant}", own, change)
    b = batch_of(xml)
    assert b.hit.sum() >= 100 and (~b.hit).sum() >= 1
    rng = np.random.default_rng(44)
    sets = [draw_lights("deep", rng, 1 + g % 2) for g in range(G)]
    rec = set_records(sets, len(b), K, seed=4)
    want, counts = oracle_sets("deep", scene_dir, f"k2_{variant}", [own + L for L in sets],
                               b.o, b.d, change=change)
    for traversal in MODES:
        with ceng795_amd.Scene(xml, traversal=traversal) as s:
            assert s.bvh_depth > 64
            rad, st = s.shade_rays_lit(b.o, b.d, rec, stats=True)
        assert_same(rad, want, f"deep/{variant}/{traversal}")
        assert_counts(st, counts, f"deep/{variant}/{traversal}")


# ---------------------------------------------------------------- 5. the emitter term
EMITTER = {"soup1": ((0.0, 3.5, -4.0), 1.0), "single_sphere": ((0.0, 2.5, -3.0), 1.0)}


def emitter_samples(name, n, seed, normal=(0.0, -1.0, 0.0)):
    """One point per ray on a square in the plane y = const above the scene."""
    (cx, cy, cz), half = EMITTER[name]
    rng = np.random.default_rng(seed)
    u = rng.uniform(-half, half, (n, 2)).astype(np.float32)
    pos = np.stack([np.float32(cx) + u[:, 0], np.full(n, cy, np.float32),
                    np.float32(cz) + u[:, 1]], axis=1)
    return records(pos[:, None, :], np.full((n, 1, 3), 900.0), np.broadcast_to(
        np.array(normal, np.float32), (n, 1, 3)))


@pytest.mark.parametrize("name", ["soup1", "single_sphere"])
def test_emitter_term(scene_dir, name):
    """Depth 0 against the restatement: the scene's lights, then one sample of a square emitter
    per ray; the same records as point lights and with the normal flipped."""
    import ceng795_amd
    xml = base_xml(name, scene_dir)
    desc = desc_xml.Desc(xml)
    assert desc.d.max_recursion_depth == 0
    b = scene_batch(name, xml)
    n = len(b)
    own = np.broadcast_to(lit_util.scene_records(desc)[None, :], (n, desc.d.num_lights))
    # 1.5: the normal is used as given, not normalised
    cases = {"emitter": emitter_samples(name, n, 45), "long": emitter_samples(name, n, 45, (0, -1.5, 0)),
             "point": emitter_samples(name, n, 45, (0, 0, 0)),
             "flipped": emitter_samples(name, n, 45, (0, 1, 0))}
    cases["point"]["normal"][1::2] = -0.0  # -0 is a point light too
    got = {}
    with ceng795_amd.Scene(xml) as s:
        for tag, rec in cases.items():
            for scene_lights in (True, False):
                full = np.concatenate([own, rec], axis=1) if scene_lights else rec
                want, shadow = lit_util.restate(xml, b.o, b.d, full)
                rad, st = s.shade_rays_lit(b.o, b.d, rec, depth=0, scene_lights=scene_lights,
                                           stats=True)
                what = f"{name}/{tag}/scene_lights={scene_lights}"
                assert_same(rad, want, what)
                assert st.shadow_rays == shadow and st.primary_rays == n and \
                    st.primary_hits == b.hit.sum() and st.secondary_rays == 0, what
                got[tag, scene_lights] = rad
        ambient_only = s.shade_rays_lit(b.o, b.d, cases["emitter"][:, :0], scene_lights=False)
        dev, _ = shade_lit_device(s, b.o, b.d, cases["emitter"], depth=0, reorder=True)
        assert same_bytes(dev, got["emitter", True])
    for other in ("point", "flipped", "long"):
        assert (bits(got["emitter", True]["rgb"]) != bits(got[other, True]["rgb"])).sum() >= 100, other
    # seen from behind, the emitter subtracts light: no clamp
    below = (got["flipped", False]["rgb"] < ambient_only["rgb"]).any(axis=1) & b.hit
    assert below.sum() >= 100
    assert (bits(got["flipped", False]["t"]) == bits(ambient_only["t"])).all()


# ---------------------------------------------------------------- 6. films
def test_film(scene_dir):
    """Film.shade_rays_lit = Scene.shade_rays_lit + Film.splat: 24 x 24 Gaussian film, 4 samples
    per pixel, each with its own emitter sample; samples of invalid rays are dropped and counted."""
    import ceng795_amd
    name = "soup1"
    xml = base_xml(name, scene_dir)
    cam = film_util.camera(xml, 0)
    W = H = 24
    S = 4
    rng = np.random.default_rng(46)
    i = np.tile(np.repeat(np.arange(W, dtype=np.float32), S), H)
    j = np.repeat(np.arange(H, dtype=np.float32), W * S)
    xy = np.stack([i, j], axis=1) + rng.uniform(0, 1, (W * H * S, 2)).astype(np.float32)
    xy = np.minimum(xy, np.nextafter(np.float32(W), np.float32(0))).astype(np.float32)
    scale = np.float32(cam[4] / W)
    o, d = film_util.rays_through(cam, xy[:, 0] * scale, xy[:, 1] * scale)
    n = len(o)
    bad = np.array([0, 63, 64, 1000, n - 1])
    d[bad[:3]] = np.nan
    o[bad[3:]] = np.inf
    rec = emitter_samples(name, n, 47)
    with ceng795_amd.Scene(xml) as s:
        rad, st = s.shade_rays_lit(o, d, rec, stats=True)
        good = np.ones(n, bool)
        good[bad] = False
        assert (bits(rad["rgb"][bad]) == 0).all() and (bits(rad["t"][bad]) == bits(INF)).all()
        assert (rad["rgb"][good] != 0).any(axis=1).sum() >= 1000
        plain = s.shade_rays(o, d)
        assert (bits(plain["rgb"]) != bits(rad["rgb"])).any(axis=1).sum() >= 100
        with ceng795_amd.Film(s, W, H) as two, ceng795_amd.Film(s, W, H) as fused:
            two.splat(xy[good], rad[good])
            fst = fused.shade_rays_lit(o, d, xy, rec, stats=True)
            assert fused.counts() == (n - len(bad), len(bad)) and two.counts() == (n - len(bad), 0)
            assert same_bytes(fused.accumulators(), two.accumulators())
            assert same_bytes(fused.resolve(), two.resolve())
            assert (fused.accumulators()[..., 3] > 0).all()
            for k in COUNTS:
                assert getattr(fst, k) == getattr(st, k), k
            # the device entry on a stream of its own, reordered, into a cleared film
            import torch
            stream = torch.cuda.Stream()
            dr = rq_util.to_device(ceng795_amd.pack_rays(o, d))
            dxy = rq_util.to_device(xy)
            dl = rq_util.to_device(rec)
            torch.cuda.synchronize()
            fused.clear_device(stream=stream.cuda_stream)
            fused.shade_rays_lit_device(dr.data_ptr(), dxy.data_ptr(), n, dl.data_ptr(), 1,
                                        reorder=True, stream=stream.cuda_stream)
            stream.synchronize()
            assert same_bytes(fused.accumulators(), two.accumulators())
            s.release_stream(stream.cuda_stream)


# ---------------------------------------------------------------- 7. remaining plumbing
def test_plumbing(scene_dir):
    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    name = "soup_depth3"
    xml, b, rec, _ = recursion_case(name, scene_dir)
    n = len(b)
    half = n // 2
    none = rec[:, :0]
    with ceng795_amd.Scene(xml) as s:
        plain, pst = s.shade_rays(b.o, b.d, stats=True)
        # k == 0 is rt_shade_rays bit for bit
        zero, zst = s.shade_rays_lit(b.o, b.d, none, stats=True)
        assert same_bytes(zero, plain)
        for k in COUNTS:
            assert getattr(zst, k) == getattr(pst, k), k
        assert same_bytes(s.shade_rays_lit(b.o, b.d, rec[0, :0], shared=True), plain)
        dev0, _ = shade_lit_device(s, b.o, b.d, none, reorder=True)
        assert same_bytes(dev0, plain)
        whole, wst = s.shade_rays_lit(b.o, b.d, rec, stats=True)
        # the device entries on streams of their own, a frame between two calls on one of them
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r1 = rq_util.to_device(ceng795_amd.pack_rays(b.o[:half], b.d[:half]))
        r2 = rq_util.to_device(ceng795_amd.pack_rays(b.o[half:], b.d[half:]))
        l1 = rq_util.to_device(rec[:half])
        l2 = rq_util.to_device(rec[half:])
        o1 = torch.zeros(half * 16, dtype=torch.uint8, device="cuda")
        o1b = torch.zeros(half * 16, dtype=torch.uint8, device="cuda")
        o2 = torch.zeros((n - half) * 16, dtype=torch.uint8, device="cuda")
        c = s.camera(0)
        frame = torch.zeros((c.height, c.width, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        want_frame = s.render_image(0)[0]
        s.collect_stats()
        K = rec.shape[1]
        s.shade_rays_lit_device(r1.data_ptr(), half, l1.data_ptr(), K, o1.data_ptr(), reorder=True,
                                stream=s1.cuda_stream)
        s.shade_rays_lit_device(r2.data_ptr(), n - half, l2.data_ptr(), K, o2.data_ptr(),
                                stream=s2.cuda_stream)
        s.render_device(0, frame.data_ptr(), stream=s1.cuda_stream)
        s.shade_rays_lit_device(r1.data_ptr(), half, l1.data_ptr(), K, o1b.data_ptr(),
                                stream=s1.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        dt = ceng795_amd.RADIANCE_DTYPE
        assert same_bytes(o1.cpu().numpy().view(dt), whole[:half])
        assert same_bytes(o1b.cpu().numpy().view(dt), whole[:half])
        assert same_bytes(o2.cpu().numpy().view(dt), whole[half:])
        assert same_bytes(frame.cpu().numpy(), want_frame)
        st = s.collect_stats()
        cam0 = int((b.cam == 0).sum())
        assert st.primary_rays == wst.primary_rays + half + cam0
        # scratch released and reused
        assert s.stream_frame_scratch_bytes(s1.cuda_stream) > 0
        s.release_stream(s1.cuda_stream)
        assert s.stream_frame_scratch_bytes(s1.cuda_stream) == 0
        again, _ = shade_lit_device(s, b.o[:half], b.d[:half], rec[:half], stream=s1, reorder=True)
        assert same_bytes(again, whole[:half])
        for st_ in (s1, s2):
            s.release_stream(st_.cuda_stream)
        # the existing entries still refuse the two new flag bits
        L = _lib.lib()
        rays = ceng795_amd.pack_rays(b.o[:64], b.d[:64])
        d_rays = rq_util.to_device(rays)
        out = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
        d_xy = torch.zeros(64 * 2, dtype=torch.float32, device="cuda")
        raw = np.zeros(64 * 32 + 16, np.uint8)
        raw_p = raw.ctypes.data + (-raw.ctypes.data % 16)
        with ceng795_amd.Film(s, 8, 8) as film:
            for bit in (_lib.RT_QUERY_LIGHTS_SHARED, _lib.RT_QUERY_NO_SCENE_LIGHTS):
                calls = [
                    lambda: L.rt_trace_rays(s.handle, rays.ctypes.data, 64, raw_p, bit),
                    lambda: L.rt_occluded(s.handle, rays.ctypes.data, 64, raw_p, bit),
                    lambda: L.rt_shade_rays(s.handle, rays.ctypes.data, 64, -1, raw_p, bit, None),
                    lambda: L.rt_trace_rays_device(s.handle, d_rays.data_ptr(), 64, out.data_ptr(),
                                                   bit, None),
                    lambda: L.rt_occluded_device(s.handle, d_rays.data_ptr(), 64, out.data_ptr(),
                                                 bit, None),
                    lambda: L.rt_shade_rays_device(s.handle, d_rays.data_ptr(), 64, -1,
                                                   out.data_ptr(), bit, None),
                    lambda: L.rt_film_shade_rays_device(film.handle, d_rays.data_ptr(),
                                                        d_xy.data_ptr(), 64, -1, bit, None),
                    lambda: L.rt_film_shade_rays(film.handle, rays.ctypes.data, raw_p, 64, -1, bit,
                                                 None)]
                for k, call in enumerate(calls):
                    assert call() == _lib.RT_E_INVALID and "flag" in L.rt_last_error().decode(), (k, bit)
    # multi-device scenes are refused
    d_out = torch.zeros(64 * 16, dtype=torch.uint8, device="cuda")
    d_lit = rq_util.to_device(rec[:64])
    with ceng795_amd.Scene(xml, devices=[0, 0]) as s:
        for call in (lambda: s.shade_rays_lit(b.o[:64], b.d[:64], rec[:64]),
                     lambda: s.shade_rays_lit_device(d_rays.data_ptr(), 64, d_lit.data_ptr(),
                                                     rec.shape[1], d_out.data_ptr())):
            with pytest.raises(ceng795_amd.RTError) as e:
                call()
            assert e.value.code == _lib.RT_E_UNSUPPORTED and "multi-device" in str(e.value)
    torch.cuda.synchronize()
