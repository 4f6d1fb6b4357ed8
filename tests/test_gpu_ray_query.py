"""Ray queries on the GPU (rt_trace_rays* / rt_occluded*): closest hit and occlusion of
caller-supplied rays against the CPU oracle's per-ray records, bit for bit.

Every batch is the rays of a scene's own cameras plus a rig of six 33x31 cameras at one point
(rq_util.rig), concatenated in camera order, and the same rays under a seeded permutation, so
that a wave mixes origins and directions.  Each test first asserts from the oracle alone that
its batch holds the mix it is meant to check (hits, misses, rays with a skipped axis,
negative-t hits), so it cannot pass vacuously."""
import functools

import numpy as np
import pytest

import desc_xml
import rq_util
from conftest import assert_parity
from oracle.cpu_ref import OracleScene
from rq_util import INF, assert_hits_match, bits, occlusion, same_records, to_device, trace

pytestmark = pytest.mark.gpu

SCENES = ["soup1", "hf_small", "single_sphere", "single_triangle", "graze_plane"]


@functools.lru_cache(maxsize=None)
def batch_of(xml):
    return rq_util.oracle_batch(xml)


def assert_mix(name, b):
    if name in ("single_triangle", "deep"):  # (small scenes: some of each)
        assert b.hit.sum() >= 1 and (~b.hit).sum() >= 1
        return
    assert b.hit.sum() >= 1000 and (~b.hit).sum() >= 1000
    assert b.skipped_axis.sum() >= 100
    if name == "single_sphere":
        assert (b.hit & (b.t < 0)).sum() >= 50


def closest_hit_case(s, name, b, reorder):
    hits, _ = trace(s, b.o, b.d, reorder=reorder)
    assert_hits_match(hits, b, f"{name}/ordered/reorder{reorder}")
    perm = np.random.default_rng(795).permutation(len(b))
    mixed, _ = trace(s, b.o[perm], b.d[perm], reorder=reorder)
    assert same_records(mixed, hits[perm]), f"{name}/permuted/reorder{reorder}"
    return hits


# ---------------------------------------------------------------- 1. closest hit vs the oracle
@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("traversal", ["fast", "reference"])
@pytest.mark.parametrize("name", SCENES)
def test_closest_hit_matches_oracle(scene_dir, name, traversal, reorder):
    import ceng795_amd
    xml = rq_util.write_rigged(name, scene_dir)
    b = batch_of(xml)
    assert len(b) < 40000
    assert_mix(name, b)
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        closest_hit_case(s, name, b, reorder)


# ---------------------------------------------------------------- 2. leaf vs the renderer
def test_leaf_object_material_match_renderer(scene_dir):
    """soup1 camera 0: the query's leaf is the leaf of the frame kernel's pixel record, and its
    object / material are that leaf's in the host-side leaf table and the object lists."""
    import torch
    import ceng795_amd
    xml = rq_util.write_rigged("soup1", scene_dir)
    b = batch_of(xml)
    cam0 = b.cam == 0
    desc = desc_xml.Desc(xml)
    leaf_objects = ceng795_amd.host_leaf_objects(desc.d)
    objects = rq_util.object_list(desc)
    with ceng795_amd.Scene(xml) as s:
        c = s.camera(0)
        rec = torch.zeros((c.height, c.width), dtype=torch.int32, device="cuda")
        s.render_device(0, rec.data_ptr(), records=True,
                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rec = rec.cpu().numpy().view(np.uint32).reshape(-1)
        hits, _ = trace(s, b.o[cam0], b.d[cam0])
    k_leaf_mask, k_miss = (1 << 26) - 1, 1  # rt_internal.h kRecLeafMask, kRecMiss >> 30
    hit = hits["leaf"] >= 0
    assert np.array_equal(hit, b.hit[cam0]) and hit.sum() >= 1000 and (~hit).sum() >= 1000
    assert np.array_equal((rec >> 30) == 0, hit) and ((rec >> 30)[~hit] == k_miss).all()
    assert np.array_equal((rec & k_leaf_mask)[hit], hits["leaf"][hit].astype(np.uint32))
    assert np.array_equal(hits["object"][hit], leaf_objects[hits["leaf"][hit]])
    want_material = np.array([objects[o][-1] for o in hits["object"][hit]], np.int32)
    assert np.array_equal(hits["material"][hit], want_material)


# ---------------------------------------------------------------- 3. occlusion
def tmax_cycle(b):
    """tmax by ray index over {t, next above t, next below t, t/2, 2t, 0, -1, +inf, NaN}."""
    t = b.t.astype(np.float32)
    choices = np.stack([t, np.nextafter(t, INF), np.nextafter(t, -INF), t / 2, 2 * t,
                        np.zeros_like(t), -np.ones_like(t), np.full_like(t, np.inf),
                        np.full_like(t, np.nan)])
    return choices[np.arange(len(t)) % 9, np.arange(len(t))]


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_occlusion_matches_oracle(scene_dir, name, reorder):
    import ceng795_amd
    xml = rq_util.write_rigged(name, scene_dir)
    b = batch_of(xml)
    assert_mix(name, b)
    tmax = tmax_cycle(b)
    with np.errstate(invalid="ignore"):
        want = (b.hit & (b.t > 0) & (b.t < tmax)).astype(np.uint8)
    if name != "single_triangle":
        assert want.sum() >= 300 and (b.hit & (want == 0)).sum() >= 300
    perm = np.random.default_rng(796).permutation(len(b))
    for mode in ("fast", "reference"):
        with ceng795_amd.Scene(xml, traversal=mode) as s:
            got, _ = occlusion(s, b.o, b.d, tmax, reorder=reorder)
            assert np.array_equal(got, want), (name, mode)
            mixed, _ = occlusion(s, b.o[perm], b.d[perm], tmax[perm], reorder=reorder)
            assert np.array_equal(mixed, want[perm]), (name, mode)


# ---------------------------------------------------------------- 4. batch shapes
def test_prefixes_and_untouched_tail(scene_dir):
    import ceng795_amd
    xml = rq_util.write_rigged("soup1", scene_dir)
    b = batch_of(xml)
    tmax = tmax_cycle(b)
    with ceng795_amd.Scene(xml) as s:
        whole, _ = trace(s, b.o, b.d)
        whole_occ, _ = occlusion(s, b.o, b.d, tmax)
        for reorder in (False, True):
            for n in (0, 1, 63, 64, 65, 257):
                hits, tail = trace(s, b.o[:300], b.d[:300], reorder=reorder, n=n, pad=64)
                assert same_records(hits, whole[:n]), (n, reorder)
                assert len(tail) == 64 * 32 and (tail == 0xA5).all(), (n, reorder)
                occ, tail = occlusion(s, b.o[:300], b.d[:300], tmax[:300], reorder=reorder, n=n,
                                      pad=64)
                assert np.array_equal(occ, whole_occ[:n]), (n, reorder)
                assert len(tail) == 64 and (tail == 0xA5).all(), (n, reorder)


# ---------------------------------------------------------------- 5. invalid rays
@pytest.mark.parametrize("reorder", [False, True])
def test_invalid_rays_miss_and_disturb_nothing(scene_dir, reorder):
    import ceng795_amd
    xml = rq_util.write_rigged("soup1", scene_dir)
    b = batch_of(xml)
    n = len(b)
    rng = np.random.default_rng(797)
    bad = np.unique(np.concatenate([rng.choice(n, 200, replace=False),
                                    [0, 63, 64 * 7, 64 * 7 + 63, 64 * 100, 64 * 100 + 63, n - 1]]))
    assert b.hit[bad].sum() >= 20  # some of them would have hit
    o, d = b.o.copy(), b.d.copy()
    kinds = [("d", (np.nan, 0, 1)), ("d", (np.inf, 0, 0)), ("d", (0, -np.inf, 0)), ("d", (0, 0, 0)),
             ("o", (np.nan, 0, 0)), ("o", (0, np.inf, 0)), ("o", (0, 0, -np.inf)),
             ("d", (1e-7, -1e-7, 9e-7)), ("d", (-0.0, 0.0, -0.0))]
    for k, i in enumerate(bad):
        which, v = kinds[k % len(kinds)]
        (o if which == "o" else d)[i] = v
    tmax = np.full(n, np.inf, np.float32)
    with ceng795_amd.Scene(xml) as s:
        clean, _ = trace(s, b.o, b.d)
        clean_occ, _ = occlusion(s, b.o, b.d, tmax)
        assert clean_occ[b.hit].all()
        hits, _ = trace(s, o, d, reorder=reorder)
        occ, _ = occlusion(s, o, d, tmax, reorder=reorder)
    good = np.ones(n, bool)
    good[bad] = False
    assert same_records(hits[good], clean[good]) and np.array_equal(occ[good], clean_occ[good])
    assert (occ[bad] == 0).all()
    h = hits[bad]
    assert (bits(h["t"]) == bits(INF)).all() and (bits(h["normal"]) == 0).all()
    assert (h["object"] == -1).all() and (h["material"] == -1).all() and (h["leaf"] == -1).all()


# ---------------------------------------------------------------- 6. far origin
def test_far_origin_fast_mode(scene_dir):
    """A camera 2e5 scene diameters away: its rays' origins lie far outside every culling box,
    where the ray's own margin share 2^-18 |o| / |d| is what keeps the slot tests conservative
    (DESIGN.md §4.11)."""
    import ceng795_amd
    spec = rq_util.spec_for("soup1")
    v = np.array(desc_xml.floats(spec.vertex_text), np.float32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    diameter = float(np.linalg.norm(hi - lo))
    centre = tuple(float(x) for x in (lo + hi) / 2)
    xml = rq_util.write_rigged("soup1", scene_dir, extra=[rq_util.far_camera(centre, diameter)])
    far = OracleScene(xml).num_cameras - 1
    b = rq_util.oracle_batch(xml, [far])
    assert np.linalg.norm(b.o[0] - np.array(centre)) >= 1e5 * diameter
    assert b.hit.sum() >= 100 and (~b.hit).sum() >= 100
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        for reorder in (False, True):
            hits, _ = trace(s, b.o, b.d, reorder=reorder)
            assert_hits_match(hits, b, f"far/reorder{reorder}")


# ---------------------------------------------------------------- 7. streams and scratch
def test_streams_scratch_and_host_variants(scene_dir):
    import torch
    import ceng795_amd
    xml = rq_util.write_rigged("soup1", scene_dir)
    b = batch_of(xml)
    tmax = tmax_cycle(b)
    half = len(b) // 2
    ref_frame = OracleScene(xml).render(0, threads=8)[0]
    with ceng795_amd.Scene(xml) as s:
        whole, _ = trace(s, b.o, b.d)
        whole_occ, _ = occlusion(s, b.o, b.d, tmax)
        assert_hits_match(whole, b, "whole")
        # two streams, each with a flagged query on the same scene, in flight together
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r1 = to_device(ceng795_amd.pack_rays(b.o[:half], b.d[:half]))
        r2 = to_device(ceng795_amd.pack_rays(b.o[half:], b.d[half:], tmax[half:]))
        o1 = torch.zeros(half * 32, dtype=torch.uint8, device="cuda")
        o2 = torch.zeros(len(b) - half, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s.trace_rays_device(r1.data_ptr(), half, o1.data_ptr(), reorder=True, stream=s1.cuda_stream)
        s.occluded_device(r2.data_ptr(), len(b) - half, o2.data_ptr(), reorder=True,
                          stream=s2.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        assert same_records(o1.cpu().numpy().view(ceng795_amd.HIT_DTYPE), whole[:half])
        assert np.array_equal(o2.cpu().numpy(), whole_occ[half:])
        # a frame before and after a flagged query on one stream: still the oracle's
        c = s.camera(0)
        for _ in range(2):
            frame = torch.zeros((c.height, c.width, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s1):
                s.render_device(0, frame.data_ptr(), stream=s1.cuda_stream)
                s.trace_rays_device(r1.data_ptr(), half, o1.data_ptr(), reorder=True,
                                    stream=s1.cuda_stream)
            s1.synchronize()
            assert assert_parity(frame.cpu().numpy(), ref_frame, "frame around a query") == 0
        # release the stream's scratch, then query on it again
        s.release_stream(s1.cuda_stream)
        again, _ = trace(s, b.o[:half], b.d[:half], reorder=True, stream=s1)
        assert same_records(again, whole[:half])
        s.release_stream(s1.cuda_stream)
        s.release_stream(s2.cuda_stream)
        # host variants = device variants
        for reorder in (False, True):
            assert same_records(s.trace_rays(b.o, b.d, reorder=reorder), whole)
            assert np.array_equal(s.occluded(b.o, b.d, tmax, reorder=reorder), whole_occ)
        assert len(s.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
        # queries leave the ray counters alone
        s.collect_stats()
        s.trace_rays(b.o[:100], b.d[:100])
        st = s.collect_stats()
        assert st.primary_rays == 0 and st.shadow_rays == 0 and st.primary_hits == 0


# ---------------------------------------------------------------- 8. multi-device scenes
def test_multi_device_scene_is_unsupported(scene_dir):
    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    xml = rq_util.write_rigged("soup1", scene_dir)
    b = batch_of(xml)
    rays = to_device(ceng795_amd.pack_rays(b.o[:64], b.d[:64]))
    out = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    with ceng795_amd.Scene(xml, devices=[0, 0]) as s:
        calls = [lambda: s.trace_rays(b.o[:64], b.d[:64]),
                 lambda: s.occluded(b.o[:64], b.d[:64], 1.0),
                 lambda: s.trace_rays_device(rays.data_ptr(), 64, out.data_ptr()),
                 lambda: s.occluded_device(rays.data_ptr(), 64, out.data_ptr())]
        for call in calls:
            with pytest.raises(ceng795_amd.RTError) as e:
                call()
            assert e.value.code == _lib.RT_E_UNSUPPORTED and "multi-device" in str(e.value)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 9. a tree deeper than 64
@pytest.mark.parametrize("traversal", ["fast", "reference"])
def test_deep_tree(scene_dir, traversal):
    """rq_util.deep_scene: more levels than the per-lane stack holds, so every kernel takes its
    LDS spill stack.  First the frame (no other test renders a deep ray-tracing scene), then
    the closest-hit comparison of test 1."""
    import ceng795_amd
    xml = rq_util.write_rigged("deep", scene_dir)
    b = batch_of(xml)
    assert_mix("deep", b)
    assert b.hit.sum() >= 300
    o = OracleScene(xml)
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        assert s.bvh_depth > 64
        got, _ = s.render_image(0)
        assert assert_parity(got, o.render(0, threads=8)[0], "deep frame") == 0
        for reorder in (False, True):
            closest_hit_case(s, "deep", b, reorder)
            occ, _ = occlusion(s, b.o, b.d, np.full(len(b), np.inf, np.float32), reorder=reorder)
            assert np.array_equal(occ, (b.hit & (b.t > 0)).astype(np.uint8))
