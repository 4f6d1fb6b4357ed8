"""GPU parity on scenes far from the origin and off unit scale (scenes.PLACED, tests/placed.py):
both traversals against the CPU oracle, which tests/test_placed_host.py pins to the reference on
exactly these scenes.  Every comparison is bit for bit; no tolerance.

What depends on the scene's magnitude: the per-axis culling margin
2^-18 max|root box coordinate| + 2^-100 and the fp16 slot planes built with it, the ray's share
2^-18 |o| / |d| of that margin, the 2^-20 decision band of the guard test, and the reference's
own absolute constants, which a resized scene meets on other branches.  At offsets of 1e5 .. 7e5
the margin exceeds most primitives: nearly every slot is entered and the guard tests decide.

  * frames: render_image of every camera, with the ray counts (test_gpu_parity.py);
  * camera 0's pixel rays through trace_rays / occluded / shade_rays (test_wide_slots.py);
  * the MSAA base: the jittered, splatted frame against render_msaa for one seed;
  * the pixel-record exchange (test_gpu_records.py) on one translated and one small soup;
  * the `interior` and `surface` ray families, whose rays derive from the scene's root box, on
    the soup at offset (1e5, 3e5, -7e5) and at scale 2^-20 (their mix conditions hold from the
    oracle alone on both: test_placed_host.py, so neither family is left out)."""
import functools
import os

import numpy as np
import pytest

import ray_batches as rb
import rq_util
import scenes
from oracle.cpu_ref import OracleScene
from rq_util import assert_hits_match, bits

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
MODES = ["fast", "reference"]
NAMES = list(scenes.PLACED)
FLAT = [n for n in NAMES if scenes.placed_parts(n)[0] != "msaa"]
MSAA = [n for n in NAMES if scenes.placed_parts(n)[0] == "msaa"]
MSAA_SEED = 12345
RECORD_SCENES = ["soup@t1e5", "soup@s2m31"]
FAMILY_SCENES = ["soup@t1e5", "soup@s2m20"]
FAMILIES = ["interior", "surface"]


def differing(got, ref):
    return int((bits(got) != bits(ref)).sum())


# ---------------------------------------------------------------- the oracle's side, once
@functools.lru_cache(maxsize=None)
def oracle_frames(xml):
    o = OracleScene(xml)
    return [o.render(cam, threads=THREADS) for cam in range(o.num_cameras)]


@functools.lru_cache(maxsize=None)
def oracle_msaa_frames(xml):
    o = OracleScene(xml)
    return [o.render_msaa(cam, seed=MSAA_SEED, threads=THREADS) for cam in range(o.num_cameras)]


@functools.lru_cache(maxsize=None)
def pixel_rays(xml):
    """Camera 0's pixel rays with the oracle's closest hits and radiance."""
    b = rq_util.oracle_batch(xml, cameras=[0])
    o = OracleScene(xml)
    rad, st = o.shade_rays(b.o, b.d)
    o.close()
    for a in (b.o, b.d, b.t, b.normal, b.hit, rad):
        a.setflags(write=False)
    return b, rad, st.as_dict()


@functools.lru_cache(maxsize=None)
def family_rays(xml, name, family):
    b = rb.family(rb.scene_info(xml, name), family)
    o = OracleScene(xml)
    rec, shape = o.intersect_rays(b.o, b.d)
    rad, st = o.shade_rays(b.o, b.d)
    o.close()
    assert not np.isnan(rec[:, 3]).any()
    return b, rec, shape, rad, st.as_dict()


def assert_counts(gst, st, what, recursive):
    assert gst.primary_rays == st.primary_rays, what
    assert gst.primary_hits == st.primary_hits, what
    assert gst.shadow_rays == st.shadow_rays, what
    if recursive:
        assert gst.secondary_rays == st.secondary_rays, what


# ---------------------------------------------------------------- frames
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FLAT)
def test_render_matches_oracle(scene_dir, name, mode):
    import ceng795_amd
    xml = scenes.write(name, scene_dir)
    refs = oracle_frames(xml)
    with ceng795_amd.Scene(xml, traversal=mode) as s:
        assert s.num_cameras == len(refs)
        got = [s.render_image(cam) for cam in range(s.num_cameras)]
    bad = [differing(g, ref) for (g, _), (ref, _) in zip(got, refs)]
    print(f"{name}/{mode}: channels differing from the oracle per camera {bad}")
    for cam, ((g, gst), (ref, st)) in enumerate(zip(got, refs)):
        what = f"{name}/cam{cam}/{mode}"
        assert np.isfinite(ref).all(), what
        assert g.shape == ref.shape and bad[cam] == 0, f"{what}: {bad[cam]} channels differ"
        assert_counts(gst, st, what, scenes.placed_parts(name)[0] == "depth3")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", MSAA)
def test_msaa_matches_oracle(scene_dir, name, mode):
    import ceng795_amd
    xml = scenes.write(name, scene_dir)
    refs = oracle_msaa_frames(xml)
    with ceng795_amd.Scene(xml, traversal=mode) as s:
        s.set_msaa_seed(MSAA_SEED)
        got = [s.render_image(cam) for cam in range(s.num_cameras)]
    bad = [differing(g, ref) for (g, _), (ref, _) in zip(got, refs)]
    print(f"{name}/{mode}/seed{MSAA_SEED}: channels differing per camera {bad}")
    for cam, ((g, gst), (ref, st)) in enumerate(zip(got, refs)):
        what = f"{name}/cam{cam}/{mode}"
        assert np.isfinite(ref).all(), what
        assert bad[cam] == 0, f"{what}: {bad[cam]} channels differ"
        assert_counts(gst, st, what, True)


# ---------------------------------------------------------------- camera 0's rays as queries
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_pixel_rays_as_queries_match_oracle(scene_dir, name, mode):
    """trace_rays: hit set, t, normal and ids; occluded: tmax cycled over {t, just above, just
    below, t/2, 2t, 0, -1, inf, NaN} of the oracle's t; shade_rays: the colour and t of
    Scene::trace_ray, which for these rays is the frame's pixel."""
    import ceng795_amd
    xml = scenes.write(name, scene_dir)
    b, rad, counts = pixel_rays(xml)
    tmax = rb.tmax_cycle(b.t)
    with np.errstate(invalid="ignore"):
        occ = (b.hit & (b.t > 0) & (b.t < tmax)).astype(np.uint8)
    assert b.hit.sum() >= 100 and occ.sum() >= 10 and (b.hit & (occ == 0)).sum() >= 10
    if name in FLAT:
        frame = oracle_frames(xml)[0][0].reshape(-1, 3)
        assert np.array_equal(bits(rad[:, 0:3]), bits(frame))
    with ceng795_amd.Scene(xml, traversal=mode) as s:
        hits = s.trace_rays(b.o, b.d)
        got_occ = s.occluded(b.o, b.d, tmax)
        got_rad, gst = s.shade_rays(b.o, b.d, stats=True)
    what = f"{name}/{mode}"
    print(f"{what}: {len(b)} rays, {int(b.hit.sum())} hits; "
          f"{int(((hits['leaf'] >= 0) != b.hit).sum())} hit flags, "
          f"{int((got_occ != occ).sum())} occlusion bytes, "
          f"{differing(got_rad['rgb'], rad[:, 0:3])} colour channels differ")
    assert_hits_match(hits, b, what)
    assert np.array_equal(got_occ, occ), what
    assert differing(got_rad["rgb"], rad[:, 0:3]) == 0, what
    assert np.array_equal(bits(got_rad["t"]), bits(rad[:, 3])), what
    for k in ("primary_rays", "shadow_rays", "secondary_rays"):
        assert getattr(gst, k) == counts[k], (what, k)


# ---------------------------------------------------------------- pixel records
@pytest.mark.parametrize("name", RECORD_SCENES)
def test_record_exchange_matches_oracle(scene_dir, name):
    import ceng795_amd
    from test_gpu_records import assembled
    xml = scenes.write(name, scene_dir)
    refs = [f for f, _ in oracle_frames(xml)]
    with ceng795_amd.Scene(xml) as s:
        assert all(s.records_ok(c) for c in range(s.num_cameras))
        for world in (1, 3, 8):
            for inplace in (False, True):
                got = assembled(s, world, root_inplace=inplace)
                for c, (g, ref) in enumerate(zip(got, refs)):
                    what = f"{name}/cam{c}/world{world}/inplace{inplace}"
                    assert differing(g, ref) == 0, what


# ---------------------------------------------------------------- rays from the root box
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", FAMILY_SCENES)
def test_ray_families_match_oracle(scene_dir, name, family, mode):
    """Origins inside the (far or tiny) root box and on its surfaces with and without the scaled
    epsilon, shadow rays built as Scene.cpp builds them: closest hit, occlusion and radiance,
    in the given order and under the seeded permutation."""
    import ceng795_amd
    xml = scenes.write(name, scene_dir)
    b, rec, shape, rad, counts = family_rays(xml, name, family)
    want = rq_util.Batch(b.o, b.d, rec[:, 3], rec[:, 4:7], rec[:, 7] == 1.0, None)
    tmax = rb.occlusion_tmax(b, want.t)
    with np.errstate(invalid="ignore"):
        occ = (want.hit & (want.t > 0) & (want.t < tmax)).astype(np.uint8)
    perm = rb.permutation(b)
    with ceng795_amd.Scene(xml, traversal=mode) as s:
        hits = s.trace_rays(b.o, b.d)
        hits_perm = s.trace_rays(b.o[perm], b.d[perm], reorder=True)
        got_occ = s.occluded(b.o, b.d, tmax)
        occ_perm = s.occluded(b.o[perm], b.d[perm], tmax[perm], reorder=True)
        got_rad, gst = s.shade_rays(b.o, b.d, stats=True)
    what = f"{name}/{family}/{mode}"
    print(f"{what}: {len(b)} rays, {int(want.hit.sum())} hits, {int(occ.sum())} occluded; "
          f"{int(((hits['leaf'] >= 0) != want.hit).sum())} hit flags, "
          f"{int((got_occ != occ).sum())} occlusion bytes, "
          f"{differing(got_rad['rgb'], rad[:, 0:3])} colour channels differ")
    assert_hits_match(hits, want, what)
    assert np.array_equal(hits["object"][want.hit], shape[want.hit]), what
    assert rq_util.same_records(hits_perm, hits[perm]), what + "/permuted"
    assert np.array_equal(got_occ, occ), what
    assert np.array_equal(occ_perm, occ[perm]), what + "/permuted"
    assert differing(got_rad["rgb"], rad[:, 0:3]) == 0, what
    assert np.array_equal(bits(got_rad["t"]), bits(rad[:, 3])), what
    for k in ("primary_rays", "shadow_rays", "secondary_rays"):
        assert getattr(gst, k) == counts[k], (what, k)
