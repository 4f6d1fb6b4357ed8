"""Radiance queries on the GPU (rt_shade_rays*): Scene::trace_ray of caller-supplied rays against
the library's own frames (bit for bit: the same arithmetic) and the CPU oracle's frames.

A camera is only a ray generator, so the oracle's per-ray records of a scene's cameras (plus the
rig of rq_util for the depth-0 scenes) are the batches, and its frames the expected colours.  Each
test first asserts from the oracle alone that its batch holds the mix it is meant to check."""
import functools
import os

import numpy as np
import pytest

import desc_xml
import rq_util
import scenes
from conftest import assert_parity
from oracle.cpu_ref import OracleScene
from rq_util import INF, bits, shade_device, to_device

pytestmark = pytest.mark.gpu

FLAT = ["soup1", "hf_small", "single_sphere", "single_triangle", "graze_plane"]
MODES = ["fast", "reference"]


# ---------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def batch_of(xml):
    return rq_util.oracle_batch(xml)


@functools.lru_cache(maxsize=None)
def oracle_frames(xml):
    """Every camera's oracle frame as (n, 3) in ray order, concatenated, and the summed stats."""
    o = OracleScene(xml)
    frames, total = [], {"primary_rays": 0, "primary_hits": 0, "shadow_rays": 0, "secondary_rays": 0}
    for c in range(o.num_cameras):
        img, st = o.render(c, threads=8)
        frames.append(img.reshape(-1, 3))
        for k in total:
            total[k] += getattr(st, k)
    o.close()
    out = np.ascontiguousarray(np.concatenate(frames))
    out.setflags(write=False)
    return out, total


def write_variant(name, directory, tag, change):
    """A catalogue scene with `change(spec)` applied, as <name>_<tag>.xml."""
    path = os.path.join(directory, f"{name}_{tag}.xml")
    if not os.path.exists(path):
        spec = rq_util.spec_for(name) if name == "deep" else \
            {**scenes.CATALOGUE, **scenes.RECURSIVE}[name][0]()
        change(spec)
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            f.write(spec.to_xml())
        os.replace(tmp, path)
    return path


def with_depth(k):
    def change(spec):
        spec.max_depth = k
    return change


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                          np.ascontiguousarray(b).view(np.uint8))


def library_frames(s):
    """render_image of every camera as (n, 3) in ray order, concatenated."""
    return np.concatenate([s.render_image(c)[0].reshape(-1, 3) for c in range(s.num_cameras)])


def assert_t_matches(rad, b, what):
    assert np.array_equal(bits(rad["t"][b.hit]), bits(b.t[b.hit])), what
    assert (bits(rad["t"][~b.hit]) == bits(INF)).all(), what


# ---------------------------------------------------------------- 1. frames, depth-0 scenes
@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("name", FLAT)
def test_flat_scenes_give_their_frames(scene_dir, name, traversal):
    import ceng795_amd
    xml = rq_util.write_rigged(name, scene_dir)
    b = batch_of(xml)
    want, _ = oracle_frames(xml)
    if name == "single_triangle":
        assert b.hit.sum() >= 1 and (~b.hit).sum() >= 1
    else:
        assert b.hit.sum() >= 1000 and (~b.hit).sum() >= 1000
    assert b.skipped_axis.sum() >= 100  # from the rig
    if name == "single_sphere":
        assert (b.hit & (b.t < 0)).sum() >= 50
    background = np.array(desc_xml.Desc(xml).d.background[:], np.float32)
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        rad = s.shade_rays(b.o, b.d)
        frames = library_frames(s)
        hits = s.trace_rays(b.o, b.d)
        assert len(frames) == len(b)
        for c in range(s.num_cameras):  # camera by camera: the frame of that camera
            assert np.array_equal(bits(rad["rgb"][b.cam == c]), bits(frames[b.cam == c])), (name, c)
    assert assert_parity(rad["rgb"], want, f"{name}/{traversal}") == 0
    assert np.array_equal(bits(rad["t"]), bits(hits["t"]))
    assert_t_matches(rad, b, name)
    assert (bits(rad["rgb"][~b.hit]) == bits(background)).all()
    if name == "soup1":
        assert background.tolist() == [7, 13, 29]  # a zero would show


# ---------------------------------------------------------------- 2. recursion
@pytest.mark.parametrize("traversal", MODES)
@pytest.mark.parametrize("name", list(scenes.RECURSIVE))
def test_recursive_scenes_give_their_frames(scene_dir, name, traversal):
    import ceng795_amd
    xml = scenes.write(name, scene_dir)
    b = batch_of(xml)
    want, counts = oracle_frames(xml)
    for c in np.unique(b.cam):
        assert (b.hit & (b.cam == c)).sum() >= 481 and (~b.hit & (b.cam == c)).sum() >= 481
    assert counts["secondary_rays"] >= 100
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        rad, st = s.shade_rays(b.o, b.d, stats=True)
        frames = library_frames(s)
    assert np.array_equal(bits(rad["rgb"]), bits(frames))  # the same library arithmetic
    nbad = assert_parity(rad["rgb"], want, f"{name}/{traversal}")
    print(f"{name}/{traversal}: {nbad} channels differ from the oracle by 1 ulp")
    assert_t_matches(rad, b, name)
    for k, v in counts.items():
        assert getattr(st, k) == v, (k, getattr(st, k), v)


# ---------------------------------------------------------------- 3. the depth argument
@pytest.mark.parametrize("name", ["soup_depth3", "soup_depth6"])
def test_depth_argument(scene_dir, name):
    import ceng795_amd
    from ceng795_amd import _lib
    xml = scenes.write(name, scene_dir)
    D = desc_xml.Desc(xml).d.max_recursion_depth
    b = batch_of(xml)
    hit = b.hit
    at = {k: oracle_frames(write_variant(name, scene_dir, f"d{k}", with_depth(k)))[0]
          for k in (0, 1, D - 1)}
    at[D] = oracle_frames(xml)[0]

    def changed(x, y):
        return (hit & (bits(x) != bits(y)).any(axis=1)).sum()
    assert changed(at[0], at[1]) >= 100 and changed(at[1], at[D]) >= 100
    with ceng795_amd.Scene(xml) as s:
        for k in (0, 1, D - 1):
            rad = s.shade_rays(b.o, b.d, depth=k)
            nbad = assert_parity(rad["rgb"][hit], at[k][hit], f"{name}/depth{k}")
            if k == 0:
                assert nbad == 0
            assert_t_matches(rad, b, f"{name}/depth{k}")
            assert (bits(rad["rgb"][~hit]) == 0).all(), k  # below the maximum: black
        full = s.shade_rays(b.o, b.d, depth=D)
        assert same_bytes(full, s.shade_rays(b.o, b.d, depth=-1))
        assert same_bytes(full, s.shade_rays(b.o, b.d))
        for bad in (D + 1, -2):
            with pytest.raises(ceng795_amd.RTError) as e:
                s.shade_rays(b.o[:8], b.d[:8], depth=bad)
            assert e.value.code == _lib.RT_E_INVALID and "depth" in str(e.value)


# ---------------------------------------------------------------- 4. a caller-side bounce
def f32(x):
    return np.asarray(x, np.float32)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize(a):
    return a / np.sqrt(dot(a, a))[:, None]


def test_caller_side_bounce_and_in_medium(scene_dir):
    """The mirror ray of Scene.cpp:141-146 built by the caller in fp32 from rt_trace_rays' hit,
    shaded at depth 0 and combined by the caller, is the library's own depth-1 colour."""
    import ceng795_amd
    xml = write_variant("mirror_only", scene_dir, "d1", with_depth(1))
    desc = desc_xml.Desc(xml)
    eps = np.float32(desc.d.shadow_ray_epsilon)
    background = np.array(desc.d.background[:], np.float32)
    mirror = np.array([desc.mats[m].mirror[:] for m in range(desc.d.num_materials)], np.float32)
    b = batch_of(xml)
    with ceng795_amd.Scene(xml) as s:
        hits = s.trace_rays(b.o, b.d)
        hit = hits["leaf"] >= 0
        assert np.array_equal(hit, b.hit)
        km = np.zeros((len(b), 3), np.float32)
        km[hit] = mirror[hits["material"][hit]]
        is_mirror = hit & (km != 0).any(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.where(hit, hits["t"], f32(1))
            p = b.o + b.d * t[:, None]              # Ray::point_at
            w0 = normalize(b.o - p)
            n = hits["normal"]
            wr = normalize(n * (f32(2) * dot(n, w0))[:, None] - w0)
            mo, md = p + wr * eps, wr
        mo[~is_mirror], md[~is_mirror] = 0, (0, 0, 1)
        assert mo.dtype == md.dtype == np.float32
        A = s.shade_rays(b.o, b.d, depth=0)
        B = s.shade_rays(mo, md, depth=0)
        full = s.shade_rays(b.o, b.d, depth=1)
        medium = s.shade_rays(b.o, b.d, depth=1, in_medium=True)
        medium0 = s.shade_rays(b.o, b.d, depth=0, in_medium=True)
    lit = is_mirror & (B["rgb"] != 0).any(axis=1)
    assert lit.sum() >= 100
    zero = f32(0)
    want = zero + (A["rgb"] + km * B["rgb"])
    assert np.array_equal(bits(full["rgb"][is_mirror]), bits(want[is_mirror]))
    assert np.array_equal(bits(full["rgb"][hit & ~is_mirror]), bits(A["rgb"][hit & ~is_mirror]))
    want_medium = zero + (zero + km * B["rgb"])
    assert np.array_equal(bits(medium["rgb"][is_mirror]), bits(want_medium[is_mirror]))
    assert (bits(medium["rgb"][hit & ~is_mirror]) == 0).all()
    assert np.array_equal(bits(medium["t"]), bits(full["t"])) and \
        np.array_equal(bits(full["t"]), bits(hits["t"]))
    # the miss rule does not look at in_medium (Scene.cpp:94-99): depth 1 is this scene's maximum
    assert (bits(medium["rgb"][~hit]) == bits(background)).all()
    # depth 0: no local shading and nothing spawned; misses are below the maximum
    assert (bits(medium0["rgb"]) == 0).all() and np.array_equal(bits(medium0["t"]), bits(hits["t"]))


def test_in_medium_without_mirror_or_glass(scene_dir):
    """No material can spawn a ray, so in_medium leaves nothing to add: all-zero rgb wherever the
    miss rule gives black (depth below the maximum); at the maximum a miss is still the
    background, as trace_ray returns it before it looks at in_medium."""
    import ceng795_amd
    xml = write_variant("soup1", scene_dir, "d2", with_depth(2))
    b = batch_of(xml)
    assert b.hit.sum() >= 1000 and (~b.hit).sum() >= 1000
    with ceng795_amd.Scene(xml) as s:
        below = s.shade_rays(b.o, b.d, depth=1, in_medium=True)
        top = s.shade_rays(b.o, b.d, in_medium=True)
        plain = s.shade_rays(b.o, b.d)
    assert (bits(below["rgb"]) == 0).all()
    assert_t_matches(below, b, "in_medium")
    assert (bits(top["rgb"][b.hit]) == 0).all()
    assert (top["rgb"][~b.hit] == np.array([7, 13, 29], np.float32)).all()
    assert np.array_equal(bits(top["t"]), bits(plain["t"]))
    assert (plain["rgb"][b.hit] != 0).any(axis=1).sum() >= 1000


# ---------------------------------------------------------------- 5. independence
def test_independence(scene_dir):
    import ceng795_amd
    xml = scenes.write("soup_depth3", scene_dir)
    b = batch_of(xml)
    n = len(b)
    with ceng795_amd.Scene(xml) as s:
        whole = s.shade_rays(b.o, b.d)
        assert (whole["rgb"] != 0).any(axis=1).sum() >= 1000
        perm = np.random.default_rng(798).permutation(n)
        assert same_bytes(s.shade_rays(b.o[perm], b.d[perm]), whole[perm])
        assert same_bytes(s.shade_rays(b.o, b.d, reorder=True), whole)
        assert same_bytes(s.shade_rays(b.o[perm], b.d[perm], reorder=True), whole[perm])
        lo = (n // 6) // 64 * 64  # the middle rows of camera 0: hits, misses and bounces
        part = slice(lo, lo + 300)
        assert b.hit[part].sum() >= 50 and (~b.hit[part]).sum() >= 50
        for reorder in (False, True):
            for k in (0, 1, 63, 64, 65, 257):
                rad, tail = shade_device(s, b.o[part], b.d[part], n=k, pad=64, reorder=reorder)
                assert same_bytes(rad, whole[lo:lo + k]), (k, reorder)
                assert len(tail) == 64 * 16 and (tail == 0xA5).all(), (k, reorder)
        # invalid rays in the first and last lane of a wave
        o, d = b.o[lo:lo + 256].copy(), b.d[lo:lo + 256].copy()
        bad = [0, 63, 64, 127, 191]
        d[0], d[63], d[64] = (np.nan, 0, 1), (np.inf, 0, 0), (1e-7, -1e-7, 9e-7)
        o[127], d[191] = (0, np.inf, 0), (0, 0, 0)
        for reorder in (False, True):
            rad = s.shade_rays(o, d, reorder=reorder)
            good = np.ones(256, bool)
            good[bad] = False
            assert same_bytes(rad[good], whole[lo:lo + 256][good]), reorder
            assert (bits(rad["rgb"][bad]) == 0).all() and (bits(rad["t"][bad]) == bits(INF)).all()


# ---------------------------------------------------------------- 6. chunks
def test_chunks(scene_dir):
    import ceng795_amd
    from ceng795_amd import _lib
    xml = scenes.write("soup_depth6", scene_dir)
    b = batch_of(xml)
    n = 5700
    assert len(b) >= n
    per_ray = 4 * 28 * (6 + 1)  # (depth + 1) x 28 floats
    limit = 2048 * per_ray
    chunk = limit // per_ray // 64 * 64
    assert -(-n // chunk) >= 3 and (n % chunk) % 64 != 0 and n % chunk != 0
    with ceng795_amd.Scene(xml) as s:
        whole = s.shade_rays(b.o[:n], b.d[:n])
        s.set_radiance_scratch_limit(limit)
        for reorder in (False, True):
            assert same_bytes(s.shade_rays(b.o[:n], b.d[:n], reorder=reorder), whole), reorder
            rad, tail = shade_device(s, b.o[:n], b.d[:n], pad=64, reorder=reorder)
            assert same_bytes(rad, whole) and (tail == 0xA5).all(), reorder
        # one wave exactly still works; one byte less does not
        s.set_radiance_scratch_limit(64 * per_ray)
        assert same_bytes(s.shade_rays(b.o[:200], b.d[:200]), whole[:200])
        with pytest.raises(ceng795_amd.RTError) as e:
            s.set_radiance_scratch_limit(64 * per_ray - 1)
        assert e.value.code == _lib.RT_E_INVALID
        s.set_radiance_scratch_limit(0)  # the default again
        assert same_bytes(s.shade_rays(b.o[:n], b.d[:n]), whole)


# ---------------------------------------------------------------- 7. a tree deeper than 64
def mirror_floor(spec):
    spec.max_depth = 2
    spec.materials[0].mirror = (0.5, 0.4, 0.3)
    spec.cameras = list(spec.cameras) + rq_util.rig(rq_util.RIG_AT["deep"])


@pytest.mark.parametrize("variant", ["flat", "mirror"])
def test_deep_tree(scene_dir, variant):
    """rq_util.deep_scene (99 levels: the LDS spill stack), as it is and with a mirror material
    at depth 2 (the recursing kernel's spill-stack variant)."""
    import ceng795_amd
    xml = rq_util.write_rigged("deep", scene_dir) if variant == "flat" else \
        write_variant("deep", scene_dir, "mirror", mirror_floor)
    b = batch_of(xml)
    want, counts = oracle_frames(xml)
    assert b.hit.sum() >= 300 and (~b.hit).sum() >= 1
    if variant == "mirror":
        assert counts["secondary_rays"] >= 300
    for traversal in MODES:
        with ceng795_amd.Scene(xml, traversal=traversal) as s:
            assert s.bvh_depth > 64
            rad = s.shade_rays(b.o, b.d)
            assert np.array_equal(bits(rad["rgb"]), bits(library_frames(s)))
        assert_parity(rad["rgb"], want, f"deep/{variant}/{traversal}")
        assert_t_matches(rad, b, "deep")


# ---------------------------------------------------------------- 8. streams and scratch
def test_streams_and_scratch(scene_dir):
    import torch
    import ceng795_amd
    xml = scenes.write("soup_depth3", scene_dir)
    b = batch_of(xml)
    half = len(b) // 2
    ref_frame = OracleScene(xml).render(0, threads=8)[0]
    with ceng795_amd.Scene(xml) as s:
        whole, host_stats = s.shade_rays(b.o, b.d, stats=True)
        assert same_bytes(s.shade_rays(b.o, b.d, reorder=True), whole)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        r1 = to_device(ceng795_amd.pack_rays(b.o[:half], b.d[:half]))
        r2 = to_device(ceng795_amd.pack_rays(b.o[half:], b.d[half:]))
        o1 = torch.zeros(half * 16, dtype=torch.uint8, device="cuda")
        o1b = torch.zeros(half * 16, dtype=torch.uint8, device="cuda")
        o2 = torch.zeros((len(b) - half) * 16, dtype=torch.uint8, device="cuda")
        c = s.camera(0)
        frame = torch.zeros((c.height, c.width, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.collect_stats()
        # two streams in flight; on the first a frame between two queries
        s.shade_rays_device(r1.data_ptr(), half, o1.data_ptr(), reorder=True, stream=s1.cuda_stream)
        s.shade_rays_device(r2.data_ptr(), len(b) - half, o2.data_ptr(), stream=s2.cuda_stream)
        s.render_device(0, frame.data_ptr(), stream=s1.cuda_stream)
        s.shade_rays_device(r1.data_ptr(), half, o1b.data_ptr(), stream=s1.cuda_stream)
        s1.synchronize()
        s2.synchronize()
        rad_dtype = ceng795_amd.RADIANCE_DTYPE
        assert same_bytes(o1.cpu().numpy().view(rad_dtype), whole[:half])
        assert same_bytes(o1b.cpu().numpy().view(rad_dtype), whole[:half])
        assert same_bytes(o2.cpu().numpy().view(rad_dtype), whole[half:])
        assert_parity(frame.cpu().numpy(), ref_frame, "frame between two queries")
        # the device variant counts into the scene's counters: two half batches, one whole one
        # and one frame of camera 0
        st = s.collect_stats()
        cam0 = int((b.cam == 0).sum())
        assert st.primary_rays == host_stats.primary_rays + half + cam0
        assert s.stream_frame_scratch_bytes(s1.cuda_stream) > 0
        s.release_stream(s1.cuda_stream)
        assert s.stream_frame_scratch_bytes(s1.cuda_stream) == 0
        again, _ = shade_device(s, b.o[:half], b.d[:half], stream=s1, reorder=True)
        assert same_bytes(again, whole[:half])
        # a query that cannot recurse leaves no ray-tree scratch behind: depth 0 on a fresh stream
        s3 = torch.cuda.Stream()
        flat, _ = shade_device(s, b.o, b.d, stream=s3, depth=0, reorder=True)
        assert same_bytes(flat, s.shade_rays(b.o, b.d, depth=0))
        assert s.stream_frame_scratch_bytes(s3.cuda_stream) == 0
        for st_ in (s1, s2, s3):
            s.release_stream(st_.cuda_stream)
        # the other queries still leave the counters alone
        s.collect_stats()
        s.trace_rays(b.o[:100], b.d[:100])
        assert s.collect_stats().primary_rays == 0
        assert len(s.shade_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    # ... and any depth on a scene without mirror or glass
    flat_xml = rq_util.write_rigged("soup1", scene_dir)
    fb = batch_of(flat_xml)
    with ceng795_amd.Scene(flat_xml) as s:
        s4 = torch.cuda.Stream()
        rad, _ = shade_device(s, fb.o, fb.d, stream=s4)
        assert same_bytes(rad, s.shade_rays(fb.o, fb.d))
        assert s.stream_frame_scratch_bytes(s4.cuda_stream) == 0
        s.release_stream(s4.cuda_stream)


# ---------------------------------------------------------------- 9. refusals
def test_refusals(scene_dir):
    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    xml = rq_util.write_rigged("soup1", scene_dir)
    b = batch_of(xml)
    rays = ceng795_amd.pack_rays(b.o[:64], b.d[:64])
    d_rays = to_device(rays)
    out = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
    with ceng795_amd.Scene(xml, devices=[0, 0]) as s:
        for call in (lambda: s.shade_rays(b.o[:64], b.d[:64]),
                     lambda: s.shade_rays_device(d_rays.data_ptr(), 64, out.data_ptr())):
            with pytest.raises(ceng795_amd.RTError) as e:
                call()
            assert e.value.code == _lib.RT_E_UNSUPPORTED and "multi-device" in str(e.value)
    hits = np.zeros(64 * 32 + 16, np.uint8)
    hits_p = hits.ctypes.data + (-hits.ctypes.data % 16)
    with ceng795_amd.Scene(xml) as s:
        L = _lib.lib()
        for fn in (L.rt_trace_rays, L.rt_occluded):
            rc = fn(s.handle, rays.ctypes.data, 64, hits_p, _lib.RT_QUERY_IN_MEDIUM)
            assert rc == _lib.RT_E_INVALID and "flag" in L.rt_last_error().decode()
        for fn in (L.rt_trace_rays_device, L.rt_occluded_device):
            rc = fn(s.handle, d_rays.data_ptr(), 64, out.data_ptr(), _lib.RT_QUERY_IN_MEDIUM, None)
            assert rc == _lib.RT_E_INVALID and "flag" in L.rt_last_error().decode()
    torch.cuda.synchronize()
