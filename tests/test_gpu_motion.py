"""Scenes with motion on the GPU (rt_scene_create_moving, RT_QUERY_RAY_TIME):
closest hits, occlusion, radiance, films and frames against the composite reference with per-ray
matrices (tests/motion_util.py), bit for bit, in both traversal modes.  The mix of the main batch
is asserted on the CPU (tests/test_motion_host.py::test_main_batch_mix)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ceng795_amd
import instance_util as iu
import motion_util as mu
from ceng795_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ["fast", "reference"]
COUNTERS = ("primary_rays", "primary_hits", "shadow_rays", "secondary_rays")
_REF = {}  # restated answers, computed once and left unchanged


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def cases(scene_dir):
    """name -> (spec, composite, scene), made once."""
    made = {}

    def get(name):
        if name not in made:
            spec = mu.written(name, scene_dir)
            comp = mu.MotionComposite(spec)
            made[name] = (spec, comp, spec.create(comp.desc.d))
        return made[name]
    yield get
    for spec, comp, s in made.values():
        s.close()
        comp.close()


def main_reference(cases):
    spec, comp, s = cases("main")
    if "main" not in _REF:
        o, d, time = mu.main_batch()
        ref = comp.intersect(o, d, time)
        _REF["main"] = (o, d, time, ref)
    return (spec, comp, s) + _REF["main"]


def check_occlusion(s, comp, o, d, time, ref, what):
    h = ref.hit
    t = ref.t[h]
    for tmax, want in ((t, 0), (np.nextafter(t, F(0)), 0), (np.nextafter(t, F(np.inf)), 1)):
        occ = s.occluded(o[h], d[h], tmax, time=time[h])
        assert np.array_equal(occ, comp.occluded(o[h], d[h], tmax, time[h])), what
        assert (occ == want).all(), what
    big = np.full(len(o), 1e30, F)
    assert np.array_equal(s.occluded(o, d, big, time=time), ref.hit.astype(np.uint8)), what


@pytest.mark.parametrize("mode", MODES)
def test_main_closest_and_occlusion(cases, mode):
    """The main scene, every ray at its own time (64 different times in every wave): t bits,
    object, material, leaf, instance and normal; occlusion with tmax at, just below and just
    above the hit's t.  A library that ignored the time would fail on >= 100 rays."""
    spec, comp, s, o, d, time, ref = main_reference(cases)
    assert s.has_motion and s.num_instances == 4
    s.set_traversal(mode)
    hits = s.trace_rays(o, d, time=time)
    iu.assert_hits(hits, ref, mode)
    check_occlusion(s, comp, o, d, time, ref, mode)
    again = s.trace_rays(o, d, time=time, reorder=True)
    assert np.array_equal(hits.view(np.uint8), again.view(np.uint8))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [50, 114, 17 * 9])
def test_time_patterns_shuffles_and_invalid_times(cases, mode, n):
    """Batches of n rays drawn from the main batch and shuffled, with the times one per wave, the
    special times 0, +-1, 1.5 and -0.0, and a NaN and an inf time in lanes 0 and 63 (invalid
    rays; their neighbours undisturbed); RT_QUERY_REORDER gives identical records."""
    spec, comp, s, o, d, time, ref = main_reference(cases)
    s.set_traversal(mode)
    rng = np.random.default_rng(n)
    pick = rng.permutation(len(o))[:n]
    o, d = o[pick].copy(), d[pick].copy()
    per_wave = np.repeat(rng.random((n + 63) // 64).astype(F), 64)[:n]
    special = mu.SPECIAL_TIMES[np.arange(n) % len(mu.SPECIAL_TIMES)]
    for what, tau in (("wave", per_wave), ("special", special), ("own", time[pick])):
        want = comp.intersect(o, d, tau)
        hits = s.trace_rays(o, d, time=tau)
        iu.assert_hits(hits, want, (mode, n, what))
        assert np.array_equal(hits.view(np.uint8), s.trace_rays(o, d, time=tau, reorder=True).view(np.uint8))
        tm = np.where(want.hit, np.nextafter(want.t, F(np.inf)), F(1e30)).astype(F)
        occ = s.occluded(o, d, tm, time=tau)
        assert np.array_equal(occ, comp.occluded(o, d, tm, tau)), (mode, n, what)
        assert np.array_equal(occ, s.occluded(o, d, tm, time=tau, reorder=True))
    bad = time[pick].copy()
    bad[0] = np.nan
    bad[min(63, n - 1)] = np.inf
    if n > 64:
        bad[64] = -np.inf
    want = comp.intersect(o, d, bad)
    hits = s.trace_rays(o, d, time=bad)
    iu.assert_hits(hits, want, (mode, n, "invalid"))
    assert not want.hit[0] and not want.hit[min(63, n - 1)]
    clean = s.trace_rays(o, d, time=time[pick])
    keep = np.isfinite(bad)
    assert np.array_equal(hits[keep].view(np.uint8), clean[keep].view(np.uint8))
    assert not s.occluded(o, d, np.full(n, 1e30, F), time=bad)[~keep].any()


@pytest.mark.parametrize("mode", MODES)
def test_without_the_flag_pad_is_ignored(cases, mode):
    """Without RT_QUERY_RAY_TIME a batch with garbage in pad equals the batch at time 0."""
    spec, comp, s, o, d, time, ref = main_reference(cases)
    s.set_traversal(mode)
    want = comp.intersect(o, d, np.zeros(len(o), F))
    rays = ceng795_amd.pack_rays(o, d, tmax=1e30, time=np.where(np.arange(len(o)) % 3 == 0, np.nan, time * 50))
    hits = ceng795_amd.scene._aligned(len(o), ceng795_amd.HIT_DTYPE)
    _lib.check(_lib.lib().rt_trace_rays(s.handle, rays.ctypes.data, len(o), hits.ctypes.data, 0))
    iu.assert_hits(hits, want, mode)
    assert np.array_equal(hits.view(np.uint8), s.trace_rays(o, d, time=0.0).view(np.uint8))
    assert np.array_equal(hits.view(np.uint8), s.trace_rays(o, d).view(np.uint8))
    occ = np.zeros(len(o), np.uint8)
    _lib.check(_lib.lib().rt_occluded(s.handle, rays.ctypes.data, len(o), occ.ctypes.data, 0))
    assert np.array_equal(occ, want.hit.astype(np.uint8))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["lone_sphere", "lone_instance"])
def test_lone_objects(cases, mode, name):
    """A one-object list answers with the object's own rule: the moving sphere's negative roots
    included."""
    spec, comp, s = cases(name)
    s.set_traversal(mode)
    rng = np.random.default_rng(4)
    n = 300
    tau = rng.random(n).astype(F)
    centre = np.array((-0.8 * 1.5, 2.4 * 0.7, 0.6 * 1.1) if name == "lone_sphere" else (2.5, 1.0, -0.4))
    vel = np.array(mu.VEL_SPHERE if name == "lone_sphere" else mu.VEL_CHAIN)
    o = (rng.normal(size=(n, 3)) * 3).astype(F)
    target = centre + tau[:, None] * vel + rng.uniform(-0.6, 0.6, size=(n, 3))
    d = (target.astype(F) - o).astype(F)
    d[::2] = -d[::2]  # half of them point away: a sphere behind the origin has negative roots
    ref = comp.intersect(o, d, tau)
    hits = s.trace_rays(o, d, time=tau)
    iu.assert_hits(hits, ref, (mode, name))
    assert ref.hit.sum() >= 60 and (~ref.hit).sum() >= 20
    if name == "lone_sphere":
        assert (ref.t[ref.hit] < 0).sum() >= 20
    tm = np.full(n, 1e30, F)
    assert np.array_equal(s.occluded(o, d, tm, time=tau), comp.occluded(o, d, tm, tau))


@pytest.mark.parametrize("mode", MODES)
def test_scaled_and_singular_per_ray_matrices(cases, mode):
    """Moving instances under the 1e7 and 1e-3 scalings (skipped axes, all-tiny local rays); and
    the instance whose per-ray determinant is exactly 0 from time 0.5 on: missed there, hit
    before."""
    spec, comp, s = cases("scaled")
    s.set_traversal(mode)
    o, d = iu.camera_rays(17, 9)
    d2, o2 = d.copy(), o.copy()
    d2[:, 0] = F(5e-7)
    o2[:, 0] = F(2e-4)
    oo, dd = np.concatenate([o, o2]), np.concatenate([d, d2])
    tau = (np.arange(len(oo)) % 7).astype(F) / F(8)
    ref = comp.intersect(oo, dd, tau)
    iu.assert_hits(s.trace_rays(oo, dd, time=tau), ref, (mode, "scaled"))
    won = set(np.unique(ref.inst[ref.hit]).tolist())
    assert 0 in won and 2 in won and 1 not in won
    tm = np.full(len(oo), 1e30, F)
    assert np.array_equal(s.occluded(oo, dd, tm, time=tau), comp.occluded(oo, dd, tm, tau))

    spec, comp, s = cases("det_zero")
    s.set_traversal(mode)
    o, d = iu.camera_rays(33, 17)
    tm = np.full(len(o), 1e30, F)
    early = comp.intersect(o, d, 0.0)
    assert (early.inst[early.hit] == 0).sum() >= 20
    for tau in mu.DET_ZERO_TIMES:
        ref = comp.intersect(o, d, tau)
        assert not (ref.inst[ref.hit] == 0).any()
        iu.assert_hits(s.trace_rays(o, d, time=tau), ref, (mode, "det 0", tau))
        assert np.array_equal(s.occluded(o, d, tm, time=tau), comp.occluded(o, d, tm, tau))
    iu.assert_hits(s.trace_rays(o, d, time=0.0), early, (mode, "det 1"))


def test_debug_motion_inverse(cases, scene_dir):
    """The device's per-ray T(tau v) * M and inversion = the batched numpy one, entry by entry in
    bits: a rotated-and-scaled moving instance, a moving sphere under a non-uniform scaling, the
    1e-7 scaling; 256 random times and the special ones; NaNs where det == 0."""
    rng = np.random.default_rng(9)
    times = np.concatenate([rng.uniform(-1, 1, 256).astype(F), mu.SPECIAL_TIMES,
                            np.array([1e-30, 3e5, -7.25], F)])
    base = iu.scene_single()
    tiny = mu.MotionSpec(base.vertices, base.meshes, [(0, 0, iu.scaling(1e-7, 1e-7, 1e-7))],
                         materials=base.materials, velocity=[(0.25, -1.5, 3.0)]).write(scene_dir, "motion_tiny")
    comp_tiny = mu.MotionComposite(tiny)
    s_tiny = tiny.create(comp_tiny.desc.d)
    L = _lib.lib()

    def device(s, obj, tt):
        out = np.zeros((len(tt), 12), F)
        _lib.check(L.rt_debug_motion_inverse(s.handle, obj, tt.ctypes.data_as(C.POINTER(C.c_float)), len(tt),
                                             out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    spec, comp, s = cases("main")
    for what, scene, obj, fwd, vel in (
            ("instance", s, 1, spec.instances[1][2], mu.VEL_CHAIN),
            ("sphere", cases("lone_sphere")[2], 0, cases("lone_sphere")[0].sphere_xf[0], mu.VEL_SPHERE),
            ("tiny", s_tiny, 0, tiny.instances[0][2], tiny.velocity[0])):
        want, ok = mu.motion_inverse(fwd, vel, times)
        assert ok.all(), what
        assert np.array_equal(bits(device(scene, obj, times)), bits(want)), what
    # main's sphere 1 (object 4 + 1 + 1): a moving sphere under the identity
    want, ok = mu.motion_inverse(np.eye(4, dtype=F), mu.VEL_SPHERE, times)
    assert np.array_equal(bits(device(s, 6, times)), bits(want))
    dz_spec, dz_comp, dz = cases("det_zero")
    tt = np.concatenate([mu.DET_ONE_TIMES, mu.DET_ZERO_TIMES])
    got = device(dz, 0, tt)
    want, ok = mu.motion_inverse(dz_spec.instances[0][2], dz_spec.velocity[0], tt)
    assert ok.tolist() == [True] * 3 + [False] * 3
    assert np.isnan(got[3:]).all() and np.array_equal(bits(got[:3]), bits(want[:3]))
    # an object that does not move has no per-ray inverse
    assert L.rt_debug_motion_inverse(s.handle, 0, times.ctypes.data_as(C.POINTER(C.c_float)), 1,
                                     got.ctypes.data_as(C.POINTER(C.c_float))) == _lib.RT_E_INVALID
    s_tiny.close()
    comp_tiny.close()


# ---------------------------------------------------------------- radiance, films, frames
FIVE_TIMES = np.array([0.0, 0.25, 0.5, 0.8125, -0.375], F)


def shiny_reference(cases, depth, medium):
    import film_util as FU
    spec, comp, s = cases("shiny")
    key = ("shiny", depth, medium)
    if key not in _REF:
        o, d, xy = FU.pixel_centre_samples(FU.camera(spec.all_xml))
        o, d = o[::2], d[::2]
        time = FIVE_TIMES[np.arange(len(o)) % 5]  # interleaved lane by lane
        _REF[key] = (o, d, time) + mu.trace_at(comp, o, d, time, depth=depth, in_medium=medium)
    return (s,) + _REF[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("medium", [False, True])
@pytest.mark.parametrize("depth", [0, 3])
def test_radiance_depths(cases, mode, depth, medium):
    """rt_shade_rays at depth 0 and 3 on the scene with a moving mirror instance and a moving
    glass sphere, five times interleaved lane by lane: every secondary and shadow ray inherits its
    tree's time; rgb, t and the ray counters; reorder; three chunks under a scratch limit."""
    s, o, d, time, rgb, t, counts = shiny_reference(cases, depth, medium)
    assert (counts["secondary_rays"] >= 50) == (depth == 3)
    s.set_traversal(mode)
    rad, st = s.shade_rays(o, d, depth=depth, in_medium=medium, stats=True, time=time)
    assert np.array_equal(bits(rad["rgb"]), bits(rgb)), (mode, depth, medium)
    assert np.array_equal(bits(rad["t"]), bits(t)), (mode, depth, medium)
    got = {k: getattr(st, k) for k in COUNTERS}
    got["primary_hits"] = got["primary_hits"] if depth == 3 else 0
    want = dict(counts)
    want["primary_rays"] = len(o)
    assert got == want, (mode, depth, medium)
    assert np.array_equal(s.shade_rays(o, d, depth=depth, in_medium=medium, reorder=True, time=time).view(np.uint8),
                          rad.view(np.uint8))
    if depth == 3:
        per_ray = 4 * 28 * 4
        s.set_radiance_scratch_limit(per_ray * 64 * ((len(o) + 191) // 192))
        try:
            chunked = s.shade_rays(o, d, depth=depth, in_medium=medium, time=time)
        finally:
            s.set_radiance_scratch_limit(0)
        assert np.array_equal(chunked.view(np.uint8), rad.view(np.uint8))
        if not medium:  # the times matter to the picture (in a medium the first hit is not shaded)
            still = s.shade_rays(o, d, depth=depth)
            assert (bits(still["rgb"]) != bits(rad["rgb"])).any(axis=1).sum() >= 20


@pytest.mark.parametrize("mode", MODES)
def test_lit_query_on_a_timed_batch(cases, mode):
    """A lit query with one emitter record per ray: the record's shadow ray has the ray's time."""
    import film_util as FU
    import lit_util
    spec, comp, s = cases("main")
    s.set_traversal(mode)
    key = ("lit",)
    if key not in _REF:
        o, d, xy = FU.pixel_centre_samples(FU.camera(spec.all_xml))
        n = len(o)
        rng = np.random.default_rng(3)
        own = np.zeros((n, 1), ceng795_amd.LIGHT_SAMPLE_DTYPE)
        own["position"][:, 0] = np.stack([lit_util.eighths(rng, -3, 3, n), lit_util.eighths(rng, -3, 3, n),
                                          lit_util.eighths(rng, 3, 6, n)], axis=1)
        own["intensity"][:, 0] = (400, 300, 200)
        own["normal"][:, 0] = (0, 0, -1)
        time = FIVE_TIMES[np.arange(n) % 5]
        want = np.zeros((n, 4), F)
        shadow = 0
        for tau in FIVE_TIMES:
            sel = time == tau
            comp.set_time(F(tau))
            w, sh = iu.restate_lit(comp, o[sel], d[sel], own[sel])
            want[sel] = w
            shadow += sh
        _REF[key] = (o, d, own, time, want, shadow)
    o, d, own, time, want, shadow = _REF[key]
    rad, st = s.shade_rays_lit(o, d, own, scene_lights=False, stats=True, time=time)
    assert np.array_equal(bits(rad["rgb"]), bits(want[:, :3])), mode
    assert np.array_equal(bits(rad["t"]), bits(want[:, 3])), mode
    assert st.shadow_rays == shadow and shadow >= 10


@pytest.mark.parametrize("mode", MODES)
def test_film_of_timed_samples(cases, mode):
    """Film.shade_rays(time=...) on a 24 x 24 Gaussian film, 4 samples per pixel at 4 times, =
    shade_rays(time=...) + splat, and differs from the film at time 0: motion blur."""
    import film_util as FU
    spec, comp, s = cases("shiny")
    s.set_traversal(mode)
    rng = np.random.default_rng(12)
    w = h = 24
    n = w * h * 4
    xy = np.stack([np.tile(np.arange(w).repeat(4), h) + rng.random(n), np.repeat(np.arange(h), w * 4) + rng.random(n)],
                  1).astype(F)
    o = np.broadcast_to(np.array((0.2, -0.4, 6.0), F), (n, 3)).copy()
    d = np.stack([(xy[:, 0] / w - 0.5) * 6, (0.5 - xy[:, 1] / h) * 6, np.full(n, -6.0)], 1).astype(F)
    time = (np.arange(n) % 4).astype(F) / F(4)
    with ceng795_amd.Film(s, w, h) as film:
        film.shade_rays(o, d, xy, time=time)
        fused = film.accumulators()
    with ceng795_amd.Film(s, w, h) as film:
        rad = s.shade_rays(o, d, time=time)
        film.splat(xy, rad)
        assert FU.same_bits(film.accumulators(), fused)
    with ceng795_amd.Film(s, w, h) as film:
        film.shade_rays(o, d, xy)
        assert (bits(film.accumulators()) != bits(fused)).any(axis=-1).sum() >= 10
    with ceng795_amd.Film(s, w, h) as film:  # the films' flag rule: bit 16 is still unknown
        rays = ceng795_amd.pack_rays(o[:4], d[:4])
        rc = _lib.lib().rt_film_shade_rays(film._h, rays.ctypes.data, xy[:4].ctypes.data, 4, 0, 16, None)
        assert rc == _lib.RT_E_INVALID and b"flag" in _lib.lib().rt_last_error()


@pytest.mark.parametrize("mode", MODES)
def test_frames_render_at_time_zero(cases, mode):
    """rt_render and a 2 x 2 MSAA frame of the moving scene = the restatement at time 0."""
    import film_util as FU
    spec, comp, s = cases("shiny")
    s.set_traversal(mode)
    key = ("frame",)
    if key not in _REF:
        o, d, xy = FU.pixel_centre_samples(FU.camera(spec.all_xml))
        _REF[key] = (o, d) + mu.trace_at(comp, o, d, 0.0)
    o, d, rgb, t, counts = _REF[key]
    frame, st = s.render_image(0)
    assert np.array_equal(bits(frame.reshape(-1, 3)), bits(rgb)), mode
    assert {k: getattr(st, k) for k in COUNTERS} == counts
    assert np.isfinite(t).sum() >= 100

    mspec, mcomp, ms = cases("shiny_msaa")
    ms.set_traversal(mode)
    seed = 5
    key = ("msaa",)
    if key not in _REF:
        o, d, xy, (w, h, S) = FU.msaa_samples(mspec.all_xml, 0, seed)
        assert (w, h, S) == (17, 9, 4)
        rgb, _, counts = mu.trace_at(mcomp, o, d, 0.0)
        acc = FU.new_film(w, h)
        FU.splat(acc, xy, rgb)
        _REF[key] = (counts, acc)
    counts, acc = _REF[key]
    ms.set_msaa_seed(seed)
    frame, st = ms.render_image(0)
    assert FU.same_bits(frame, FU.resolve(acc)), "the MSAA frame"
    assert {k: getattr(st, k) for k in COUNTERS} == counts


# ---------------------------------------------------------------- XML, CLI, trivial descriptors
def _xml_moving(scene_dir, tag):
    import test_motion_host as host
    return iu.xml_three(scene_dir, host._moving_edit, tag=tag)


@pytest.mark.parametrize("mode", MODES)
def test_xml_scene_equals_the_descriptor_scene(scene_dir, mode):
    """Scene(xml, instanced=True, motion=True) gives, byte for byte, the records of the descriptor
    scene made from what the library reports for the file; both equal the composite."""
    path, flat = _xml_moving(scene_dir, "xml_moving_gpu")
    mesh, mat, xf = ceng795_amd.host_instances_xml(iu.xml_three(scene_dir, tag="xml_moving_plain")[0])
    vel, sxf, svel = ceng795_amd.host_motion_xml(path)
    base = iu.scene_three()
    spec = mu.MotionSpec(base.vertices, base.meshes, [(int(m), int(k), x) for m, k, x in zip(mesh, mat, xf)],
                         triangles=base.triangles, spheres=base.spheres, materials=base.materials,
                         velocity=[tuple(v) for v in vel], sphere_xf=list(sxf), sphere_vel=[tuple(v) for v in svel])
    spec.write(scene_dir, "xml_moving_desc")
    comp = mu.MotionComposite(spec)
    o, d, time = mu.main_batch(seed=8)
    ref = comp.intersect(o, d, time)
    assert ref.hit.sum() >= 100
    tm = np.where(ref.hit, np.nextafter(ref.t, F(np.inf)), F(1e30)).astype(F)
    got = []
    with ceng795_amd.Scene(path, device=0, traversal=mode, instanced=True, motion=True) as s:
        assert s.has_motion and s.num_instances == 5
        got.append((s.trace_rays(o, d, time=time), s.occluded(o, d, tm, time=time), s.render_image(0)[0]))
    with spec.create(comp.desc.d) as s:
        s.set_traversal(mode)
        got.append((s.trace_rays(o, d, time=time), s.occluded(o, d, tm, time=time), s.render_image(0)[0]))
    assert np.array_equal(got[0][0].view(np.uint8), got[1][0].view(np.uint8))
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(bits(got[0][2]), bits(got[1][2]))
    iu.assert_hits(got[0][0], ref, mode)
    assert np.array_equal(got[0][1], comp.occluded(o, d, tm, time))
    comp.close()


def test_raytracer_moving(scene_dir):
    """`raytracer --moving scene.xml` writes the frame Scene(xml, instanced=True, motion=True)
    renders."""
    path, _ = _xml_moving(scene_dir, "cli_moving")
    exe = os.path.join(os.path.dirname(os.path.abspath(ceng795_amd.__file__)), "bin", "raytracer")
    work = os.path.join(scene_dir, "cli_moving")
    os.makedirs(work, exist_ok=True)
    r = subprocess.run([exe, "--moving", path], cwd=work, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with ceng795_amd.Scene(path, device=0, instanced=True, motion=True) as s:
        frame, _ = s.render_image(0)
        name = s.camera(0).image_name
    want = os.path.join(work, "want.png")
    ceng795_amd.write_png(want, frame)
    assert open(os.path.join(work, name), "rb").read() == open(want, "rb").read()
    assert (frame.reshape(-1, 3) != 0).any(axis=1).sum() >= 10


def test_trivial_descriptor_and_static_scenes(scene_dir):
    """A NULL or trivial motion descriptor gives rt_scene_create_instanced's scene: no motion
    kernels, the same bytes in every query and frame.  On such a scene and on a flat one
    RT_QUERY_RAY_TIME with garbage in pad changes nothing."""
    spec = mu.written("still", scene_dir)
    comp = mu.MotionComposite(spec)
    o, d, time = mu.main_batch()
    garbage = np.where(np.arange(len(o)) % 2 == 0, np.nan, time * 1e6).astype(F)
    tm = np.full(len(o), 1e30, F)
    mesh, mat, xf = spec.arrays()

    def answers(s, **kw):
        return (s.trace_rays(o, d, **kw).tobytes(), s.occluded(o, d, tm, **kw).tobytes(),
                s.shade_rays(o, d, **kw).tobytes(), s.render_image(0)[0].tobytes())

    with ceng795_amd.Scene.create(comp.desc.d, instance_mesh=mesh, instance_material=mat,
                                  instance_transform=xf, device=0) as s:
        want = answers(s)
        assert not s.has_motion
        assert answers(s, time=garbage) == want
    with spec.create(comp.desc.d) as s:  # zero velocities, identity matrices
        assert not s.has_motion and s.num_instances == 4
        assert answers(s) == want and answers(s, time=garbage) == want
    inst, keep = ceng795_amd.scene._instance_desc(mesh, mat, xf)
    h = C.c_void_p()
    _lib.check(_lib.lib().rt_scene_create_moving(C.byref(comp.desc.d), C.byref(inst), None, 0, C.byref(h)))
    with ceng795_amd.Scene._from_handle(h) as s:
        assert not s.has_motion and answers(s) == want
    h = C.c_void_p()
    _lib.check(_lib.lib().rt_scene_create(C.byref(comp.desc.d), 0, C.byref(h)))
    with ceng795_amd.Scene._from_handle(h) as s:  # a flat scene
        flat = answers(s)
        assert answers(s, time=garbage) == flat
    comp.close()


def test_churn_and_refusals(cases, scene_dir):
    """Twelve create / destroy cycles; what an instanced scene refuses, a scene with motion does."""
    spec, comp, s, o, d, time, ref = main_reference(cases)
    first = None
    for k in range(12):
        with spec.create(comp.desc.d) as s2:
            got = s2.trace_rays(o[:128], d[:128], time=time[:128]).tobytes()
        first = first or got
        assert got == first
    assert not s.records_ok(0)
    hits = s.trace_rays(o[:4], d[:4], time=time[:4])
    with pytest.raises(ceng795_amd.RTError) as e:
        s.hit_attributes(o[:4], d[:4], hits)
    assert e.value.code == _lib.RT_E_UNSUPPORTED
    keep = os.path.join(scene_dir, "motion_keep.txt")
    with open(keep, "w") as f:
        f.write("keep")
    with pytest.raises(ceng795_amd.RTError) as e:
        s.dump_bvh(keep)
    assert e.value.code == _lib.RT_E_UNSUPPORTED and open(keep).read() == "keep"
    with pytest.raises(ceng795_amd.RTError) as e:
        ceng795_amd.Scene("nowhere.xml", instanced=True, motion=True, devices=[0, 0])
    assert e.value.code == _lib.RT_E_UNSUPPORTED
