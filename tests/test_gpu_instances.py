"""Instanced scenes on the GPU (rt_scene_create_instanced): closest hits and
occlusion through the two-level walk against the composite reference (tests/instance_util.py), bit
for bit, in both traversal modes."""
import numpy as np
import pytest

import ceng795_amd
import instance_util as iu
from ceng795_amd import _lib

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ["fast", "reference"]


@pytest.fixture(scope="module")
def cases(scene_dir):
    """name -> (spec, composite, scene), made once; the references are computed per test from the
    composite and never changed."""
    made = {}

    def get(name):
        if name not in made:
            spec = iu.written(name, scene_dir)
            comp = iu.Composite(spec)
            mesh, mat, xf = spec.arrays()
            s = ceng795_amd.Scene.create(comp.desc.d, instance_mesh=mesh, instance_material=mat,
                                         instance_transform=xf, device=0)
            made[name] = (spec, comp, s)
        return made[name]
    yield get
    for spec, comp, s in made.values():
        s.close()
        comp.close()


def rays_for(name):
    o1, d1 = iu.camera_rays(17, 9)
    o2, d2 = iu.random_rays(200, 11 + len(name))
    # ... and at the instance under the composed matrix, which every test scene has
    rng = np.random.default_rng(len(name))
    o3 = (rng.normal(size=(150, 3)) * 4).astype(F)
    d3 = ((np.array([2.5, 1.0, -0.4]) + rng.uniform(-0.7, 0.7, size=(150, 3))).astype(F) - o3).astype(F)
    return np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])


def check_closest(s, comp, o, d, what, **kw):
    ref = comp.intersect(o, d)
    hits = s.trace_rays(o, d, **kw)
    iu.assert_hits(hits, ref, what)
    return hits, ref


@pytest.mark.parametrize("mode", MODES)
def test_three_closest_and_occlusion(cases, mode):
    """Scene "three": every kind of object wins somewhere; t bits, object, material, instance,
    leaf and normal; occlusion with tmax at, just below and just above the hit's t."""
    spec, comp, s = cases("three")
    s.set_traversal(mode)
    assert s.num_instances == 4
    o, d = rays_for("three")
    hits, ref = check_closest(s, comp, o, d, mode)
    assert set(np.unique(ref.inst[ref.hit]).tolist()) == {-1, 0, 1, 2, 3}
    assert (~ref.hit).sum() >= 20
    h = ref.hit
    t = ref.t[h]
    for tmax, want in ((t, 0), (np.nextafter(t, F(0)), 0), (np.nextafter(t, F(np.inf)), 1)):
        occ = s.occluded(o[h], d[h], tmax)
        assert np.array_equal(occ, comp.occluded(o[h], d[h], tmax)), mode
        assert (occ == want).all(), mode
    big = np.full(len(o), 1e30, F)
    assert np.array_equal(s.occluded(o, d, big), ref.hit.astype(np.uint8)), mode
    assert np.array_equal(s.occluded(o, d, big), comp.occluded(o, d, big)), mode
    assert not s.occluded(o, d, np.zeros(len(o), F)).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,first", [("ties", 1), ("ties_swapped", 2)])
def test_ties_take_the_earlier_top_level_leaf(cases, mode, name, first):
    """Two instances with one matrix: every hit on them ties in t; the earlier top-level DFS
    leaf wins, whichever material it carries."""
    spec, comp, s = cases(name)
    s.set_traversal(mode)
    o, d = rays_for(name)
    hits, ref = check_closest(s, comp, o, d, (mode, name))
    on = ref.hit & (ref.inst >= 0)
    assert on.sum() >= 30
    early = min((0, 1), key=lambda i: comp.top_of[i])
    assert (hits["pad"][on] == early).all()
    assert (hits["material"][on] == spec.instances[early][1]).all()
    assert spec.instances[0][1] == first


@pytest.mark.parametrize("mode", MODES)
def test_single_instance_list(cases, mode):
    spec, comp, s = cases("single")
    s.set_traversal(mode)
    o, d = rays_for("single")
    hits, ref = check_closest(s, comp, o, d, mode)
    assert ref.hit.sum() >= 30 and (~ref.hit).sum() >= 30
    big = np.full(len(o), 1e30, F)
    assert np.array_equal(s.occluded(o, d, big), comp.occluded(o, d, big))


@pytest.mark.parametrize("mode", MODES)
def test_rays_inside_boxes_and_meshes(cases, mode):
    """Origins inside an instance's box and between the mesh's faces, in every direction."""
    spec, comp, s = cases("three")
    s.set_traversal(mode)
    rng = np.random.default_rng(2)
    n = 256
    centre = np.array([(0.0, 0.0, 0.15), (2.5, 1.0, -0.4), (-2.5, 1.2, 0.45), (0.3, -2.2, 0.9)], F)
    o = (centre[rng.integers(0, 4, n)] + rng.normal(size=(n, 3)) * 0.2).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    hits, ref = check_closest(s, comp, o, d, mode)
    assert ref.hit.sum() >= 60
    tm = np.full(n, 1e30, F)
    assert np.array_equal(s.occluded(o, d, tm), comp.occluded(o, d, tm))


@pytest.mark.parametrize("mode", MODES)
def test_skipped_axes_and_tiny_local_rays(cases, mode):
    """World directions with a skipped axis (|d_i| < 1e-6) that the rotation un-skips locally;
    under the 1e7 scalings the reverse, and the all-tiny local ray, which misses its instance."""
    spec, comp, s = cases("three")
    s.set_traversal(mode)
    k = np.arange(120)
    o = np.stack([-3.5 + 7.0 * (k % 12) / 11, -3.0 + 6.0 * (k // 12) / 9, np.full(120, 2.5)], 1).astype(F)
    d = np.tile(np.array([[0.4, 0.0, -1.0], [-0.3, 1e-7, -1.0], [-5e-7, 0.35, -1.0]], F), (40, 1))
    assert (np.abs(d) < iu.EPS).any(axis=1).all()
    lo, ld = comp.local_rays(1, o, d)
    assert not (np.abs(ld) < iu.EPS).any()  # the rotation un-skips the axis locally
    hits, ref = check_closest(s, comp, o, d, mode)
    assert ref.hit.sum() >= 30 and {0, 1, 2} <= set(np.unique(ref.inst[ref.hit]).tolist())

    spec, comp, s = cases("scaled")
    s.set_traversal(mode)
    o, d = iu.camera_rays(17, 9)
    lo, ld = comp.local_rays(0, o, d)
    assert (np.abs(ld[:, 0]) < iu.EPS).all() and not (np.abs(d[:, 0]) < iu.EPS).all()
    lo, ld = comp.local_rays(1, o, d)
    assert (np.abs(ld) < iu.EPS).all()  # all-tiny: no valid query ray
    d2 = d.copy()
    d2[:, 0] = F(5e-7)  # skipped in the world, 5e-4 locally under the 1e-3 scaling
    o2 = o.copy()
    o2[:, 0] = F(2e-4)  # inside the squeezed instance's x range
    lo, ld = comp.local_rays(2, o2, d2)
    assert (np.abs(d2[:, 0]) < iu.EPS).all() and not (np.abs(ld[:, 0]) < iu.EPS).any()
    oo, dd = np.concatenate([o, o2]), np.concatenate([d, d2])
    hits, ref = check_closest(s, comp, oo, dd, (mode, "scaled"))
    won = set(np.unique(ref.inst[ref.hit]).tolist())
    assert 0 in won and 2 in won and 1 not in won
    tm = np.full(len(oo), 1e30, F)
    assert np.array_equal(s.occluded(oo, dd, tm), comp.occluded(oo, dd, tm))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [50, 114])
def test_mixed_waves_invalid_rays_and_reorder(cases, mode, n):
    """Batches whose lanes hit different instances, shuffled so that one wave mixes them all, with
    invalid rays between valid ones; RT_QUERY_REORDER gives identical records."""
    spec, comp, s = cases("three")
    s.set_traversal(mode)
    o, d = rays_for("three")
    ref = comp.intersect(o, d)
    rng = np.random.default_rng(n)
    pick = np.concatenate([rng.choice(np.flatnonzero(ref.hit & (ref.inst == i)), n // 6) for i in (0, 1, 2, 3, -1)]
                          + [rng.choice(np.flatnonzero(~ref.hit), n - 5 * (n // 6))])
    rng.shuffle(pick)
    o, d = o[pick].copy(), d[pick].copy()
    bad = np.arange(3, n, 7)
    d[bad[0::3]] = 0.0
    d[bad[1::3], 1] = np.nan
    o[bad[2::3], 2] = np.inf
    hits, ref = check_closest(s, comp, o, d, (mode, n))
    assert not ref.hit[bad].any() and len(set(ref.inst[ref.hit][:64].tolist())) == 5
    again = s.trace_rays(o, d, reorder=True)
    assert np.array_equal(hits.view(np.uint8), again.view(np.uint8))
    tm = np.where(ref.hit, np.nextafter(ref.t, F(np.inf)), F(1e30)).astype(F)
    occ = s.occluded(o, d, tm)
    assert np.array_equal(occ, comp.occluded(o, d, tm))
    assert np.array_equal(occ, s.occluded(o, d, tm, reorder=True))
    assert np.array_equal(occ, ref.hit.astype(np.uint8))


def test_modes_agree_and_flat_tree_entries_are_refused(cases):
    spec, comp, s = cases("three")
    o, d = rays_for("three")
    s.set_traversal("fast")
    a = s.trace_rays(o, d)
    s.set_traversal("reference")
    b = s.trace_rays(o, d)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # like a smooth scene: no pixel records; and nothing that reads the flat tree
    assert not s.records_ok(0)
    with pytest.raises(ceng795_amd.RTError) as e:
        s.hit_attributes(o[:4], d[:4], a[:4])
    assert e.value.code == _lib.RT_E_UNSUPPORTED


# ---------------------------------------------------------------- radiance, films, frames
COUNTERS = ("primary_rays", "primary_hits", "shadow_rays", "secondary_rays")
_REF = {}  # restated answers, computed once and left unchanged


def shiny_reference(cases, depth, medium):
    import film_util as FU
    spec, comp, s = cases("shiny")
    key = ("shiny", depth, medium)
    if key not in _REF:
        o, d, xy = FU.pixel_centre_samples(FU.camera(spec.all_xml))
        _REF[key] = (o, d, xy) + iu.trace(comp, o, d, depth=depth, in_medium=medium)
    return (s,) + _REF[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("medium", [False, True])
@pytest.mark.parametrize("depth", [0, 3])
def test_radiance_depths(cases, mode, depth, medium):
    """rt_shade_rays at depth 0 and at the scene's maximum on the scene with a mirror and a glass
    instance, 33 x 31, with and without RT_QUERY_IN_MEDIUM: rgb, t and the ray counters."""
    s, o, d, xy, rgb, t, counts = shiny_reference(cases, depth, medium)
    assert len(o) == 33 * 31 and (counts["secondary_rays"] >= 100) == (depth == 3)
    s.set_traversal(mode)
    rad, st = s.shade_rays(o, d, depth=depth, in_medium=medium, stats=True)
    assert np.array_equal(bits(rad["rgb"]), bits(rgb)), (mode, depth, medium)
    assert np.array_equal(bits(rad["t"]), bits(t)), (mode, depth, medium)
    got = {k: getattr(st, k) for k in COUNTERS}
    # (the library counts every first hit; the restatement only those at the scene's depth)
    got["primary_hits"] = got["primary_hits"] if depth == 3 else 0
    assert got == counts, (mode, depth, medium)
    assert np.array_equal(s.shade_rays(o, d, depth=depth, in_medium=medium, reorder=True).view(np.uint8),
                          rad.view(np.uint8))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["three", "ties", "single", "scaled", "shiny"])
def test_render_equals_shade_rays_of_the_camera_rays(cases, mode, name):
    """rt_render of each scene is rt_shade_rays of its camera's rays, and both are the
    restatement's; the frame's ray counters are the query's."""
    import film_util as FU
    spec, comp, s = cases(name)
    s.set_traversal(mode)
    o, d, xy = FU.pixel_centre_samples(FU.camera(spec.all_xml))
    frame, fst = s.render_image(0)
    rad, st = s.shade_rays(o, d, stats=True)
    assert np.array_equal(bits(frame.reshape(-1, 3)), bits(rad["rgb"])), (mode, name)
    assert {k: getattr(fst, k) for k in COUNTERS} == {k: getattr(st, k) for k in COUNTERS}
    key = ("frame", name)
    if key not in _REF:
        _REF[key] = iu.trace(comp, o, d)
    rgb, t, counts = _REF[key]
    assert np.array_equal(bits(rad["rgb"]), bits(rgb)) and np.array_equal(bits(rad["t"]), bits(t))
    assert {k: getattr(st, k) for k in COUNTERS} == counts
    assert np.isfinite(t).sum() >= 5


@pytest.mark.parametrize("mode", MODES)
def test_msaa_frame_and_films(cases, mode):
    """A 2 x 2-sample MSAA frame equals the film fed with the reference's samples; and
    rt_film_shade_rays equals the splat of rt_shade_rays."""
    import film_util as FU
    spec, comp, s = cases("shiny_msaa")
    s.set_traversal(mode)
    seed = 5
    key = ("msaa",)
    if key not in _REF:
        o, d, xy, (w, h, S) = FU.msaa_samples(spec.all_xml, 0, seed)
        assert (w, h, S) == (17, 9, 4)
        rgb, _, counts = iu.trace(comp, o, d)
        acc = FU.new_film(w, h)
        FU.splat(acc, xy, rgb)
        _REF[key] = (o, d, xy, w, h, counts, acc)
    o, d, xy, w, h, counts, acc = _REF[key]
    s.set_msaa_seed(seed)
    frame, st = s.render_image(0)
    assert FU.same_bits(frame, FU.resolve(acc)), "the MSAA frame"
    assert {k: getattr(st, k) for k in COUNTERS} == counts
    with ceng795_amd.Film(s, w, h) as film:
        film.shade_rays(o, d, xy)
        assert FU.same_bits(film.accumulators(), acc)
        assert FU.same_bits(film.resolve(), FU.resolve(acc))
    with ceng795_amd.Film(s, w, h) as film:  # the fused entry = the splat of the query's colours
        rad = s.shade_rays(o, d)
        film.splat(xy, rad)
        assert FU.same_bits(film.accumulators(), acc)


@pytest.mark.parametrize("mode", MODES)
def test_lit_query_with_an_emitter_record(cases, mode):
    """A lit query: the scene's lights dark, every ray with one emitter record of its own."""
    import film_util as FU
    import lit_util
    spec, comp, s = cases("three")
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
        _REF[key] = (o, d, own) + iu.restate_lit(comp, o, d, own)
    o, d, own, want, shadow = _REF[key]
    rad, st = s.shade_rays_lit(o, d, own, scene_lights=False, stats=True)
    assert np.array_equal(bits(rad["rgb"]), bits(want[:, :3])), mode
    assert np.array_equal(bits(rad["t"]), bits(want[:, 3])), mode
    assert st.shadow_rays == shadow and shadow >= 10


def test_empty_descriptor_is_the_flat_scene(scene_dir):
    """A NULL or empty instance descriptor gives rt_scene_create's scene: the same records."""
    import ctypes as C
    spec = iu.written("identity", scene_dir)
    comp = iu.Composite(spec)
    o, d = rays_for("identity")
    got = []
    for inst in (None, _lib.rt_instance_desc(struct_size=C.sizeof(_lib.rt_instance_desc))):
        h = C.c_void_p()
        ceng795_amd._lib.check(_lib.lib().rt_scene_create_instanced(
            C.byref(comp.desc.d), None if inst is None else C.byref(inst), 0, C.byref(h)))
        with ceng795_amd.Scene._from_handle(h) as s:
            assert s.num_instances == 0
            got.append(s.trace_rays(o, d))
    h = C.c_void_p()
    ceng795_amd._lib.check(_lib.lib().rt_scene_create(C.byref(comp.desc.d), 0, C.byref(h)))
    with ceng795_amd.Scene._from_handle(h) as s:
        flat = s.trace_rays(o, d)
    comp.close()
    for g in got:
        assert np.array_equal(g.view(np.uint8), flat.view(np.uint8))


@pytest.mark.parametrize("mode", MODES)
def test_xml_scene_equals_the_descriptor_scene(scene_dir, mode):
    """Scene(xml, instanced=True) gives the records of the descriptor scene made from the matrices
    the library reports for the file (vertexOffset, resetTransform and the inherited base
    transformation included), and both equal the composite over those matrices."""
    path, flat = iu.xml_three(scene_dir)
    mesh, mat, xf = ceng795_amd.host_instances_xml(path)
    spec = iu.scene_three()
    spec.instances = [(int(m), int(k), x) for m, k, x in zip(mesh, mat, xf)]
    spec.write(scene_dir, "xml_three_desc")
    comp = iu.Composite(spec)
    o, d = rays_for("three")
    ref = comp.intersect(o, d)
    assert set(np.unique(ref.inst[ref.hit]).tolist()) >= {-1, 0, 1, 2, 3}
    tm = np.where(ref.hit, np.nextafter(ref.t, F(np.inf)), F(1e30)).astype(F)
    got = []
    with ceng795_amd.Scene(path, device=0, traversal=mode, instanced=True) as s:
        assert s.num_instances == 5
        got.append((s.trace_rays(o, d), s.occluded(o, d, tm)))
    with ceng795_amd.Scene.create(comp.desc.d, instance_mesh=mesh, instance_material=mat,
                                  instance_transform=xf, device=0) as s:
        s.set_traversal(mode)
        got.append((s.trace_rays(o, d), s.occluded(o, d, tm)))
    assert np.array_equal(got[0][0].view(np.uint8), got[1][0].view(np.uint8))
    assert np.array_equal(got[0][1], got[1][1])
    iu.assert_hits(got[0][0], ref, mode)
    assert np.array_equal(got[0][1], comp.occluded(o, d, tm))
    comp.close()


def test_empty_descriptor_dumps_the_flat_tree(scene_dir):
    """A scene made with an empty instance descriptor dumps rt_host_dump_bvh_desc's tree."""
    import ctypes as C
    import os
    import desc_xml
    spec = iu.written("identity", scene_dir)
    desc = desc_xml.Desc(spec.all_xml)
    want = os.path.join(scene_dir, "identity_host.bvh")
    assert _lib.lib().rt_host_dump_bvh_desc(C.byref(desc.d), want.encode()) == 0
    inst = _lib.rt_instance_desc(struct_size=C.sizeof(_lib.rt_instance_desc))
    h = C.c_void_p()
    _lib.check(_lib.lib().rt_scene_create_instanced(C.byref(desc.d), C.byref(inst), 0, C.byref(h)))
    with ceng795_amd.Scene._from_handle(h) as s:
        got = os.path.join(scene_dir, "identity_empty.bvh")
        s.dump_bvh(got)
    assert open(got).read() == open(want).read() and len(open(want).read()) > 1000


def test_dump_of_an_instanced_scene_leaves_the_file_alone(cases, scene_dir):
    import os
    spec, comp, s = cases("three")
    path = os.path.join(scene_dir, "keep.txt")
    with open(path, "w") as f:
        f.write("keep")
    with pytest.raises(ceng795_amd.RTError) as e:
        s.dump_bvh(path)
    assert e.value.code == _lib.RT_E_UNSUPPORTED and open(path).read() == "keep"


def test_raytracer_instanced(scene_dir):
    """`raytracer --instanced scene.xml` writes the frame Scene(xml, instanced=True) renders."""
    import os
    import subprocess
    path, _ = iu.xml_three(scene_dir, tag="cli_three")
    exe = os.path.join(os.path.dirname(os.path.abspath(ceng795_amd.__file__)), "bin", "raytracer")
    work = os.path.join(scene_dir, "cli")
    os.makedirs(work, exist_ok=True)
    r = subprocess.run([exe, "--instanced", path], cwd=work, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    with ceng795_amd.Scene(path, device=0, instanced=True) as s:
        frame, _ = s.render_image(0)
        name = s.camera(0).image_name
    want = os.path.join(work, "want.png")
    ceng795_amd.write_png(want, frame)
    assert open(os.path.join(work, name), "rb").read() == open(want, "rb").read()
    assert (frame.reshape(-1, 3) != 0).any(axis=1).sum() >= 10
    r = subprocess.run([exe, "--instanced", "--smooth", path], cwd=work, capture_output=True, text=True)
    assert r.returncode == 1 and "--instanced" in r.stderr
