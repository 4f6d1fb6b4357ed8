"""Scenes with motion (rt_scene_create_moving), the part that needs no GPU: the ABI
surface and the argument rules, the host's expanded boxes, sphere inverses and top-level order
against the numpy restatement (tests/motion_util.py), the XML reader, the composite reference the
GPU tests judge by, and the mix of the GPU tests' ray batches."""
import collections
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ceng795_amd
import desc_xml
import instance_util as iu
import motion_util as mu
from ceng795_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ceng795_rt.h")
SYMBOLS = ["rt_motion_version", "rt_scene_create_moving", "rt_scene_load_xml_moving",
           "rt_scene_has_motion", "rt_host_motion_info_desc", "rt_host_motion_xml",
           "rt_debug_motion_inverse"]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------- ABI surface
def test_version_header_symbols_and_descriptor():
    L = _lib.lib()
    assert L.rt_motion_version() == 1
    text = open(HEADER).read()
    assert re.search(r"#define\s+CENG795_RT_HAS_MOTION\s+1", text)
    assert re.search(r"enum \{ RT_QUERY_RAY_TIME = 32 \};", text) and _lib.RT_QUERY_RAY_TIME == 32
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    D = _lib.rt_motion_desc
    assert C.sizeof(D) == 40
    assert [getattr(D, f).offset for f, _ in D._fields_] == [0, 8, 12, 16, 24, 32]
    dt = np.dtype([("struct_size", np.uint64), ("num_instances", np.int32), ("num_spheres", np.int32),
                   ("instance_velocity", np.uint64), ("sphere_transform", np.uint64),
                   ("sphere_velocity", np.uint64)])
    assert dt.itemsize == 40 and [dt.fields[f][1] for f in dt.names] == [0, 8, 12, 16, 24, 32]
    assert L.rt_scene_has_motion(None) == 0
    # rt_ray::pad is where pack_rays puts the time
    rays = ceng795_amd.pack_rays(np.zeros((3, 3)), np.ones((3, 3)), time=[0.25, 0.5, -1.0])
    assert rays["pad"].tolist() == [0.25, 0.5, -1.0]
    assert ceng795_amd.pack_rays(np.zeros((3, 3)), np.ones((3, 3)), time=0.75)["pad"].tolist() == [0.75] * 3
    assert ceng795_amd.pack_rays(np.zeros((3, 3)), np.ones((3, 3)))["pad"].tolist() == [0.0] * 3


def _aligned_bytes(n):
    raw = np.zeros(n + 16, np.uint8)
    return raw, raw.ctypes.data + (-raw.ctypes.data % 16)


def _ray_entries():
    """(name, call(flags) -> rc) of every entry that takes rt_ray, on a NULL scene / film."""
    L = _lib.lib()
    rays = ceng795_amd.pack_rays(np.zeros((4, 3)), np.ones((4, 3)))
    keep, out_p = _aligned_bytes(4 * 32)
    lights, lt_p = _aligned_bytes(4 * 48)
    xy = np.zeros((4, 2), F)
    r, o, l, x = (C.c_void_p(rays.ctypes.data), C.c_void_p(out_p), C.c_void_p(lt_p),
                  C.c_void_p(xy.ctypes.data))
    null = C.c_void_p(None)
    entries = [
        ("rt_trace_rays", lambda f: L.rt_trace_rays(null, r, 4, o, f)),
        ("rt_trace_rays_device", lambda f: L.rt_trace_rays_device(null, r, 4, o, f, None)),
        ("rt_occluded", lambda f: L.rt_occluded(null, r, 4, o, f)),
        ("rt_occluded_device", lambda f: L.rt_occluded_device(null, r, 4, o, f, None)),
        ("rt_shade_rays", lambda f: L.rt_shade_rays(null, r, 4, 0, o, f, None)),
        ("rt_shade_rays_device", lambda f: L.rt_shade_rays_device(null, r, 4, 0, o, f, None)),
        ("rt_shade_rays_lit", lambda f: L.rt_shade_rays_lit(null, r, 4, 0, l, 1, o, f, None)),
        ("rt_shade_rays_lit_device", lambda f: L.rt_shade_rays_lit_device(null, r, 4, 0, l, 1, o, f, None)),
        ("rt_film_shade_rays", lambda f: L.rt_film_shade_rays(null, r, x, 4, 0, f, None)),
        ("rt_film_shade_rays_device", lambda f: L.rt_film_shade_rays_device(null, r, x, 4, 0, f, None)),
        ("rt_film_shade_rays_lit", lambda f: L.rt_film_shade_rays_lit(null, r, x, 4, 0, l, 1, f, None)),
        ("rt_film_shade_rays_lit_device",
         lambda f: L.rt_film_shade_rays_lit_device(null, r, x, 4, 0, l, 1, f, None)),
    ]
    return entries, (rays, keep, lights, xy)


def test_ray_time_passes_every_flag_rule_and_bit_16_none():
    """RT_QUERY_RAY_TIME gets past the flag rule of every ray entry (the NULL scene or film is what
    is refused next); bit 16 is still unknown to all of them."""
    L = _lib.lib()
    entries, keep = _ray_entries()
    assert len(entries) == 12
    for name, call in entries:
        # (the film entries look at their film first: their flag rule is checked on a real film,
        # tests/test_gpu_motion.py)
        word = b"film is NULL" if "film" in name else b"flag"
        assert call(16) == _lib.RT_E_INVALID and word in L.rt_last_error(), name
        assert call(_lib.RT_QUERY_RAY_TIME | 16) == _lib.RT_E_INVALID and word in L.rt_last_error(), name
        assert call(_lib.RT_QUERY_RAY_TIME) == _lib.RT_E_INVALID, name
        msg = L.rt_last_error()
        assert b"flag" not in msg and (b"NULL" in msg or b"film" in msg), (name, msg)
        assert call(_lib.RT_QUERY_RAY_TIME | _lib.RT_QUERY_REORDER) == _lib.RT_E_INVALID, name
        assert b"flag" not in L.rt_last_error(), name


# ---------------------------------------------------------------- descriptor rules
@pytest.fixture(scope="module")
def main(scene_dir):
    spec = mu.written("main", scene_dir)
    comp = mu.MotionComposite(spec)
    yield spec, comp
    comp.close()


def _descs(spec, desc):
    inst, keep = ceng795_amd.scene._instance_desc(*spec.arrays())
    vel, xf, sv = spec.motion_arrays()
    mo, keep2 = ceng795_amd.scene._motion_desc(desc, inst, vel, xf, sv)
    return inst, mo, (keep, keep2, vel, xf, sv)


def test_invalid_descriptors_before_any_hip_call(main):
    """Every RT_E_INVALID rule, through the host-only entry and through rt_scene_create_moving
    (which then makes no scene: this runs on a machine without a GPU)."""
    spec, comp = main
    desc = comp.desc.d
    L = _lib.lib()

    def both(inst, mo, word):
        rc = L.rt_host_motion_info_desc(C.byref(desc), C.byref(inst), C.byref(mo), None, None, None, None)
        assert rc == _lib.RT_E_INVALID and word in L.rt_last_error(), (word, L.rt_last_error())
        h = C.c_void_p()
        rc = L.rt_scene_create_moving(C.byref(desc), C.byref(inst), C.byref(mo), 0, C.byref(h))
        assert rc == _lib.RT_E_INVALID and word in L.rt_last_error() and not h.value, word

    inst, mo, keep = _descs(spec, desc)
    assert L.rt_host_motion_info_desc(C.byref(desc), C.byref(inst), C.byref(mo), None, None, None, None) == 0
    mo.struct_size = 32
    both(inst, mo, b"struct_size")
    inst, mo, keep = _descs(spec, desc)
    mo.num_instances = 3
    both(inst, mo, b"num_instances")
    inst, mo, keep = _descs(spec, desc)
    mo.num_spheres = 2
    both(inst, mo, b"num_spheres")
    inst, mo, keep = _descs(spec, desc)
    mo.num_spheres = 0  # 0 goes only with NULL arrays
    both(inst, mo, b"num_spheres")
    for which, index, value in (("vel", (1, 2), np.nan), ("xf", (2, 1, 3), np.inf), ("sv", (0, 0), -np.inf)):
        inst, mo, keep = _descs(spec, desc)
        arrays = dict(vel=keep[2], xf=keep[3], sv=keep[4])
        arrays[which][index] = value
        mo2, keep2 = ceng795_amd.scene._motion_desc(desc, inst, arrays["vel"], arrays["xf"], arrays["sv"])
        both(inst, mo2, b"non-finite")
    inst, mo, keep = _descs(spec, desc)
    xf = keep[3].copy()
    xf[0] = iu.scaling(1.0, 0.0, 1.0)
    mo2, keep2 = ceng795_amd.scene._motion_desc(desc, inst, keep[2], xf, keep[4])
    both(inst, mo2, b"not invertible")
    # a NULL description; a NULL motion descriptor is no error (the instanced scene's answers)
    assert L.rt_host_motion_info_desc(None, C.byref(inst), C.byref(mo), None, None, None, None) == _lib.RT_E_INVALID
    assert L.rt_host_motion_info_desc(C.byref(desc), C.byref(inst), None, None, None, None, None) == 0
    h = C.c_void_p()
    assert L.rt_scene_create_moving(None, None, None, 0, C.byref(h)) == _lib.RT_E_INVALID
    assert L.rt_scene_load_xml_moving(None, 0, C.byref(h)) == _lib.RT_E_INVALID
    assert L.rt_debug_motion_inverse(None, 0, None, 0, None) == _lib.RT_E_INVALID


def test_own_bvh_with_motion_is_unsupported(main, scene_dir):
    spec, comp = main
    desc = desc_xml.Desc(spec.all_xml)
    dump = os.path.join(scene_dir, "motion_main_all.bvh")
    assert _lib.lib().rt_host_dump_bvh_desc(C.byref(desc.d), dump.encode()) == 0
    desc.set_tree(*desc_xml.tree_from_dump(open(dump).read(), desc))
    inst, mo, keep = _descs(spec, desc.d)
    L = _lib.lib()
    assert L.rt_host_motion_info_desc(C.byref(desc.d), C.byref(inst), C.byref(mo), None, None, None,
                                      None) == _lib.RT_E_UNSUPPORTED
    h = C.c_void_p()
    assert L.rt_scene_create_moving(C.byref(desc.d), C.byref(inst), C.byref(mo), 0,
                                    C.byref(h)) == _lib.RT_E_UNSUPPORTED and not h.value


# ---------------------------------------------------------------- host info
def _info(spec, comp):
    vel, xf, sv = spec.motion_arrays()
    kw = {}
    if spec.instances:
        mesh, mat, m = spec.arrays()
        kw = dict(instance_mesh=mesh, instance_material=mat, instance_transform=m)
    return ceng795_amd.host_motion_info(comp.desc.d, instance_velocity=vel if spec.instances else None,
                                        sphere_transform=xf if spec.spheres else None,
                                        sphere_velocity=sv if spec.spheres else None, **kw)


def _assert_info(spec, comp, what):
    inst_box, sph_inv, sph_box, top = _info(spec, comp)
    for i in range(len(spec.instances)):
        assert np.array_equal(bits(inst_box[i]), bits(comp.inst_box[i])), (what, i)
    for k in range(len(spec.spheres)):
        assert np.array_equal(bits(sph_inv[k]), bits(comp.sphere_inverse[k])), (what, k)
        assert np.array_equal(bits(sph_box[k]), bits(comp.sphere_box[k])), (what, k)
    assert top.tolist() == [comp.top_of[o] for o in range(len(top))], what
    return top


@pytest.mark.parametrize("name", ["main", "lone_sphere", "lone_instance", "scaled", "det_zero", "shiny"])
def test_motion_info_equals_the_restatement(scene_dir, name):
    """Expanded instance boxes, sphere inverses and boxes and the top-level DFS position of every
    object equal numpy's, bit for bit."""
    spec = mu.written(name, scene_dir)
    comp = mu.MotionComposite(spec)
    _assert_info(spec, comp, name)
    comp.close()


def test_motion_info_cases(scene_dir):
    """Non-uniform, negative and 1e-7 scalings under a velocity; a velocity along y, which moves a
    median split of the top-level tree (another DFS order), and one along z, which does not; a
    velocity with a -0 component; the velocity (-0, -0, -0), which is no velocity."""
    base = iu.scene_three()
    mats = [iu.scaling(0.7, 1.3, 0.9), iu.scaling(-1.0, 1.0, 1.2), iu.scaling(1e-7, 1e-7, 1e-7), iu.chain_matrix()]
    tops = {}
    for tag, vel in (("y", [(0, 6.0, 0), None, None, None]), ("z", [(0, 0, 6.0), None, None, None]),
                     ("none", [None] * 4), ("negzero", [(-0.0, 0.5, -0.0), (0.0, -0.0, 0.25), None, (-0.0, -0.0, -0.0)])):
        spec = mu.MotionSpec(base.vertices, base.meshes, [(0, k % 3, m) for k, m in enumerate(mats)],
                             triangles=base.triangles, spheres=base.spheres, materials=base.materials,
                             velocity=vel, sphere_xf=[iu.scaling(-2.0, 0.5, 1e-7)],
                             sphere_vel=[(0.0, -0.0, 3.0)])
        spec.write(scene_dir, "motion_case_" + tag)
        comp = mu.MotionComposite(spec)
        tops[tag] = _assert_info(spec, comp, tag).tolist()
        if tag == "negzero":
            plain = iu.apply_transform(comp.mesh_box[0], mats[3])
            assert np.array_equal(bits(comp.inst_box[3]), bits(plain))  # -0 == 0: not expanded
            assert not np.array_equal(bits(comp.inst_box[0]), bits(iu.apply_transform(comp.mesh_box[0], mats[0])))
        comp.close()
    assert tops["y"] != tops["none"] and tops["z"] == tops["none"]


def test_trivial_descriptor_gives_the_instanced_answers(scene_dir):
    spec = mu.written("still", scene_dir)
    comp = mu.MotionComposite(spec)
    plain = iu.Composite(spec)
    inst_box, sph_inv, sph_box, top = _info(spec, comp)
    mesh, mat, xf = spec.arrays()
    inverse, box, itop = ceng795_amd.host_instance_info(comp.desc.d, mesh, mat, xf)
    assert np.array_equal(bits(inst_box), bits(box)) and top[:len(mesh)].tolist() == itop.tolist()
    assert all(np.array_equal(bits(m), bits(np.eye(4, dtype=F))) for m in sph_inv)
    # the composite with nothing moving equals instance_util's in every field
    o, d, time = mu.main_batch()
    a, b = comp.intersect(o, d, time), plain.intersect(o, d)
    assert a.hit.sum() >= 200
    for name in ("hit", "object", "material", "leaf", "inst", "top"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(bits(a.t), bits(b.t)) and np.array_equal(bits(a.normal), bits(b.normal))
    tm = np.full(len(o), 1e30, F)
    assert np.array_equal(comp.occluded(o, d, tm, time), plain.occluded(o, d, tm))
    comp.close()
    plain.close()


# ---------------------------------------------------------------- the restatement itself
def test_batched_inverse_equals_the_scalar_one():
    rng = np.random.default_rng(1)
    m = rng.normal(size=(200, 16)).astype(F)
    m[:20, 12:] = (0, 0, 0, 1)
    m[20] = iu.scaling(1.0, 0.0, 1.0).reshape(16)
    inv, ok = mu.invert_batch(m)
    for k in range(len(m)):
        want = iu.invert_matrix(m[k])
        assert (want is None) == (not ok[k])
        if want is not None:
            assert np.array_equal(bits(inv[k]), bits(want.reshape(16))), k
    assert not ok[20] and np.isnan(inv[20]).all()
    # the product with the translation written out equals Matrix4x4::operator*
    fwd, vel = iu.chain_matrix(), np.array(mu.VEL_CHAIN, F)
    tau = np.array([0.0, 0.37, -1.0, 1.5], F)
    got = mu.motion_matrix(fwd, vel, tau)
    for k, t in enumerate(tau):
        delta = (t * vel).astype(F)
        assert np.array_equal(bits(got[k]), bits(iu.matmul(iu.translation(*delta), fwd).reshape(16))), k
    # scene_det_zero's determinants: 1 at the early times, exactly 0 later
    spec = mu.scene_det_zero()
    m, v = spec.instances[0][2], spec.velocity[0]
    assert mu.motion_inverse(m, v, mu.DET_ONE_TIMES)[1].all()
    assert not mu.motion_inverse(m, v, mu.DET_ZERO_TIMES)[1].any()
    assert iu.invert_matrix(m) is not None


# ---------------------------------------------------------------- XML
def _moving_edit(text):
    text = text.replace("<MotionBlur>0 0 0</MotionBlur>", "<MotionBlur>-0.4 0.3 -0</MotionBlur>")  # mesh 2
    text = text.replace("<Transformations>s1 r1 t1</Transformations>",
                        "<Transformations>s1 r1 t1</Transformations>\n      <MotionBlur>0.8 -0.5 0.3</MotionBlur>")
    text = text.replace("<Transformations>r2</Transformations>",
                        "<Transformations>r2</Transformations>\n      <MotionBlur>0 0 2</MotionBlur>")
    return text.replace('    <Sphere id="1">', '    <Sphere id="1">\n      <Transformations>s1 t3</Transformations>'
                        '\n      <MotionBlur>0.6 0.9 -0.4</MotionBlur>')


def test_motion_xml(scene_dir):
    """<MotionBlur> on a mesh, on an instance (its own, not its base's) and on a sphere with
    <Transformations>; the instanced loader still refuses the file and reads the plain one as
    before."""
    path, spec = iu.xml_three(scene_dir, _moving_edit, tag="xml_moving")
    vel, xf, sv = ceng795_amd.host_motion_xml(path)
    # instances: mesh 1, mesh 2, instance of 1 (reset), instance of 1 (keeps), instance of 2
    assert vel.tolist() == np.array([(0.8, -0.5, 0.3), (-0.4, 0.3, -0.0), (0, 0, 0), (0, 0, 2), (0, 0, 0)], F).tolist()
    assert np.signbit(vel[1, 2])
    assert sv.tolist() == np.array([(0.6, 0.9, -0.4)], F).tolist()
    want = iu.matmul(iu.translation(0.3, -2.2, 0.8), iu.scaling(0.7, 1.3, 0.9))  # s1 then t3
    assert xf.shape == (1, 4, 4) and np.array_equal(bits(xf[0]), bits(want))
    L = _lib.lib()
    assert L.rt_host_instances_xml(path.encode(), None, None, None, 0) == _lib.RT_E_UNSUPPORTED
    plain, _ = iu.xml_three(scene_dir, tag="xml_plain")
    mesh, mat, m = ceng795_amd.host_instances_xml(plain)
    vel0, xf0, sv0 = ceng795_amd.host_motion_xml(plain)
    assert not vel0.any() and not sv0.any() and np.array_equal(xf0[0], np.eye(4, dtype=F))
    assert len(vel0) == len(mesh) == 5

    def tri(text):
        return _moving_edit(text).replace('    <Triangle id="1">',
                                          '    <Triangle id="1">\n      <Transformations>t1</Transformations>')
    bad, _ = iu.xml_three(scene_dir, tri, tag="xml_moving_tri")
    assert L.rt_host_motion_xml(bad.encode(), None, None, None, 0, None) == _lib.RT_E_UNSUPPORTED
    h = C.c_void_p()
    assert L.rt_scene_load_xml_moving(bad.encode(), 0, C.byref(h)) == _lib.RT_E_UNSUPPORTED and not h.value


# ---------------------------------------------------------------- the GPU batches' mix
def test_main_batch_mix(main):
    """What test_gpu_motion.py relies on, from the composite alone: every kind of winner on >= 8
    rays, >= 100 rays whose winner at their own time differs from the one at time 0 (a library
    that ignores the time fails), >= 8 rays that miss a moving object only at its box."""
    spec, comp = main
    o, d, time = mu.main_batch()
    ref = comp.intersect(o, d, time)
    kinds = collections.Counter(comp.winner_kind(ref).tolist())
    for kind in ("moving_instance", "static_instance", "moving_sphere", "placed_sphere", "sphere",
                 "triangle", "miss"):
        assert kinds[kind] >= 8, (kind, kinds)
    still = comp.intersect(o, d, np.zeros(len(o), F))
    differ = (ref.hit != still.hit) | (ref.top != still.top) | (bits(ref.t) != bits(still.t))
    assert differ.sum() >= 100, differ.sum()
    assert mu.missed_at_the_box(comp, o, d, time).sum() >= 8
    # occlusion follows the time too
    big = np.full(len(o), 1e30, F)
    assert (comp.occluded(o, d, big, time) != comp.occluded(o, d, big, np.zeros(len(o), F))).sum() >= 30


def test_bench_tool_moving_dry_run():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ray_query_bench.py"),
                          "--instances", "4", "--moving", "--dry-run"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "moving" in out.stdout and "instances=4" in out.stdout.replace(" ", "")
