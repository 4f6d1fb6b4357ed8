"""Instanced scenes (rt_scene_create_instanced), the part that needs no GPU: the
composite reference the GPU tests judge by (tests/instance_util.py) against the plain oracle, the
host's inverse matrices, instance boxes and top-level order against the numpy restatement, the
argument rules and the refused combinations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ceng795_amd
import desc_xml
import instance_util as iu
from ceng795_amd import _lib
from oracle.cpu_ref import OracleScene

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "ceng795_rt.h")
SYMBOLS = ["rt_instances_version", "rt_scene_create_instanced", "rt_scene_num_instances",
           "rt_host_instance_info_desc"]
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------- the composite reference
def test_identity_composite_equals_the_plain_oracle(scene_dir):
    """With every transformation the identity the composite gives the plain oracle's t and object
    on the baked scene, for rays without -0 components (0 + -0 is +0 in the local ray)."""
    spec = iu.written("identity", scene_dir)
    comp = iu.Composite(spec)
    baked = os.path.join(scene_dir, "identity_baked.xml")
    with open(baked, "w") as f:
        f.write(spec.baked().to_xml())
    orc = OracleScene(baked)
    o1, d1 = iu.camera_rays(33, 31)
    o2, d2 = iu.random_rays(600, 5)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    assert not (np.signbit(o) & (o == 0)).any() and not (np.signbit(d) & (d == 0)).any()
    rec, shape = orc.intersect_rays(o, d)
    got = comp.intersect(o, d)
    hit = rec[:, 7] == 1.0
    assert hit.sum() >= 200 and (~hit).sum() >= 100
    assert np.array_equal(got.hit, hit)
    assert np.array_equal(bits(got.t[hit]), bits(rec[hit, 3]))
    assert np.array_equal(got.object[hit], shape[hit])
    # every kind of object wins somewhere: both instances, the triangle, the sphere
    assert set(np.unique(got.inst[hit]).tolist()) == {-1, 0, 1}
    comp.close()
    orc.close()


# ---------------------------------------------------------------- host entries
def test_version_header_and_symbols():
    assert _lib.lib().rt_instances_version() == 1
    text = open(HEADER).read()
    assert re.search(r"#define\s+CENG795_RT_HAS_INSTANCES\s+1", text)
    for name in SYMBOLS:
        assert name in text and hasattr(_lib.lib(), name), name
    assert C.sizeof(_lib.rt_instance_desc) == 40


@pytest.mark.parametrize("name", ["three", "ties", "ties_swapped", "single", "identity"])
def test_instance_info_equals_the_restatement(scene_dir, name):
    """Inverse matrices, instance boxes and top-level DFS positions equal numpy's, bit for bit."""
    spec = iu.written(name, scene_dir)
    comp = iu.Composite(spec)
    mesh, mat, xf = spec.arrays()
    inverse, box, top = ceng795_amd.host_instance_info(comp.desc.d, mesh, mat, xf)
    for i in range(len(mesh)):
        assert np.array_equal(bits(inverse[i]), bits(comp.inverse[i])), (name, i)
        assert np.array_equal(bits(box[i]), bits(comp.inst_box[i])), (name, i)
        assert top[i] == comp.top_of[i], (name, i)
    comp.close()


def test_matrix_cases():
    """The inverse of scalings (non-uniform, negative), a translation and the composed chain."""
    cases = [iu.scaling(0.7, 1.3, 0.9), iu.scaling(-1.0, 1.0, 1.2), iu.scaling(1e-7, 1e-7, 1e-7),
             iu.translation(2.5, 1.0, -0.5), iu.chain_matrix(), iu.mirror_matrix()]
    spec = iu.scene_single()
    spec.instances = [(0, 0, m) for m in cases]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        spec.write(d, "mat")
        comp = iu.Composite(spec)
        mesh, mat, xf = spec.arrays()
        inverse, box, top = ceng795_amd.host_instance_info(comp.desc.d, mesh, mat, xf)
        comp.close()
    for i, m in enumerate(cases):
        want = iu.invert_matrix(m)
        assert np.array_equal(bits(inverse[i]), bits(want)), i
        assert np.array_equal(bits(box[i]), bits(iu.apply_transform(comp.mesh_box[0], m))), i
    assert sorted(top.tolist()) == list(range(len(cases)))
    # the negative scaling has a negative determinant and still inverts
    assert np.linalg.det(cases[1].astype(np.float64)) < 0


def _call(desc, mesh, mat, xf, size=None):
    inst, keep = ceng795_amd.scene._instance_desc(mesh, mat, xf)
    if size is not None:
        inst.struct_size = size
    return _lib.lib().rt_host_instance_info_desc(C.byref(desc), C.byref(inst), None, None, None)


def test_errors(scene_dir):
    spec = iu.written("three", scene_dir)
    desc = desc_xml.Desc(spec.all_xml)
    mesh, mat, xf = spec.arrays()
    L = _lib.lib()
    assert _call(desc.d, mesh, mat, xf) == _lib.RT_OK
    singular = xf.copy()
    singular[1] = iu.scaling(1.0, 0.0, 1.0)
    assert _call(desc.d, mesh, mat, singular) == _lib.RT_E_INVALID
    assert b"not invertible" in L.rt_last_error()
    bad = mesh.copy()
    bad[2] = 2
    assert _call(desc.d, bad, mat, xf) == _lib.RT_E_INVALID
    assert b"mesh id out of range" in L.rt_last_error()
    bad = mat.copy()
    bad[0] = 3
    assert _call(desc.d, mesh, bad, xf) == _lib.RT_E_INVALID
    assert b"material id out of range" in L.rt_last_error()
    assert _call(desc.d, mesh, mat, xf, size=8) == _lib.RT_E_INVALID
    inst = _lib.rt_instance_desc()
    inst.struct_size = C.sizeof(inst)
    inst.num_instances = 2  # NULL arrays
    assert L.rt_host_instance_info_desc(C.byref(desc.d), C.byref(inst), None, None, None) == _lib.RT_E_INVALID
    assert L.rt_host_instance_info_desc(None, C.byref(inst), None, None, None) == _lib.RT_E_INVALID
    inst.num_instances = -1
    assert L.rt_host_instance_info_desc(C.byref(desc.d), C.byref(inst), None, None, None) == _lib.RT_E_INVALID
    # scene creation takes the same rules before any HIP call
    h = C.c_void_p()
    sing, keep = ceng795_amd.scene._instance_desc(mesh, mat, singular)
    assert L.rt_scene_create_instanced(C.byref(desc.d), C.byref(sing), 0, C.byref(h)) == _lib.RT_E_INVALID
    assert not h.value
    assert L.rt_scene_num_instances(None) == 0


def test_own_bvh_with_instances_is_refused(scene_dir):
    """The caller's own BVH (bvh_*) together with instances: RT_E_UNSUPPORTED."""
    spec = iu.written("three", scene_dir)
    desc = desc_xml.Desc(spec.all_xml)
    dump = os.path.join(scene_dir, "three_all.bvh")
    assert _lib.lib().rt_host_dump_bvh_desc(C.byref(desc.d), dump.encode()) == 0
    desc.set_tree(*desc_xml.tree_from_dump(open(dump).read(), desc))
    mesh, mat, xf = spec.arrays()
    assert _call(desc.d, mesh, mat, xf) == _lib.RT_E_UNSUPPORTED
    assert b"bvh_" in _lib.lib().rt_last_error()
    with pytest.raises(ceng795_amd.RTError) as e:
        ceng795_amd.Scene.create(desc.d, mesh_smooth=[1, 0], instance_mesh=mesh,
                                 instance_material=mat, instance_transform=xf)
    assert e.value.code == _lib.RT_E_UNSUPPORTED


def test_deep_top_level_is_refused():
    """A top-level tree deeper than the wave stack: 71 instances of one triangle scaled by
    2^35 .. 2^-35 (the determinants stay in fp32's range), each alone on one side of every split."""
    verts = [(1.0, 1.0, 1.0), (1.8, 1.0, 1.0), (1.0, 1.8, 1.8)]
    insts = []
    for k in range(71):
        s = 2.0 ** (35 - k)
        insts.append((0, 0, iu.scaling(s, s, s)))
    spec = iu.InstSpec(verts, [[(0, 1, 2)]], insts)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        spec.write(d, "deep")
        desc = desc_xml.Desc(spec.all_xml)
        mesh, mat, xf = spec.arrays()
        assert _call(desc.d, mesh, mat, xf) == _lib.RT_E_UNSUPPORTED
        assert b"top-level tree deeper" in _lib.lib().rt_last_error()


# ---------------------------------------------------------------- the XML dialect
def test_instances_xml_matrices(scene_dir):
    """rt_host_instances_xml: <Mesh> k is instance k, then the <MeshInstance>s; Scaling and
    Translation compositions are exact against numpy; Rotation entries are within 2^-18 (9 terms x
    (one faithful cos / sin + 3 roundings) x 2^-24 on entries <= 1)."""
    path, spec = iu.xml_three(scene_dir)
    mesh, mat, xf = ceng795_amd.host_instances_xml(path)
    assert mesh.tolist() == [0, 1, 0, 0, 1] and mat.tolist() == [0, 0, 2, 1, 0]
    assert np.array_equal(bits(xf[1]), bits(iu.translation(0.3, -2.2, 0.8)))
    want = iu.matmul(iu.translation(-2.5, 1.2, 0.3), iu.scaling(-1.0, 1.0, 1.2))  # s2 then t2
    assert np.array_equal(bits(xf[2]), bits(want))
    assert np.abs(xf[4].astype(np.float64) - iu.rotation64(30, (0, 0, 1))).max() <= 2.0 ** -18
    r2 = iu.rotation64(-75, (1, 2, -0.5))
    s1, t1 = iu.scaling(0.7, 1.3, 0.9).astype(np.float64), iu.translation(2.5, 1.0, -0.5).astype(np.float64)
    base = t1 @ iu.rotation64(30, (0, 0, 1)) @ s1
    assert np.abs(xf[0].astype(np.float64) - base).max() <= 4 * 2.0 ** -18   # entries <= 2.5
    assert np.abs(xf[3].astype(np.float64) - r2 @ base).max() <= 8 * 2.0 ** -18  # keeps mesh 1's
    assert xf[:, 3].tolist() == [[0, 0, 0, 1]] * 5
    # capacity cuts the output, not the count
    m2 = np.full(2, -7, np.int32)
    n = _lib.lib().rt_host_instances_xml(path.encode(), m2.ctypes.data_as(C.POINTER(C.c_int)), None, None, 1)
    assert n == 5 and m2.tolist() == [0, -7]


@pytest.mark.parametrize("what,old,new", [
    ("triangle", "    <Triangle id=\"1\">", "    <Triangle id=\"1\">\n      <Transformations>t1</Transformations>"),
    ("sphere", "    <Sphere id=\"1\">", "    <Sphere id=\"1\">\n      <Transformations>s1</Transformations>"),
    ("motion blur", "<MotionBlur>0 0 0</MotionBlur>", "<MotionBlur>0 0.5 0</MotionBlur>"),
    ("instance blur", "<Transformations>s2 t2</Transformations>",
     "<Transformations>s2 t2</Transformations><MotionBlur>1 0 0</MotionBlur>"),
    ("ply", "<Faces vertexOffset=", "<Faces plyFile=\"bunny.ply\" vertexOffset="),
])
def test_refused_xml_constructs(scene_dir, what, old, new):
    def edit(text):
        assert text.count(old) == 1, what
        return text.replace(old, new)
    path, _ = iu.xml_three(scene_dir, edit, tag="bad_" + what.replace(" ", "_"))
    L = _lib.lib()
    assert L.rt_host_instances_xml(path.encode(), None, None, None, 0) == _lib.RT_E_UNSUPPORTED
    assert b"not supported in instanced scenes" in L.rt_last_error()
    h = C.c_void_p()
    assert L.rt_scene_load_xml_instanced(path.encode(), 0, C.byref(h)) == _lib.RT_E_UNSUPPORTED
    assert not h.value
    # rt_scene_load_xml's own reading of such a file does not change: the flat description parses
    assert L.rt_host_instances_xml(None, None, None, None, 0) == _lib.RT_E_INVALID


def test_bad_transformation_references(scene_dir):
    for old, new in (("<Transformations>t3</Transformations>", "<Transformations>t9</Transformations>"),
                     ('baseMeshId="2"', 'baseMeshId="7"')):
        path, _ = iu.xml_three(scene_dir, lambda t: t.replace(old, new), tag="badref")
        assert _lib.lib().rt_host_instances_xml(path.encode(), None, None, None, 0) == _lib.RT_E_PARSE


# ---------------------------------------------------------------- the per-mesh culling trees
@pytest.mark.parametrize("treelets", [1, 2])
def test_check_accel_holds_per_base_mesh(scene_dir, treelets):
    """Every base mesh's culling tree passes check_accel; the stats are each mesh's own: a
    242-face height field has culling nodes, the one-face mesh has no tree at all."""
    verts, faces = iu.bumpy_mesh(12)
    base = len(verts)
    verts = verts + [(-0.5, -0.5, 0.0), (0.5, -0.5, 0.1), (0.0, 0.6, 0.2)]
    spec = iu.InstSpec(verts, [faces, [(base, base + 1, base + 2)]],
                       [(0, 0, iu.chain_matrix()), (1, 0, iu.mirror_matrix()), (0, 0, np.eye(4, dtype=F))])
    spec.write(scene_dir, f"accel{treelets}")
    desc = desc_xml.Desc(spec.all_xml)
    inst, keep = ceng795_amd.scene._instance_desc(*spec.arrays())
    stats = (C.c_longlong * 8)()
    assert _lib.lib().rt_host_check_accel_instanced_desc(C.byref(desc.d), C.byref(inst), treelets, stats) == 2
    treelets_n, nodes, depth, lone = list(stats)[:4]
    assert nodes >= 2 and depth >= 1 and 242 // treelets <= treelets_n <= 242
    assert (lone == treelets_n) == (treelets == 1)
    assert list(stats)[4:] == [0, 0, 0, 0]
    # the same tree the mesh alone gets
    alone = (C.c_longlong * 4)()
    assert _lib.lib().rt_host_check_accel_xml(spec.mesh_xml[0].encode(), treelets, alone) == 0
    assert list(alone) == list(stats)[:4]


def test_partial_instance_arguments_are_an_error(scene_dir):
    spec = iu.written("single", scene_dir)
    desc = desc_xml.Desc(spec.all_xml)
    mesh, mat, xf = spec.arrays()
    for kw in ({"instance_material": mat}, {"instance_transform": xf},
               {"instance_mesh": mesh, "instance_material": mat}):
        with pytest.raises(ValueError):
            ceng795_amd.Scene.create(desc.d, **kw)
    with pytest.raises(ceng795_amd.RTError) as e:
        ceng795_amd.Scene("nowhere.xml", instanced=True, smooth=True)
    assert e.value.code == _lib.RT_E_UNSUPPORTED


def test_xml_matrices_build_the_descriptor_scene(scene_dir):
    """The host scene of the file's instances — built from the matrices the library reports for
    it — has the inverses, boxes and top-level order of the numpy restatement over those matrices:
    what the XML loader hands to the scene build is what a descriptor caller would."""
    path, flat = iu.xml_three(scene_dir, tag="xml_host")
    mesh, mat, xf = ceng795_amd.host_instances_xml(path)
    spec = iu.scene_three()
    spec.instances = [(int(m), int(k), x) for m, k, x in zip(mesh, mat, xf)]
    spec.write(scene_dir, "xml_host_desc")
    comp = iu.Composite(spec)
    inverse, box, top = ceng795_amd.host_instance_info(comp.desc.d, mesh, mat, xf)
    for i in range(len(mesh)):
        assert np.array_equal(bits(inverse[i]), bits(comp.inverse[i])), i
        assert np.array_equal(bits(box[i]), bits(comp.inst_box[i])), i
        assert top[i] == comp.top_of[i], i
    comp.close()
