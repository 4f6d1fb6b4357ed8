"""Ray queries, the part that needs no GPU: the two 32-byte records, the version symbols, the
DFS-leaf -> object table (rt_host_leaf_objects_desc) against the BVH dump, and the argument
rules of the four query entries."""
import ctypes as C

import numpy as np
import pytest

import desc_xml
import scenes
from rq_util import dump_depth, dump_leaves, object_list, write_rigged
import ceng795_amd
from ceng795_amd import _lib

NAMES = ["soup1", "hf_small", "single_sphere", "single_triangle"]


def test_record_sizes_and_versions():
    assert C.sizeof(_lib.rt_ray) == 32 and C.sizeof(_lib.rt_ray_hit) == 32
    assert ceng795_amd.RAY_DTYPE.itemsize == 32 and ceng795_amd.HIT_DTYPE.itemsize == 32
    # the numpy records lay their fields where the C structs do
    for dt, st in ((ceng795_amd.RAY_DTYPE, _lib.rt_ray), (ceng795_amd.HIT_DTYPE, _lib.rt_ray_hit)):
        for name, _ in st._fields_:
            assert dt.fields[name][1] == getattr(st, name).offset, name
    assert _lib.lib().rt_ray_query_version() == 1
    assert _lib.lib().rt_abi_version() == 7 == _lib.ABI_VERSION


def test_pack_rays_is_aligned():
    rays = ceng795_amd.pack_rays(np.zeros((5, 3)), np.ones((5, 3)), tmax=[1, 2, 3, 4, 5])
    assert rays.ctypes.data % 16 == 0 and rays.dtype == ceng795_amd.RAY_DTYPE
    assert rays["tmax"].tolist() == [1, 2, 3, 4, 5] and (rays["d"] == 1).all()
    with pytest.raises(ValueError):
        ceng795_amd.pack_rays(np.zeros((5, 3)), np.ones((4, 3)))


@pytest.mark.parametrize("name", NAMES)
def test_leaf_objects_match_the_dump(scene_dir, tmp_path, name):
    desc = desc_xml.Desc(scenes.write(name, scene_dir))
    path = str(tmp_path / "bvh.txt")
    _lib.check(_lib.lib().rt_host_dump_bvh_desc(C.byref(desc.d), path.encode()))
    with open(path) as f:
        text = f.read()
    leaves = dump_leaves(text)
    objects = object_list(desc)
    got = ceng795_amd.host_leaf_objects(desc.d)
    assert got.dtype == np.int32 and len(got) == len(leaves) == len(objects)
    assert sorted(got.tolist()) == list(range(len(leaves)))  # a permutation
    for leaf, obj in enumerate(got.tolist()):
        assert objects[obj] == leaves[leaf], (leaf, obj)
    # capacity below the leaf count: that many values, the count still returned
    few = np.full(4, -7, np.int32)
    n = _lib.lib().rt_host_leaf_objects_desc(C.byref(desc.d), few.ctypes.data_as(C.POINTER(C.c_int)),
                                             min(2, len(leaves)))
    assert n == len(leaves)
    assert few[:min(2, n)].tolist() == got[:2].tolist() and (few[2:] == -7).all()
    # the caller's own tree: the table is its bvh_leaf_object
    children, boxes, leaf_object = desc_xml.tree_from_dump(text, desc)
    desc.set_tree(children, boxes, leaf_object)
    assert ceng795_amd.host_leaf_objects(desc.d).tolist() == list(leaf_object)


def test_leaf_objects_bad_arguments():
    L = _lib.lib()
    assert L.rt_host_leaf_objects_desc(None, None, 0) == _lib.RT_E_INVALID
    d = _lib.rt_scene_desc()
    assert L.rt_host_leaf_objects_desc(C.byref(d), None, 3) == _lib.RT_E_INVALID
    assert L.rt_host_leaf_objects_desc(C.byref(d), None, 0) == _lib.RT_E_INVALID  # no objects


@pytest.mark.parametrize("fn", ["rt_trace_rays", "rt_occluded", "rt_trace_rays_device",
                                "rt_occluded_device"])
def test_argument_errors_need_no_gpu(fn):
    """n < 0, an unknown flag bit, a NULL pointer with n > 0 and a misaligned pointer are
    RT_E_INVALID before anything touches HIP (no scene exists on a machine without a GPU, and a
    NULL scene is RT_E_INVALID too)."""
    L = _lib.lib()
    f = getattr(L, fn)
    extra = (None,) if fn.endswith("_device") else ()
    rays = ceng795_amd.pack_rays(np.zeros((4, 3)), np.ones((4, 3)))
    out = np.zeros(4 * 32 + 16, np.uint8)
    out_p = out.ctypes.data + (-out.ctypes.data % 16)
    scene = C.c_void_p(None)

    def call(rp, n, op, flags):
        rc = f(scene, C.c_void_p(rp), n, C.c_void_p(op), flags, *extra)
        return rc, L.rt_last_error().decode()

    rc, msg = call(rays.ctypes.data, -1, out_p, 0)
    assert rc == _lib.RT_E_INVALID and "n < 0" in msg
    rc, msg = call(rays.ctypes.data, 4, out_p, 2)
    assert rc == _lib.RT_E_INVALID and "flag" in msg
    rc, msg = call(rays.ctypes.data, 4, out_p, ~_lib.RT_QUERY_REORDER)
    assert rc == _lib.RT_E_INVALID and "flag" in msg
    rc, msg = call(None, 4, out_p, 0)
    assert rc == _lib.RT_E_INVALID and "NULL pointer" in msg
    rc, msg = call(rays.ctypes.data, 4, None, 0)
    assert rc == _lib.RT_E_INVALID and "NULL pointer" in msg
    rc, msg = call(rays.ctypes.data + 4, 4, out_p, 0)
    assert rc == _lib.RT_E_INVALID and "aligned" in msg
    if "trace" in fn:  # the hit records too (occlusion flags are bytes)
        rc, msg = call(rays.ctypes.data, 4, out_p + 8, 0)
        assert rc == _lib.RT_E_INVALID and "aligned" in msg
    rc, msg = call(rays.ctypes.data, 4, out_p, _lib.RT_QUERY_REORDER)
    assert rc == _lib.RT_E_INVALID and "scene is NULL" in msg


def test_deep_scene_is_deeper_than_the_lane_stack(scene_dir, tmp_path):
    """The generated deep scene (rq_util.deep_scene) of the GPU tests: its reference tree has
    more levels than the 64-entry per-lane stack, by the library's own builder."""
    desc = desc_xml.Desc(write_rigged("deep", scene_dir))
    path = str(tmp_path / "bvh.txt")
    _lib.check(_lib.lib().rt_host_dump_bvh_desc(C.byref(desc.d), path.encode()))
    with open(path) as f:
        assert dump_depth(f.read()) > 64
