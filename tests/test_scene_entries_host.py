"""The twelve scene-creation entries (rt_scene_create* / rt_scene_load_xml*), the
part that needs no GPU: every argument and description check, and the whole host build, come before
the first HIP call.  So a bad argument, a bad description and a bad file are reported as such even
with a device that cannot be resolved: device -1 (the current one) where there is no GPU, device
id -1 in a multi-device list anywhere.  No case creates a scene, with or without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import ceng795_amd
import desc_xml
import instance_util as iu
from ceng795_amd import _lib

CREATE = ["rt_scene_create", "rt_scene_create_multi", "rt_scene_create_surface",
          "rt_scene_create_textured", "rt_scene_create_instanced", "rt_scene_create_moving"]
LOAD = ["rt_scene_load_xml", "rt_scene_load_xml_multi", "rt_scene_load_xml_surface",
        "rt_scene_load_xml_textured", "rt_scene_load_xml_instanced", "rt_scene_load_xml_moving"]


class Given:
    """Scene "three" (53 leaves: two meshes, a triangle, a sphere) with valid descriptors of every
    kind beside it: flat meshes, three instances, one of them moving."""

    def __init__(self, scene_dir):
        spec = iu.written("three", scene_dir)
        self.xml = spec.all_xml
        self.desc = desc_xml.Desc(self.xml)
        self.smooth = (C.c_ubyte * self.desc.d.num_meshes)()
        self.surface = _lib.rt_surface_desc(C.sizeof(_lib.rt_surface_desc), self.smooth, None, None)
        self.inst, self.keep = ceng795_amd.scene._instance_desc(*spec.arrays())
        self.velocity = np.zeros(3 * self.inst.num_instances, np.float32)
        self.velocity[1] = 0.5
        self.motion = _lib.rt_motion_desc(C.sizeof(_lib.rt_motion_desc), self.inst.num_instances, 0,
                                          self.velocity.ctypes.data_as(C.POINTER(C.c_float)), None, None)


def call(entry, first, device, out, g):
    """`entry` with `first` as its description or path, on `device`, the other arguments valid."""
    L = _lib.lib()
    ids = (C.c_int * 1)(device)
    return {
        "rt_scene_create": lambda: L.rt_scene_create(first, device, out),
        "rt_scene_create_multi": lambda: L.rt_scene_create_multi(first, 1, ids, out),
        "rt_scene_create_surface": lambda: L.rt_scene_create_surface(first, C.byref(g.surface), device, out),
        "rt_scene_create_textured": lambda: L.rt_scene_create_textured(first, C.byref(g.surface), None, device, out),
        "rt_scene_create_instanced": lambda: L.rt_scene_create_instanced(first, C.byref(g.inst), device, out),
        "rt_scene_create_moving": lambda: L.rt_scene_create_moving(first, C.byref(g.inst), C.byref(g.motion), device, out),
        "rt_scene_load_xml": lambda: L.rt_scene_load_xml(first, device, out),
        "rt_scene_load_xml_multi": lambda: L.rt_scene_load_xml_multi(first, 1, ids, out),
        "rt_scene_load_xml_surface": lambda: L.rt_scene_load_xml_surface(first, device, out),
        "rt_scene_load_xml_textured": lambda: L.rt_scene_load_xml_textured(first, None, 0, device, out),
        "rt_scene_load_xml_instanced": lambda: L.rt_scene_load_xml_instanced(first, device, out),
        "rt_scene_load_xml_moving": lambda: L.rt_scene_load_xml_moving(first, device, out),
    }[entry]()


@pytest.fixture(scope="module")
def given(scene_dir):
    return Given(scene_dir)


@pytest.mark.parametrize("entry", CREATE + LOAD)
def test_bad_argument(given, entry):
    """A NULL description or path, or a NULL `out`: RT_E_INVALID."""
    good = C.byref(given.desc.d) if entry in CREATE else given.xml.encode()
    h = C.c_void_p()
    assert call(entry, None, 0, C.byref(h), given) == _lib.RT_E_INVALID
    assert b"NULL argument" in _lib.lib().rt_last_error() and not h.value
    assert call(entry, good, 0, None, given) == _lib.RT_E_INVALID
    assert b"NULL argument" in _lib.lib().rt_last_error()


@pytest.mark.parametrize("device", [0, -1])
@pytest.mark.parametrize("entry", CREATE)
def test_bad_description(given, entry, device):
    """A face that names vertex num_vertices: RT_E_INVALID with the builder's message and a NULL
    `*out`, whatever the device."""
    faces = given.desc.arrays["mesh_faces"]
    keep = int(faces[0])
    faces[0] = given.desc.d.num_vertices
    try:
        h = C.c_void_p(1)
        assert call(entry, C.byref(given.desc.d), device, C.byref(h), given) == _lib.RT_E_INVALID
        assert _lib.lib().rt_last_error() == b"vertex index out of range"
        assert not h.value
    finally:
        faces[0] = keep


@pytest.mark.parametrize("entry", LOAD)
def test_bad_file(given, entry, scene_dir):
    """A missing file is RT_E_IO and a truncated one RT_E_PARSE, on a device that is not there."""
    h = C.c_void_p(1)
    missing = os.path.join(scene_dir, "no_such_scene.xml")
    assert call(entry, missing.encode(), -1, C.byref(h), given) == _lib.RT_E_IO
    assert not h.value
    cut = os.path.join(scene_dir, "entries_truncated.xml")
    text = open(given.xml).read()
    with open(cut, "w") as f:
        f.write(text[:len(text) // 2])
    h = C.c_void_p(1)
    assert call(entry, cut.encode(), -1, C.byref(h), given) == _lib.RT_E_PARSE
    assert not h.value
