"""Host side of the octant copies of the culling nodes (accel_build.cpp add_octant_copies,
DESIGN.md §3, §4.2): every culling-tree build stores the 8-wide nodes once per direction-sign
octant, and check_accel verifies each copy against copy 0 — the same records but for the slot
words' halves swapped on the octant's axes and inner_base shifted into the copy.

The node array must stay below 2^26 slots (32-bit byte offsets in the kernels): a scene whose
reference slots + 8 x culling slots reach that is refused.  Such a scene has about 22 M
triangles, too many to build in a test, so the size rule is put to the test through
rt_host_accel_slots_check — the function scene creation calls — at the limit and just past it."""
import ctypes as C

import pytest

import scenes
from ceng795_amd import _lib

LIMIT = 1 << 26  # rt_internal.h kMaxNodeSlots
COPIES = 8


@pytest.mark.parametrize("name", ["c1", "hf_small", "hf_side", "soup1", "soup3", "c2", "graze_plane"])
def test_octant_copies_pass_check_accel(scene_dir, name):
    xml = scenes.write(name, scene_dir)
    st = (C.c_longlong * 4)()
    rc = _lib.lib().rt_host_check_accel_xml(xml.encode(), 2, st)
    assert rc == 0, _lib.lib().rt_last_error().decode()
    assert st[1] > 0  # a culling tree was built (and with it its copies)


def test_node_slot_limit():
    L = _lib.lib()
    ref = 1 << 20
    wide = (LIMIT - ref) // COPIES  # ref + 8 * wide == 2^26: one slot too many
    assert ref + COPIES * wide == LIMIT
    assert L.rt_host_accel_slots_check(ref, wide - 2) == 0  # (a wide node is two slots)
    assert L.rt_host_accel_slots_check(0, 0) == 0
    rc = L.rt_host_accel_slots_check(ref, wide)
    assert rc == -5  # RT_E_UNSUPPORTED
    msg = L.rt_last_error().decode()
    assert "scene too large for the culling tree" in msg and str(LIMIT - 1) in msg, msg
    assert f"{COPIES} x {wide}" in msg
    assert L.rt_host_accel_slots_check(-1, 0) < 0
