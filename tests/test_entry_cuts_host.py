"""Entry cuts on the host (entry_cuts.cpp): the per-tile node references at which
the frame kernel starts its primary walks.

rt_host_check_entry_cuts_xml builds a camera's table and walks every pixel ray of every tile from
the root with the kernel's per-lane slot test restated on the host; a leafy slot a ray enters
outside its tile's cut is a violation.  Shares measured with the shipped tree (treelets of two
leaves), printed by the tests:
  cut_hf    425 tiles: 384 below the root (13 one level down, 323 two, 48 three), 73 with four
            nodes; the 41 at the root are the sign rule's (the camera looks straight down)
  cut_axis  63 tiles: 28 kept at the root by the sign rule, 35 not"""
import ctypes as C

import numpy as np
import pytest

import entry_cut_scenes as ECS
import scenes
from ceng795_amd import _lib
from oracle.cpu_ref import OracleScene

K = 2  # the shipped treelet size (kDefaultTreeletLeaves)
CUT = 4  # RT_ENTRY_CUT_NODES


def cameras(xml, name):
    n = ECS.SCENES[name][1]
    return n if n is not None else OracleScene(xml).num_cameras


def cuts(xml, cam, treelets=K):
    """(table [tiles, CUT] or None, stats) of rt_host_entry_cuts_xml."""
    st = (C.c_longlong * 24)()
    n = _lib.lib().rt_host_entry_cuts_xml(xml.encode(), treelets, cam, None, 0, st)
    assert n >= 0, _lib.lib().rt_last_error().decode()
    if n == 0:
        return None, list(st)
    out = np.full(n, -7, np.int32)
    assert _lib.lib().rt_host_entry_cuts_xml(xml.encode(), treelets, cam,
                                             out.ctypes.data_as(C.c_void_p), n, st) == n
    return out.reshape(-1, CUT), list(st)


def check(xml, cam):
    bad, first = C.c_longlong(-1), (C.c_longlong * 4)()
    n = _lib.lib().rt_host_check_entry_cuts_xml(xml.encode(), K, cam, C.byref(bad), first)
    assert n > 0, _lib.lib().rt_last_error().decode()
    return bad.value, list(first)


@pytest.mark.parametrize("name", sorted(ECS.SCENES))
def test_every_pixel_ray_stays_under_its_tiles_cut(scene_dir, name):
    xml = ECS.write(name, scene_dir)
    for cam in range(cameras(xml, name)):
        bad, first = check(xml, cam)
        assert bad == 0, (name, cam, bad, first)


@pytest.mark.parametrize("name", sorted(ECS.SCENES))
def test_tables_are_well_formed(scene_dir, name):
    """Every record names at least one node, the unused places hold -1 and follow the used ones,
    a node appears once, and the statistics add up."""
    xml = ECS.write(name, scene_dir)
    for cam in range(cameras(xml, name)):
        o = OracleScene(xml).camera(cam)
        table, st = cuts(xml, cam)
        tiles = ((o.width + 7) // 8) * ((o.height + 7) // 8)
        assert table.shape == (tiles, CUT) and st[0] == tiles
        used = table >= 0
        assert used[:, 0].all() and ((table == -1) | used).all()
        assert (used[:, :-1] | ~used[:, 1:]).all()  # no gap
        assert sum(st[1:CUT + 1]) == tiles and sum(st[8:23]) == tiles
        for n in range(1, CUT + 1):
            assert st[n] == int((used.sum(1) == n).sum())
        for rec in table[used.sum(1) > 1]:
            assert len(set(rec[rec >= 0])) == int((rec >= 0).sum())
        assert (table[used] & (1 << 30)).all()  # tagged culling-node references
        root = table[used].min()  # the culling tree's first node is its root
        assert st[8] == int((table[:, 0] == root).sum())
        assert st[6] >= tiles - st[8] and st[7] >= 2 * st[6]
        assert 0 <= st[23] <= st[8]


def test_height_field_cuts_lie_below_the_root(scene_dir):
    xml = ECS.write("cut_hf", scene_dir)
    table, st = cuts(xml, 0)
    tiles, at_root, full = st[0], st[8], st[CUT]
    print(f"cut_hf: {tiles} tiles, {tiles - at_root} below the root, {full} with {CUT} nodes, "
          f"by depth {st[8:23]}, by size {st[1:CUT + 1]}, {st[6]} visits and {st[7]} slots above")
    assert tiles == 25 * 17
    assert 4 * (tiles - at_root) >= tiles
    assert full >= 1
    # (the camera looks straight down: the tiles on its centre column and row keep the root)
    assert 0 < st[23] <= 2 * (25 + 17)


def test_axis_aligned_camera_keeps_the_zero_tiles_at_the_root(scene_dir):
    xml = ECS.write("cut_axis", scene_dir)
    table, st = cuts(xml, 0)
    tiles, to_root = st[0], st[23]
    print(f"cut_axis: {tiles} tiles, {to_root} kept at the root by the sign rule")
    assert tiles == 9 * 7
    # the centre column (pixel 32) lies in tile column 4, within a pixel of column 3's edge; the
    # centre row (pixel 24) in tile row 3, within a pixel of row 2's
    kept = np.zeros((7, 9), bool)
    kept[:, 3:5] = True
    kept[2:4, :] = True
    assert to_root == int(kept.sum())
    root = table[table >= 0].min()
    assert (table.reshape(7, 9, CUT)[kept][:, 0] == root).all()
    assert (table.reshape(7, 9, CUT)[kept][:, 1:] == -1).all()


@pytest.mark.parametrize("name", ["single_sphere", "single_triangle"])
def test_no_table_for_a_root_primitive(scene_dir, name):
    table, st = cuts(scenes.write(name, scene_dir), 0)
    assert table is None and not any(st)


def test_no_table_without_a_culling_tree(scene_dir):
    table, st = cuts(ECS.write("cut_hf", scene_dir), 0, treelets=0)
    assert table is None and not any(st)


def test_bad_arguments(scene_dir):
    L = _lib.lib()
    xml = ECS.write("cut_two", scene_dir).encode()
    bad = C.c_longlong()
    assert L.rt_host_entry_cuts_xml(None, K, 0, None, 0, None) == _lib.RT_E_INVALID
    assert L.rt_host_entry_cuts_xml(xml, K, 2, None, 0, None) == _lib.RT_E_INVALID
    assert L.rt_host_check_entry_cuts_xml(xml, K, 0, None, None) == _lib.RT_E_INVALID
    assert L.rt_host_check_entry_cuts_xml(xml, K, -1, C.byref(bad), None) == _lib.RT_E_INVALID
    assert L.rt_test_entry_cuts(2) == _lib.RT_E_INVALID
    assert L.rt_test_entry_cuts(0) == 0
