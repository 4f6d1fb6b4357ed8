"""Kind-sorted wide nodes: a culling node's inner slots lie at 0, 1, ...,
its leafy slots at 7, 6, ..., the invalid ones between them, and visit_wide runs up the one kind
and down the other without asking a slot's kind.

Host part (no GPU): the loose-triangle scenes and the 200-triangle height field of
test_wide_slots.py, `c1`, `soup1` and one further small height field pass check_accel (which
applies the slot-order rule to every node); together their (inner count, leafy count) histograms
(rt_host_accel_kind_hist_xml) hold every valid count 2 .. 8, a node without an inner slot, a node
without a leafy slot and nodes with both; a hand-built node record for each broken rule is refused
by the check (rt_host_check_wide_node).

GPU part, bit for bit against the CPU oracle: those scenes through the frame kernel (pixels and
ray counts), the camera whose rays all skip an axis, the same pixel rays through rt_trace_rays /
rt_occluded (the per-lane plane order in octant copy 0), an instanced scene (the two-level walk)
and a recursive one."""
import ctypes as C
import struct

import numpy as np
import pytest

import scenes
import test_wide_slots as ws
from conftest import assert_parity

G = ws.G
# the smallest height field (vertices per side) that fills the cells the other scenes leave
# empty: inner runs of 5, 6 and 7 slots and a leafy run of one slot (450 triangles; the scan in
# test_extra_heightfield_is_the_smallest_that_fills_the_gap)
EXTRA_HF = 16
HOST_SCENES = [str(n) for n in ws.LOOSE] + ["hf200", "hf_extra", "c1", "soup1"]
GPU_SCENES = ws.GPU_SCENES + ["hf_extra", "soup1"]


def extra_heightfield_spec():
    spec = G.heightfield_scene(EXTRA_HF, 64, 64, name="w.png")
    spec.lights = ws.heightfield_spec().lights
    return spec


def scene_xml(directory, name):
    if name == "hf_extra":
        return ws.write(directory, name, extra_heightfield_spec())
    if name in scenes.CATALOGUE:
        return scenes.write(name, directory)
    return ws.scene_xml(directory, name)


# ------------------------------------------------------------------ host
def kind_histogram(xml):
    """hist[i][l] = wide nodes with i inner and l leafy slots (of a tree that passed the check)."""
    from ceng795_amd import _lib
    hist = (C.c_longlong * 81)()
    rc = _lib.lib().rt_host_accel_kind_hist_xml(xml.encode(), 2, hist)
    assert rc == 0, _lib.lib().rt_last_error().decode()
    return np.array(list(hist), np.int64).reshape(9, 9)


@pytest.mark.parametrize("name", HOST_SCENES)
def test_culling_tree_checks_and_histograms_agree(scene_dir, name):
    xml = scene_xml(scene_dir, name)
    hist = kind_histogram(xml)
    by_valid = [int(sum(hist[i][v - i] for i in range(v + 1))) for v in range(9)]
    assert by_valid == ws.slot_histogram(xml)
    assert all(hist[i][l] == 0 for i in range(9) for l in range(9) if i + l > 8 or i + l < 2)


def test_scenes_cover_the_count_combinations(scene_dir):
    total = np.zeros((9, 9), np.int64)
    for name in HOST_SCENES:
        total += kind_histogram(scene_xml(scene_dir, name))
    print("wide nodes by (inner, leafy) slots, rows = inner count 0..8:")
    print(total)
    by_valid = [int(sum(total[i][v - i] for i in range(v + 1))) for v in range(9)]
    assert by_valid[0] == 0 and by_valid[1] == 0
    assert all(by_valid[v] >= 1 for v in range(2, 9)), by_valid
    assert total[0, :].sum() >= 1, "no node without an inner slot"
    assert total[:, 0].sum() >= 1, "no node without a leafy slot"
    assert total[1:, 1:].sum() >= 1, "no node with both kinds"
    both = [(i, l) for i in range(1, 8) for l in range(1, 8) if i + l <= 8]
    assert sum(total[i][l] for i, l in both if i + l < 8) >= 1, \
        "no node with both kinds and an invalid slot between the runs"
    assert sum(total[i][l] for i, l in both if i + l == 8) >= 1, "no full node with both kinds"


def missing_runs(hist):
    """(inner run lengths, leafy run lengths) of 0 .. 8 slots that no node of `hist` has."""
    return ([i for i in range(9) if hist[i, :].sum() == 0],
            [l for l in range(9) if hist[:, l].sum() == 0])


def test_extra_heightfield_is_the_smallest_that_fills_the_gap(scene_dir):
    """Each run of the visit has nine lengths, 0 .. 8 slots.  The scenes of test_wide_slots.py,
    c1 and soup1 lack inner runs of 5, 6 and 7 slots and the leafy run of one slot; the further
    height field has them all, and no smaller height field has."""
    others = np.zeros((9, 9), np.int64)
    for name in HOST_SCENES:
        if name != "hf_extra":
            others += kind_histogram(scene_xml(scene_dir, name))
    assert missing_runs(others) == ([5, 6, 7], [1])
    for n in range(3, EXTRA_HF):
        xml = ws.write(scene_dir, f"hf_scan{n}", G.heightfield_scene(n, 64, 64, name="w.png"))
        assert missing_runs(others + kind_histogram(xml)) != ([], []), n
    extra = kind_histogram(scene_xml(scene_dir, "hf_extra"))
    print("the further height field, rows = inner count 0..8:")
    print(extra)
    assert missing_runs(others + extra) == ([], [])


NAN_WORD = 0x7e007e00
BOX_WORD = 0x3c000000  # lo = 0, hi = 1


def node_record(inner, leafy, pair=0, counts=None, valid=None, nan=None):
    """A DevNode8 record (rt_internal.h) with the given slot bit sets."""
    valid = inner | leafy if valid is None else valid
    counts = bin(inner).count("1") | bin(leafy).count("1") << 4 if counts is None else counts
    kinds = valid | leafy << 8 | pair << 16 | counts << 24
    nan = ~valid & 0xff if nan is None else nan
    words = []
    for c in range(8):
        words += [NAN_WORD if nan >> c & 1 else BOX_WORD] * 3
    return struct.pack("<3fIiiII24I", 0.0, 0.0, 0.0, 0, 100, 0, kinds, 0, *words)


def check_node(rec):
    from ceng795_amd import _lib
    L = _lib.lib()
    buf = C.create_string_buffer(rec, len(rec))
    rc = L.rt_host_check_wide_node(buf, len(rec))
    return rc, (L.rt_last_error().decode() if rc else "")


@pytest.mark.parametrize("inner,leafy,pair", [
    (0b00000111, 0b11000000, 0b10000000), (0, 0b11000000, 0), (0b11, 0, 0),
    (0b00001111, 0b11110000, 0b01010000), (0b11111111, 0, 0), (0, 0b11111111, 0b11111111)])
def test_sorted_nodes_pass(inner, leafy, pair):
    assert check_node(node_record(inner, leafy, pair)) == (0, "")


@pytest.mark.parametrize("rec,why", [
    (node_record(0b00010011, 0b11000000), "inner slots not contiguous"),       # valid between the runs
    (node_record(0b00000011, 0b11010000), "leafy slots not contiguous"),       # valid between the runs
    (node_record(0b00000101, 0b11000010), "leafy slot below an inner one"),
    (node_record(0b00000110, 0b11000001), "leafy slot below an inner one"),
    (node_record(0b00000011, 0b11000000, counts=3 | 2 << 4), "slot counts"),
    (node_record(0b00000011, 0b11000000, counts=2 | 3 << 4), "slot counts"),
    (node_record(0b00000011, 0b11000000, counts=0), "slot counts"),
    (node_record(0b00000011, 0b11000000, pair=0b00000001), "pair flag"),
    (node_record(0b00000011, 0b11000000, valid=0b01000011), "leafy flag on an invalid slot"),
    (node_record(0b00000011, 0b11000000, nan=0b00011100), "NaN planes"),
])
def test_broken_nodes_are_refused(rec, why):
    from ceng795_amd import _lib
    rc, msg = check_node(rec)
    assert rc == _lib.RT_E_INVALID and why in msg, (rc, msg)


def test_check_entries_reject_bad_arguments():
    from ceng795_amd import _lib
    L = _lib.lib()
    rec = node_record(0b11, 0)
    assert L.rt_host_check_wide_node(None, 128) == _lib.RT_E_INVALID
    assert L.rt_host_check_wide_node(C.create_string_buffer(rec, 128), 64) == _lib.RT_E_INVALID
    assert L.rt_host_accel_kind_hist_xml(None, 2, (C.c_longlong * 81)()) == _lib.RT_E_INVALID
    assert L.rt_host_accel_kind_hist_xml(b"x.xml", 2, None) == _lib.RT_E_INVALID


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_frames_match_oracle(scene_dir, name):
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    ref, st = ws.oracle_frame(xml)
    if name in ("hf200", "hf_extra"):
        assert st.shadow_rays >= 3 * 1000  # three lights reach the shadow form
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, gst = s.render_image(0)
    nbad = assert_parity(got, ref, name)
    assert nbad == 0, f"{name}: {nbad} channels within 1 ulp but not identical"
    assert gst.primary_rays == st.primary_rays
    assert gst.primary_hits == st.primary_hits
    assert gst.shadow_rays == st.shadow_rays


@pytest.mark.gpu
@pytest.mark.parametrize("name", ws.GPU_SCENES + ["hf_extra"])
def test_pixel_rays_match_oracle(scene_dir, name):
    """rt_trace_rays / rt_occluded on the camera's pixel rays (triangle scenes: occluded below
    tmax = 1e30 exactly when the oracle's closest hit exists)."""
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    b = ws.oracle_rays(xml)
    if name == "skip_x":
        assert (np.abs(b.d[:, 0]) < 1e-6).all()
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        hits = s.trace_rays(b.o, b.d)
        occ = s.occluded(b.o, b.d, np.full(len(b), 1e30, np.float32))
    hit = b.hit
    assert np.array_equal(hits["leaf"] >= 0, hit)
    assert np.array_equal(hits["t"][hit].view(np.uint32), b.t[hit].view(np.uint32))
    assert np.isposinf(hits["t"][~hit]).all()
    assert np.array_equal(occ == 1, hit)


@pytest.mark.gpu
def test_recursive_scene_matches_oracle(scene_dir):
    import ceng795_amd
    from oracle.cpu_ref import OracleScene
    xml = scenes.write("soup_depth6", scene_dir)  # 48x40, mirrors and glass to depth 6
    ref, st = OracleScene(xml).render(0, threads=ws.THREADS)
    assert st.secondary_rays > 0
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, gst = s.render_image(0)
    assert assert_parity(got, ref, "soup_depth6") == 0
    assert (gst.primary_rays, gst.shadow_rays, gst.secondary_rays) == \
        (st.primary_rays, st.shadow_rays, st.secondary_rays)


@pytest.mark.gpu
def test_instanced_scene_matches_composite(scene_dir):
    """Scene "three" of the instance tests: closest hits and occlusion through the two-level
    walk, whose base-mesh trees are kind-sorted too."""
    import ceng795_amd
    import instance_util as iu
    spec = iu.written("three", scene_dir)
    comp = iu.Composite(spec)
    try:
        mesh, mat, xf = spec.arrays()
        o, d = iu.camera_rays(17, 9)
        o2, d2 = iu.random_rays(200, 17)
        o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
        ref = comp.intersect(o, d)
        big = np.full(len(o), 1e30, np.float32)
        with ceng795_amd.Scene.create(comp.desc.d, instance_mesh=mesh, instance_material=mat,
                                      instance_transform=xf, device=0) as s:
            s.set_traversal("fast")
            iu.assert_hits(s.trace_rays(o, d), ref, "three")
            assert np.array_equal(s.occluded(o, d, big), comp.occluded(o, d, big))
    finally:
        comp.close()
