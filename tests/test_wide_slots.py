"""The 8-wide node visit (rt_kernels.hip visit_wide) on small culling trees whose nodes have every
possible number of valid slots, and on a small height field that takes every queue-push form.

Host part (no GPU): loose-triangle scenes of 1, 2, 3, 5, 9, 11, 17, 31 and 33 triangles pass
check_accel, and their culling trees together hold wide nodes with every valid-slot count a
tree can have, 2 through 8 (rt_host_accel_slot_hist_xml).  A node with fewer than two valid
slots is itself a check_accel violation ("wide node with fewer than two slots"), so counts 0
and 1 are asserted absent rather than covered.

GPU part: those scenes at 64x64 in fast mode, bit for bit against the CPU oracle (pixels and
ray counts); the 33-triangle scene through a camera whose rays all skip the x axis (invalid
slots meet S = 0 and planes at -+inf); a 200-triangle height field at 96x96 under three lights
(lone and pair pushes in the primary and the shadow form, stack pushes); and the same pixel
rays through rt_trace_rays / rt_occluded, which inline the same visit."""
import ctypes as C
import functools
import os
import random
import sys

import numpy as np
import pytest

import rq_util
from conftest import ROOT, assert_parity

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402

# 1, 2, 3, 5, 9, 17, 33 give nodes with 2, 3, 4, 6 and 8 valid slots; 11 adds 7 and 31 adds 5
LOOSE = [1, 2, 3, 5, 9, 11, 17, 31, 33]
THREADS = min(16, os.cpu_count() or 1)
MATERIALS = [G.Material(ambient=(1, 1, 1), diffuse=(1, 1, 1), specular=(1, 1, 1), phong=1),
             G.Material(ambient=(1, 0, 0), diffuse=(1, 0.2, 0.1), specular=(1, 1, 1), phong=10)]


def front_camera(width=64, height=64, near_plane=(-1, 1, -1, 1)):
    return G.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), tuple(near_plane), 1, width, height, "w.png")


def loose_spec(n, camera=None):
    """n loose triangles scattered in the view volume of front_camera (seeded by n)."""
    rng = random.Random(795 + n)
    verts, tris = [], []
    for k in range(n):
        c = (rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-6.0, -3.0))
        for _ in range(3):
            verts.append(tuple(c[a] + rng.uniform(-0.5, 0.5) for a in range(3)))
        tris.append((1 + k % 2, (3 * k + 1, 3 * k + 2, 3 * k + 3)))
    return G.SceneSpec(cameras=[camera or front_camera()], ambient=(25, 25, 25),
                       lights=[((0, 3, 0), (800, 800, 800))], materials=MATERIALS,
                       vertex_text="\n".join("%.6f %.6f %.6f" % v for v in verts),
                       triangles=tris)


def heightfield_spec():
    """10 x 10 cells = 200 triangles, 96x96, three lights on different sides."""
    spec = G.heightfield_scene(11, 96, 96, name="w.png")
    spec.lights = [((0, 4, -5), (1000, 1000, 1000)), ((-4, 2, -3), (600, 500, 400)),
                   ((3, 1, -7), (300, 500, 700))]
    return spec


def write(directory, name, spec):
    path = os.path.join(directory, f"wide_{name}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(spec.to_xml())
    return path


def scene_xml(directory, name):
    if name == "hf200":
        return write(directory, name, heightfield_spec())
    if name == "skip_x":  # every ray's d.x is below the reference's 1e-6: the x axis is skipped
        return write(directory, name, loose_spec(33, front_camera(near_plane=(-1e-7, 1e-7, -1, 1))))
    return write(directory, name, loose_spec(int(name)))


GPU_SCENES = [str(n) for n in LOOSE] + ["skip_x", "hf200"]


# ------------------------------------------------------------------ host
def slot_histogram(xml):
    from ceng795_amd import _lib
    hist = (C.c_longlong * 9)()
    rc = _lib.lib().rt_host_accel_slot_hist_xml(xml.encode(), 2, hist)
    assert rc == 0, _lib.lib().rt_last_error().decode()
    return list(hist)


@pytest.mark.parametrize("n", LOOSE)
def test_loose_scene_culling_tree_checks(scene_dir, n):
    from ceng795_amd import _lib
    xml = scene_xml(scene_dir, str(n))
    st = (C.c_longlong * 4)()
    rc = _lib.lib().rt_host_check_accel_xml(xml.encode(), 2, st)
    assert rc == 0, _lib.lib().rt_last_error().decode()
    treelets, nodes, depth, lone = list(st)
    hist = slot_histogram(xml)
    assert sum(hist) == nodes and hist[0] == 0 and hist[1] == 0
    if n <= 2:  # the whole tree is one treelet (or the root is the primitive): no culling tree
        assert treelets == 0 and nodes == 0
    else:
        assert treelets >= 2 and nodes >= 1 and lone <= treelets


def test_loose_scenes_cover_every_valid_slot_count(scene_dir):
    total = [0] * 9
    for n in LOOSE:
        for v, k in enumerate(slot_histogram(scene_xml(scene_dir, str(n)))):
            total[v] += k
    print("wide nodes by valid slots:", total)
    assert total[0] == 0 and total[1] == 0
    assert all(total[v] >= 1 for v in range(2, 9)), total


def test_slot_histogram_rejects_null():
    from ceng795_amd import _lib
    L = _lib.lib()
    assert L.rt_host_accel_slot_hist_xml(None, 2, (C.c_longlong * 9)()) == _lib.RT_E_INVALID
    assert L.rt_host_accel_slot_hist_xml(b"x.xml", 2, None) == _lib.RT_E_INVALID


# ------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def oracle_frame(xml):
    from oracle.cpu_ref import OracleScene
    return OracleScene(xml).render(0, threads=THREADS)


@functools.lru_cache(maxsize=None)
def oracle_rays(xml):
    return rq_util.oracle_batch(xml)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_render_matches_oracle(scene_dir, name):
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    ref, st = oracle_frame(xml)
    if name == "skip_x":
        assert (np.abs(oracle_rays(xml).d[:, 0]) < 1e-6).all()
    if name == "hf200":
        assert st.shadow_rays >= 3 * 1000  # three lights reach the shadow form
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, gst = s.render_image(0)
    nbad = assert_parity(got, ref, name)
    assert nbad == 0, f"{name}: {nbad} channels within 1 ulp but not identical"
    assert gst.primary_rays == st.primary_rays
    assert gst.primary_hits == st.primary_hits
    assert gst.shadow_rays == st.shadow_rays


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_ray_queries_match_oracle(scene_dir, name):
    """The camera's pixel rays through rt_trace_rays / rt_occluded: the hit set and t bit for
    bit; and, these scenes holding triangles only (a triangle hit has t > 0), a ray is occluded
    below tmax = 1e30 exactly when the oracle's closest hit exists."""
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    b = oracle_rays(xml)
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        hits = s.trace_rays(b.o, b.d)
        occ = s.occluded(b.o, b.d, np.full(len(b), 1e30, np.float32))
    hit = b.hit
    assert np.array_equal(hits["leaf"] >= 0, hit)
    assert np.array_equal(hits["t"][hit].view(np.uint32), b.t[hit].view(np.uint32))
    assert np.isposinf(hits["t"][~hit]).all()
    assert (b.t[hit] > 0).all()
    assert np.array_equal(occ == 1, hit)
