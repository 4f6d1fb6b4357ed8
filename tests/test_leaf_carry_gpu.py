"""The leaf queue's carried remainder (rt_kernels.hip leaf_flush_full): a mid-walk
flush runs whole 64-test batches only and moves the left-over entries to the front of the queue;
only the last flush of a traversal runs a partial batch.

Scenes (tools/gen_scene.py), all at 32x32 pixels = 16 packets:
  * hf48: a 48x48-cell height field (4,608 triangles) under three lights on different sides,
    camera 0 from above, camera 1 from the side at 12-34 degrees to the surface.  Each 8x8 packet
    queues several hundred tests per traversal, so the primary and the shadow walks flush
    mid-walk;
  * hf48_below: the same field over a two-triangle floor, with one light below the floor (every
    shadow ray is occluded by the floor: lanes leave the walk while their tests sit in the
    carried remainder) and one above;
  * 33 loose triangles (test_wide_slots): no packet reaches the threshold, only the final
    flush runs.

Parity: pixels and ray counts bit for bit against the CPU oracle, fast mode and (hf48) the
reference-mode walk; the same pixel rays through rt_trace_rays / rt_occluded.

Counts, from the RT_DIAG library in one child process (tools/leaf_carry.py), on the three
height-field frames: more than one flush per traversal, and
    iterations <= guard_tests / 64 + traversals        (traversals = packets x (1 + lights))
which holds exactly when every traversal runs at most one partial batch: a traversal of T tests
runs ceil(T / 64) <= T / 64 + 1 iterations.  (Flushing every remainder, as the kernel did
before, runs 3-4 partial batches per traversal and misses the bound.)  Mid-walk flushes by
carried remainder: 0, 1-16 and 48-63 must all occur over the three frames; the counts of each
frame are printed.  A flush comes as soon as a visit takes the queue to the threshold of 128, so
its length is mostly just above 128 and the remainder small: every frame supplies the classes 0
(9-34 mid-walk flushes per frame) and 1-16 (69-148); a remainder of 48-63 needs one visit to push
about 50 tests past the threshold, which only the side camera's packets do (hf48 camera 1: 11
flushes; none from above)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rq_util
from conftest import ROOT, assert_parity
from test_wide_slots import loose_spec

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
W = H = 32
LIGHTS = [((0, 4, -5), (1000, 1000, 1000)), ((-4, 2, -3), (600, 500, 400)),
          ((3, 1, -7), (300, 500, 700))]


def hf48_spec(below=False):
    # from above: the near plane a little inside the field's edges, so every primary ray hits it
    spec = G.heightfield_scene(49, W, H, view="top", near_plane=(-0.93, 0.91, -0.92, 0.94),
                               name="top.png")
    # from the side: 2 above the field, rays 12 to 34 degrees below the horizon, all on the field
    spec.cameras.append(G.Camera((0, 0.5, 1.0), (0, -0.35, -1), (0, 1, 0),
                                 (-0.3, 0.3, -0.25, 0.1), 1, W, H, "side.png"))
    spec.lights = list(LIGHTS)
    if below:  # a floor under the field (y in [-1.65, -1.33]) and a light under the floor
        n = 49 * 49
        spec.vertex_text += "\n" + "\n".join("%.6f %.6f %.6f" % v for v in [
            (-6.0, -2.5, -11.0), (6.0, -2.5, -11.0), (6.0, -2.5, 1.0), (-6.0, -2.5, 1.0)])
        spec.triangles = [(1, (n + 1, n + 3, n + 2)), (1, (n + 1, n + 4, n + 3))]
        spec.lights = [((0.5, -4.0, -5.5), (1000, 1000, 1000)), LIGHTS[0]]
    return spec


def scene_xml(directory, name):
    path = os.path.join(directory, f"carry_{name}.xml")
    if not os.path.exists(path):
        spec = {"hf48": hf48_spec, "hf48_below": lambda: hf48_spec(True),
                "loose33": lambda: loose_spec(33, G.Camera(
                    (0, 0, 0), (0, 0, -1), (0, 1, 0), (-1, 1, -1, 1), 1, W, H, "l.png"))}[name]()
        with open(path, "w") as f:
            f.write(spec.to_xml())
    return path


# (scene, camera, traversal)
PARITY = [("hf48", 0, "fast"), ("hf48", 1, "fast"), ("hf48_below", 0, "fast"),
          ("loose33", 0, "fast"), ("hf48", 0, "reference")]
DIAG_FRAMES = [("hf48", 0), ("hf48", 1), ("hf48_below", 0)]


@functools.lru_cache(maxsize=None)
def oracle_frame(xml, camera):
    from oracle.cpu_ref import OracleScene
    return OracleScene(xml).render(camera, threads=THREADS)


@pytest.mark.gpu
@pytest.mark.parametrize("name,camera,traversal", PARITY)
def test_render_matches_oracle(scene_dir, name, camera, traversal):
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    ref, st = oracle_frame(xml, camera)
    if name != "loose33":
        assert st.primary_hits == W * H  # the field fills the frame: every packet walks
    with ceng795_amd.Scene(xml, traversal=traversal) as s:
        got, gst = s.render_image(camera)
    nbad = assert_parity(got, ref, f"{name}:{camera}:{traversal}")
    assert nbad == 0, f"{name}: {nbad} channels within 1 ulp but not identical"
    assert gst.primary_rays == st.primary_rays
    assert gst.primary_hits == st.primary_hits
    assert gst.shadow_rays == st.shadow_rays


@pytest.mark.gpu
def test_below_light_is_occluded_everywhere(scene_dir):
    """hf48_below's first light reaches no pixel: with it alone the frame is the ambient term."""
    xml = scene_xml(scene_dir, "hf48_below")
    ref, _ = oracle_frame(xml, 0)
    spec = hf48_spec(True)
    spec.lights = spec.lights[1:]
    path = os.path.join(scene_dir, "carry_hf48_floor_only.xml")
    with open(path, "w") as f:
        f.write(spec.to_xml())
    import ceng795_amd
    with ceng795_amd.Scene(path) as s:
        got, _ = s.render_image(0)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.gpu
def test_ray_queries_match_frame_hits(scene_dir):
    """hf48's camera-0 pixel rays through rt_trace_rays / rt_occluded (the same closest_hit /
    occluded, with the owner's origin fetched per entry): the oracle's hits, t bit for bit."""
    import ceng795_amd
    xml = scene_xml(scene_dir, "hf48")
    b = rq_util.oracle_batch(xml, cameras=[0, 1])
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        hits = s.trace_rays(b.o, b.d)
        occ = s.occluded(b.o, b.d, np.full(len(b), 1e30, np.float32))
    hit = b.hit
    assert hit.all()
    assert np.array_equal(hits["leaf"] >= 0, hit)
    assert np.array_equal(hits["t"].view(np.uint32), b.t.view(np.uint32))
    assert np.array_equal(occ == 1, hit)


@functools.lru_cache(maxsize=None)
def diag_counts(directory):
    args = [f"{scene_xml(directory, n)}:{c}" for n, c in DIAG_FRAMES]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "leaf_carry.py"), *args],
                       env=dict(os.environ, CENG795_LIB="diag"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(DIAG_FRAMES)))
def test_at_most_one_partial_batch_per_traversal(scene_dir, k):
    d = diag_counts(scene_dir)[k]
    print(json.dumps(d))
    assert d["waves"] == d["packets"] == 16  # a cold frame: one wave per packet
    flushes, iters = sum(d["flushes"]), sum(d["flush_iters"])
    assert flushes > d["traversals"], "flushes per traversal must exceed 1"
    assert min(d["flushes"]) > 0  # the primary and the shadow walk both flush
    assert iters <= d["guard_tests"] / 64 + d["traversals"]


@pytest.mark.gpu
def test_every_remainder_class_occurs(scene_dir):
    total = {"zero": 0, "low_1_16": 0, "high_48_63": 0}
    for d in diag_counts(scene_dir):
        print(d["scene"], d["camera"], d["carry"])
        for key in total:
            total[key] += d["carry"][key]
    assert all(v > 0 for v in total.values()), total
