"""The leaf batch's deferred guard (rt_kernels.hip batch_flush_deferred / guard_batch, DESIGN.md
§4.5), which the primary walk of the culling tree takes: stage 1 runs the triangle test of every
queued (lane, leaf) pair and appends the survivors (hit, 0 < t < inf) to a 64-entry per-wave
buffer; stage 2 takes the guard decision of 64 survivors at a time and commits the accepted ones.
A full buffer runs its guard batch at once — an iteration's survivors that did not fit are
appended after it — survivors wait across mid-walk flushes, and only a traversal's last guard
batch is partial.  The shadow walk keeps the guard in front of the triangle test (deferring it
there measured no gain) and only counts its survivors.

Frames (tools/gen_scene.py), all 32x32 pixels = 16 packets, fast mode, pixels and ray counts bit
for bit against the CPU oracle; the same pixel rays also through rt_trace_rays / rt_occluded /
rt_shade_rays, whose batches fetch the owner's origin (the frame's primary batch does not):
  * stack: 32 large triangles in 16 layers behind each other, each triangle alone covering the
    whole view, a light in front.  (Two triangles of a quad share only its diagonal, so of a stack
    of quads every ray would hit half the triangles; with whole-view triangles every queued primary
    test survives, which is the case the buffer's capacity rule is for.)  Each packet queues
    64 x 32 = 2,048 primary tests — more than one wide node's leaves, so the walk flushes mid-way
    — and every stage-1 iteration fills the buffer exactly.  A layer's two triangles are
    coincident copies (the same three vertices) with different materials, so t ties bit for bit
    in every layer and the front layer's tie decides the pixel: the lower DFS leaf must win.  The
    front layer is axis-aligned, so its guard box is flat and its guard decision falls in the
    band (guard_exact); the others are tilted.
  * hf48 from above and from the side, three lights, and hf48_below (one light under a floor:
    every shadow ray occluded; one above) — the frames of test_leaf_carry_gpu.py: one test in
    four to nine survives, survivors wait across mid-walk flushes and iterations split at the
    buffer's end.
  * the 33 loose triangles of test_wide_slots: no packet reaches the flush threshold, so a
    traversal runs only its final stage-1 batches and one final stage-2 batch at most.
  * hf48 as a mirror with MaxRecursionDepth 2: the ray trees of recursive_kernel.

Counts, from the RT_DIAG library in one child process (tools/leaf_defer.py), printed under -s:
  * survivors <= leaf tests; on the stack frame primary survivors == primary leaf tests and
    every 64-test iteration is followed by its guard batch (guard iterations == iterations);
  * primary: survivors / 64 <= guard iterations <= survivors / 64 + traversals, that is every
    survivor gets its decision and a traversal runs at most one partial guard batch (a traversal
    of S survivors runs ceil(S / 64) of them); shadow: no guard iterations;
  * iterations <= leaf tests / 64 + traversals still holds (test_leaf_carry_gpu.py's bound);
  * over the hf48 frames some guard batch splits an iteration's survivors (the capacity rule's
    late append).  On the stack frame none can: every iteration brings exactly 64 survivors to an
    empty buffer.
  * guard_rejected (survivors the guard turned down: tests the culling tree queued that the
    reference never makes) is printed and bounded by the survivors only."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rq_util
from conftest import ROOT, assert_parity
from test_leaf_carry_gpu import H, THREADS, W, hf48_spec
from test_leaf_carry_gpu import scene_xml as carry_xml

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402

LAYERS = 16


def stack_spec():
    verts, tris = [], []
    for k in range(LAYERS):
        z = -3.0 - 0.5 * k
        # the frustum is |x|, |y| <= |z| <= 10.5 here; each triangle contains that square
        tilt = (0.0, 0.0, 0.0) if k == 0 else (0.05 * k, -0.03 * k, 0.02 * k)
        verts += [(-40.0, -20.0, z + tilt[0]), (40.0, -20.0, z + tilt[1]), (0.0, 60.0, z + tilt[2])]
        tris += [(1, (3 * k + 1, 3 * k + 2, 3 * k + 3)), (2, (3 * k + 1, 3 * k + 2, 3 * k + 3))]
    cam = G.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), (-1, 1, -1, 1), 1, W, H, "stack.png")
    return G.SceneSpec(
        cameras=[cam], ambient=(25, 25, 25), lights=[((0.5, 0.7, -1.0), (300, 300, 300))],
        materials=[G.Material((1, 1, 1), (0.9, 0.3, 0.2), (0.3, 0.3, 0.3), phong=3),
                   G.Material((1, 1, 1), (0.2, 0.4, 0.9), (0.5, 0.5, 0.5), phong=7)],
        vertex_text="\n".join("%.6f %.6f %.6f" % v for v in verts), triangles=tris)


def mirror_spec():
    spec = hf48_spec()
    spec.cameras = spec.cameras[1:]  # from the side: mirror rays meet the field again
    spec.materials = [G.Material((1, 1, 1), (0.7, 0.7, 0.7), (0.4, 0.4, 0.4),
                                 mirror=(0.5, 0.5, 0.5), phong=2)]
    spec.max_depth = 2
    return spec


def scene_xml(directory, name):
    if name in ("hf48", "hf48_below", "loose33"):
        return carry_xml(directory, name)
    path = os.path.join(directory, f"defer_{name}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write({"stack": stack_spec, "hf48_mirror": mirror_spec}[name]().to_xml())
    return path


FRAMES = [("stack", 0), ("hf48", 0), ("hf48", 1), ("hf48_below", 0), ("loose33", 0),
          ("hf48_mirror", 0)]
DIAG_FRAMES = FRAMES[:5]
SPARSE = (1, 2, 3)  # the hf48 frames among DIAG_FRAMES


@functools.lru_cache(maxsize=None)
def oracle_frame(xml, camera):
    from oracle.cpu_ref import OracleScene
    return OracleScene(xml).render(camera, threads=THREADS)


@pytest.mark.gpu
@pytest.mark.parametrize("name,camera", FRAMES)
def test_render_matches_oracle(scene_dir, name, camera):
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    ref, st = oracle_frame(xml, camera)
    if name != "loose33":
        assert st.primary_hits == W * H  # the geometry fills the frame: every packet walks
    if name == "hf48_mirror":
        assert st.as_dict()["secondary_rays"] > 0
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, gst = s.render_image(camera)
    nbad = assert_parity(got, ref, f"{name}:{camera}")
    if name != "hf48_mirror":  # (a ray tree's colour sums may differ by the last bit)
        assert nbad == 0, f"{name}: {nbad} channels within 1 ulp but not identical"
    assert gst.primary_rays == st.primary_rays
    assert gst.primary_hits == st.primary_hits
    assert gst.shadow_rays == st.shadow_rays
    assert gst.secondary_rays == st.as_dict()["secondary_rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stack", "hf48", "hf48_below", "loose33"])
def test_ray_queries_match_oracle(scene_dir, name):
    """The frames' pixel rays through rt_trace_rays / rt_occluded / rt_shade_rays: the batches
    there fetch the owner's origin per entry (no CAMERA shortcut)."""
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    cams = [0, 1] if name == "hf48" else [0]
    b = rq_util.oracle_batch(xml, cameras=cams)
    frames = np.concatenate([oracle_frame(xml, c)[0].reshape(-1, 3) for c in cams])
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        hits = s.trace_rays(b.o, b.d)
        occ = s.occluded(b.o, b.d, np.full(len(b), 1e30, np.float32))
        rad = s.shade_rays(b.o, b.d)
    assert np.array_equal(hits["leaf"] >= 0, b.hit)
    assert np.array_equal(hits["t"][b.hit].view(np.uint32), b.t[b.hit].view(np.uint32))
    assert np.array_equal(occ == 1, b.hit)
    assert assert_parity(rad["rgb"][b.hit], frames[b.hit], f"{name}: shade_rays") == 0
    if name == "stack":
        assert b.hit.all()
        # the front layer's tie: both copies at the same t, the lower DFS leaf wins everywhere
        assert len(np.unique(hits["leaf"])) == 1 and len(np.unique(hits["material"])) == 1


@functools.lru_cache(maxsize=None)
def diag_counts(directory):
    args = [f"{scene_xml(directory, n)}:{c}" for n, c in DIAG_FRAMES]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "leaf_defer.py"), *args],
                       env=dict(os.environ, CENG795_LIB="diag"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(DIAG_FRAMES)))
def test_guard_batches_are_full_but_the_last(scene_dir, k):
    d = diag_counts(scene_dir)[k]
    print(json.dumps(d))
    assert d["waves"] == d["packets"] == 16  # a cold frame: one wave per packet
    assert d["guard_tests"] == d["primary"]["leaf_tests"] + d["shadow"]["leaf_tests"]
    for kind in ("primary", "shadow"):
        c = d[kind]
        assert c["survivors"] <= c["leaf_tests"]
        assert c["guard_rejected"] <= c["survivors"]
        assert c["flush_iters"] <= c["leaf_tests"] / 64 + c["traversals"]
        assert c["split_drains"] <= c["guard_iters"]
    p = d["primary"]
    assert p["survivors"] / 64 <= p["guard_iters"] <= p["survivors"] / 64 + p["traversals"]
    assert d["shadow"]["guard_iters"] == 0  # the shadow walk takes the guard first


@pytest.mark.gpu
def test_every_test_survives_on_the_stack(scene_dir):
    d = diag_counts(scene_dir)[0]
    p = d["primary"]
    print("stack", json.dumps(p))
    assert p["leaf_tests"] == 16 * 64 * 2 * LAYERS  # every lane tests every triangle
    assert p["survivors"] == p["leaf_tests"]
    assert p["guard_rejected"] == 0
    # 2,048 tests per packet run as 32 full iterations, each filling the 64-entry buffer exactly:
    # its guard batch follows at once, none is partial and none splits an iteration
    assert p["flush_iters"] == p["guard_iters"] == p["leaf_tests"] // 64
    assert p["flushes"] > p["traversals"]  # mid-walk flushes, not one final batch
    assert p["split_drains"] == 0


@pytest.mark.gpu
def test_sparse_survivors_wait_and_split(scene_dir):
    frames = [diag_counts(scene_dir)[k] for k in SPARSE]
    for d in frames:
        print(d["scene"], d["camera"], json.dumps({k: d[k] for k in ("primary", "shadow")}))
        p = d["primary"]
        assert 0 < p["survivors"] < p["leaf_tests"] / 2
    # an iteration's survivors on both sides of a full buffer: the capacity rule's late append
    assert sum(d["primary"]["split_drains"] for d in frames) > 0
    below = frames[-1]["shadow"]
    assert below["survivors"] > 0  # the floor occludes


@pytest.mark.gpu
def test_final_batches_only_on_loose_triangles(scene_dir):
    d = diag_counts(scene_dir)[4]
    print("loose33", json.dumps({k: d[k] for k in ("primary", "shadow")}))
    for kind in ("primary", "shadow"):
        c = d[kind]
        assert c["flushes"] <= c["traversals"] and c["flush_iters"] <= c["traversals"]
        assert c["guard_iters"] <= c["traversals"]
        assert c["split_drains"] == 0
    assert d["primary"]["survivors"] > 0
