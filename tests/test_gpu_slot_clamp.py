"""The coherent slot test's zero bound as a clamp, in scaled time (visit_wide).

The frame kernel's slot test reads `tf >= max3(clamp01(n0), n1, n2)` with plane distances in
scaled time t 2^-E; E is the launch's (rt_internal.h visit_time_exp): 2^E is at least twice the
camera's distance to the farthest corner of the culling tree's root box and twice the box's
diagonal.  An entry distance above 1 is clamped to 1 — earlier — so a slot can only be entered by
more lanes, and the guard test decides exactly: no frame may change, whatever E is.

Scenes: a 32 x 32 height field (one light) and a 200-triangle soup with spheres and three lights,
64 x 64 pixels, each from a camera inside the scene's box, one on a face of it and one 100 box
diagonals away.  Frames — rendered directly and assembled from pixel records — equal the CPU oracle
bit for bit; then once more with 2^E forced to the largest power of two not above 1/8 of the root
box's diagonal (rt_test_visit_time_exp, a process-wide switch no other caller sets), where nearly
every entry distance exceeds 1 and the upper clamp binds.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402
from rq_util import bits  # noqa: E402

F = np.float32
W = H = 64
THREADS = 8
FORCED_REL = -3  # 2^E <= diagonal / 8
CAMERAS = ("inside", "on", "far")


def base_spec(name):
    if name == "hf32":
        return G.heightfield_scene(32, W, H)
    spec = G.soup_scene(47, W, H, n_mesh_tris=200, n_lights=2)
    assert len(spec.lights) == 3
    return spec


def bbox(spec):
    """The scene's box from its vertices and spheres, in fp32 as the loaders keep them."""
    v = np.array([[float(x) for x in ln.split()] for ln in spec.vertex_text.strip().split("\n")],
                 F)
    lo, hi = v.copy(), v.copy()  # (both scenes use every vertex)
    for _, c, r in spec.spheres:
        lo[c - 1] = v[c - 1] - F(r)
        hi[c - 1] = v[c - 1] + F(r)
    return lo.min(axis=0), hi.max(axis=0)


@functools.lru_cache(maxsize=None)
def placed_spec(name):
    """The base scene with the three cameras; returns (spec, lo, hi)."""
    spec = base_spec(name)
    lo, hi = bbox(spec)
    c = ((lo.astype(np.float64) + hi) / 2)
    diag = float(np.sqrt(((hi.astype(np.float64) - lo) ** 2).sum()))
    inside = tuple(float(x) for x in c)
    on = (float(hi[0]), float(c[1]), float(c[2]))  # on the +x face
    far = (float(c[0]), float(c[1] + 100 * diag), float(c[2]))
    half = 0.55 * diag
    spec.cameras = [
        G.Camera(inside, (0.3, -0.25, -1), (0, 1, 0), (-1, 1, -1, 1), 1, W, H, "inside.png"),
        G.Camera(on, (-1, -0.1, 0.05), (0, 1, 0), (-1, 1, -1, 1), 1, W, H, "on.png"),
        G.Camera(far, (0, -1, 0), (0, 0, -1), (-half, half, -half, half), 100 * diag, W, H,
                 "far.png")]
    return spec, lo, hi


def scene_xml(directory, name):
    path = os.path.join(directory, f"slot_clamp_{name}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(placed_spec(name)[0].to_xml())
    return path


@functools.lru_cache(maxsize=None)
def oracle_frame(xml, camera):
    from oracle.cpu_ref import OracleScene
    o = OracleScene(xml)
    ref, st = o.render(camera, threads=THREADS)
    rec = o.primary_records(camera)
    o.close()
    ref.setflags(write=False)
    rec.setflags(write=False)
    return ref, st, rec


def time_exp(lo, hi, cam):
    from ceng795_amd import _lib
    box = np.concatenate([lo, hi]).astype(F)
    c = np.asarray(cam, F)
    return _lib.lib().rt_host_visit_time_exp(box.ctypes.data, c.ctypes.data)


def case(directory, name, k):
    """No GPU: camera k stands where its name says, its frame has hits, and E is as documented."""
    spec, lo, hi = placed_spec(name)
    xml = scene_xml(directory, name)
    pos = np.asarray(spec.cameras[k].position, F)
    diag = float(np.sqrt(((hi.astype(np.float64) - lo) ** 2).sum()))
    if CAMERAS[k] == "inside":
        assert (pos > lo).all() and (pos < hi).all()
    elif CAMERAS[k] == "on":
        assert pos[0] == hi[0] and (pos[1:] > lo[1:]).all() and (pos[1:] < hi[1:]).all()
    else:
        assert pos[1] - hi[1] >= 99 * diag
    rec = oracle_frame(xml, k)[2]
    hit = rec[..., 7] == 1.0
    assert hit.any(), (name, k)
    far = float(np.sqrt((np.maximum(np.abs(pos - lo.astype(np.float64)),
                                    np.abs(pos - hi.astype(np.float64))) ** 2).sum()))
    e = time_exp(lo, hi, pos)
    assert 2.0 ** e >= 2 * max(far, diag) > 2.0 ** (e - 1)
    t = rec[..., 3][hit].astype(np.float64)
    assert (t * 2.0 ** -e < 1).all()  # the rule keeps every entry distance below the clamp
    forced = int(np.floor(np.log2(diag))) + FORCED_REL
    share = float((t > 2.0 ** forced).mean())
    print(f"{name}/{CAMERAS[k]}: E {e}, forced E {forced}, {int(hit.sum())} of {hit.size} pixels "
          f"hit, {share:.2f} of them beyond the forced scale's clamp")
    if CAMERAS[k] == "far":
        assert share == 1.0
    return xml


def test_cases_occur(scene_dir):
    for name in ("hf32", "soup200"):
        for k in range(len(CAMERAS)):
            case(scene_dir, name, k)


def frames(xml, k):
    """Camera k's frame rendered directly and assembled from pixel records."""
    import ceng795_amd
    from test_gpu_records import assembled
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, st = s.render_image(k)
        assert s.records_ok(k)
        rec = assembled(s, 1, root_inplace=False)[k]
    return got, st, rec


def check(xml, k, what):
    ref, st, _ = oracle_frame(xml, k)
    got, gst, rec = frames(xml, k)
    d1 = int((bits(got) != bits(ref)).any(axis=-1).sum())
    d2 = int((bits(rec) != bits(ref)).any(axis=-1).sum())
    print(f"{what}: {d1} pixels differ, {d2} through records")
    assert got.shape == ref.shape and d1 == 0 and d2 == 0, what
    assert gst.primary_rays == st.primary_rays and gst.primary_hits == st.primary_hits, what
    assert gst.shadow_rays == st.shadow_rays, what


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CAMERAS)))
@pytest.mark.parametrize("name", ["hf32", "soup200"])
def test_frames_equal_the_oracle(scene_dir, name, k):
    check(case(scene_dir, name, k), k, f"{name}/{CAMERAS[k]}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CAMERAS)))
@pytest.mark.parametrize("name", ["hf32", "soup200"])
def test_frames_with_the_clamp_binding(scene_dir, name, k):
    from ceng795_amd import _lib
    xml = case(scene_dir, name, k)
    assert _lib.lib().rt_test_visit_time_exp(1, FORCED_REL) == 0
    try:
        check(xml, k, f"{name}/{CAMERAS[k]}/forced")
    finally:
        assert _lib.lib().rt_test_visit_time_exp(0, 0) == 0
