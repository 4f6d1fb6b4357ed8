"""The octant copies of the culling nodes and the frame kernel's walk over them (accel_build.cpp
add_octant_copies, rt_kernels.hip octant_walks).

A packet's active lanes are walked once per direction-sign octant present among them, each walk
in that octant's copy of the culling nodes, whose slot words hold the entry plane in the low
half; the per-lane results meet in the wave's key array.  A camera's (and a point light's) rays
change sign along a line through the image, so whether a packet is mixed depends on where those
lines fall in the 8x8 tiles.

Frames, all against the CPU oracle bit for bit (pixels and ray counts):
  * hf33: the height field of 32x32 cells seen from straight above (gaze -y, up -z; the light
    above the camera axis), so d_x and d_z flip at the image centre:
      - 32x32: the centre lies on a tile corner — every packet, primary and shadow, is coherent;
      - 24x24: the centre lies inside the middle tile — that packet holds 4 primary octants, the
        four tiles beside it 2;
      - 9x9: ragged tiles, and the centre pixel's ray runs along the gaze with an exactly zero
        component: two skipped axes in a packet of 4 octants (the any_skip walk);
      - 56x56 with a wider near plane: the field covers the middle of the frame and the sky
        packets cost next to nothing, so warm frames split the heavy tiles over quadrant waves.
  * hf33_low: the 32x32 frame with a second light just above the surface, over the middle of
    tile (1, 1)'s footprint: that packet's shadow rays span 4 octants.
  * soup: meshes, loose triangles and spheres (the SPHERES kernels) under four lights, camera
    gazing along -z: 32x32 (coherent primary packets), 24x24 and 9x9 as above; its lights make
    mixed shadow packets of their own.

The octant sets are computed here from the oracle's fp32 rays (a lane's octant is the sign bits
of its direction; a shadow ray's direction has the signs of light - hit point, the hit point
being e + d * t in fp32), and the tests fail when the intended counts do not occur.  The RT_DIAG
library (tools/octant_walks.py, one child process) reports the sub-walks the kernel made: they
must equal the CPU's count exactly, which for coherent frames is one per packet.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_parity

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402

THREADS = 8
LOW_LIGHT = (-0.75, -1.2, -5.75)  # over the middle of tile (1, 1) of the 32x32 frame, y above the field


def hf_cameras():
    pose = ((0, 1.5, -5), (0, -1, 0), (0, 0, -1))
    return [G.Camera(*pose, (-1, 1, -1, 1), 1, 32, 32, "coherent.png"),
            G.Camera(*pose, (-1, 1, -1, 1), 1, 24, 24, "mixed.png"),
            G.Camera(*pose, (-1, 1, -1, 1), 1, 9, 9, "odd.png"),
            G.Camera(*pose, (-2, 2, -2, 2), 1, 56, 56, "split.png")]


def hf33_spec(low_light=False):
    spec = G.heightfield_scene(33, 32, 32)
    spec.cameras = hf_cameras() if not low_light else hf_cameras()[:1]
    if low_light:
        spec.lights = list(spec.lights) + [(LOW_LIGHT, (30, 30, 30))]
    return spec


def soup_spec():
    spec = G.soup_scene(21, 32, 32)
    pose = ((0, 0.4, 0.5), (0, 0, -1), (0, 1, 0))
    spec.cameras = [G.Camera(*pose, (-1, 1, -1, 1), 1, 32, 32, "coherent.png"),
                    G.Camera(*pose, (-1, 1, -1, 1), 1, 24, 24, "mixed.png"),
                    G.Camera(*pose, (-1, 1, -1, 1), 1, 9, 9, "odd.png")]
    return spec


SPECS = {"hf33": hf33_spec, "hf33_low": lambda: hf33_spec(True), "soup": soup_spec}
COHERENT, MIXED, ODD, SPLIT = 0, 1, 2, 3
FRAMES = [("hf33", COHERENT), ("hf33", MIXED), ("hf33", ODD), ("hf33_low", COHERENT),
          ("soup", COHERENT), ("soup", MIXED), ("soup", ODD)]


def scene_xml(directory, name):
    path = os.path.join(directory, f"octant_{name}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(SPECS[name]().to_xml())
    return path


@functools.lru_cache(maxsize=None)
def oracle_frame(xml, camera):
    from oracle.cpu_ref import OracleScene
    return OracleScene(xml).render(camera, threads=THREADS)


def octant(v):
    """Direction-sign octant of fp32 vectors (..., 3): bit a = the sign bit of component a (the
    sign of the kernels' 1 / d, a zero included)."""
    s = np.signbit(np.asarray(v, np.float32)).astype(np.int64)
    return s[..., 0] | s[..., 1] << 1 | s[..., 2] << 2


def packet_sets(octs, active):
    """Per 8x8 packet (row-major) the set of octants among its active pixels."""
    h, w = octs.shape
    return [set(octs[y:y + 8, x:x + 8][active[y:y + 8, x:x + 8]].tolist())
            for y in range(0, h, 8) for x in range(0, w, 8)]


@functools.lru_cache(maxsize=None)
def cpu_octants(name, camera):
    """(primary sets per packet, per light the shadow sets per packet, the primary directions)."""
    import tempfile
    from oracle.cpu_ref import OracleScene
    spec = SPECS[name]()
    with tempfile.TemporaryDirectory() as d:
        o = OracleScene(scene_xml(d, name))
        rec = o.primary_records(camera)
        o.close()
    d, t, hit = rec[..., 0:3], rec[..., 3], rec[..., 7] == 1.0
    e = np.array(spec.cameras[camera].position, np.float32)
    prim = packet_sets(octant(d), np.ones(hit.shape, bool))
    point = e + d * t[..., None]  # fp32: the product, then the sum (Ray::point_at)
    shadow = [packet_sets(octant(np.array(pos, np.float32) - point), hit)
              for pos, _ in spec.lights]
    return prim, shadow, d


def sizes(sets):
    return sorted(len(s) for s in sets)


def test_intended_octant_counts_occur():
    prim, shadow, _ = cpu_octants("hf33", COHERENT)
    assert sizes(prim) == [1] * 16
    assert all(len(s) == 1 for s in shadow[0])  # the light above the camera axis: the same lines
    for name in ("hf33", "soup"):
        prim, _, _ = cpu_octants(name, MIXED)
        assert sizes(prim) == [1] * 4 + [2] * 4 + [4]  # 3x3 packets around the centre pixel
        prim, _, d = cpu_octants(name, ODD)
        assert sizes(prim) == [1, 2, 2, 4]  # tiles of 8x8, 1x8, 8x1 and 1x1 pixels
        assert len(prim[0]) == 4
        c = d[4, 4]
        # along an axis: an exactly zero component, and two skipped axes (|d| < 1e-6)
        assert (c == 0).sum() >= 1 and (abs(c) < 1e-6).sum() == 2
    prim, _, _ = cpu_octants("soup", COHERENT)
    assert sizes(prim) == [1] * 16
    prim, shadow, _ = cpu_octants("hf33_low", COHERENT)
    assert sizes(prim) == [1] * 16
    assert len(shadow[1][1 * 4 + 1]) == 4  # the packet under the low light
    assert max(len(s) for s in shadow[0]) == 1
    _, shadow, _ = cpu_octants("soup", COHERENT)
    assert max(len(s) for sets in shadow for s in sets) >= 2  # its own lights mix packets too


@pytest.mark.gpu
@pytest.mark.parametrize("name,camera", FRAMES)
def test_frame_matches_oracle(scene_dir, name, camera):
    import ceng795_amd
    xml = scene_xml(scene_dir, name)
    ref, st = oracle_frame(xml, camera)
    assert st.primary_hits > 0 and st.shadow_rays > 0
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, gst = s.render_image(camera)
    assert assert_parity(got, ref, f"{name}:{camera}") == 0
    assert gst.primary_rays == st.primary_rays
    assert gst.primary_hits == st.primary_hits
    assert gst.shadow_rays == st.shadow_rays


@functools.lru_cache(maxsize=None)
def diag_counts(directory):
    args = [f"{scene_xml(directory, n)}:{c}" for n, c in FRAMES]
    args.append(f"{scene_xml(directory, 'hf33')}:{SPLIT}:3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "octant_walks.py"), *args],
                       env=dict(os.environ, CENG795_LIB="diag"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(FRAMES)))
def test_one_sub_walk_per_octant_present(scene_dir, k):
    name, camera = FRAMES[k]
    d = diag_counts(scene_dir)[k]["frames"][0]
    prim, shadow, _ = cpu_octants(name, camera)
    print(name, camera, json.dumps(d), "cpu primary", sizes(prim),
          "shadow", [sizes(s) for s in shadow])
    assert d["waves"] == d["packets"] == len(prim)  # a cold frame: one wave per packet
    assert d["primary"]["packets"] == len(prim)
    assert d["primary"]["walks"] == sum(len(s) for s in prim)
    assert d["shadow"]["packets"] == sum(len(s) > 0 for sets in shadow for s in sets)
    assert d["shadow"]["walks"] == sum(len(s) for sets in shadow for s in sets)
    if (name, camera) == ("hf33", COHERENT):  # flip lines on tile boundaries: one walk per packet
        assert d["primary"]["walks"] == d["primary"]["packets"]
        assert d["shadow"]["walks"] == d["shadow"]["packets"] > 0
    if (name, camera) == ("soup", COHERENT):
        assert d["primary"]["walks"] == d["primary"]["packets"]


@pytest.mark.gpu
def test_split_tiles_match_oracle(scene_dir):
    """Warm frames of the 56x56 view split their heavy tiles over quadrant waves (lanes 0..15 of
    four waves); the quadrants of the centre tile are mixed-octant packets themselves."""
    import torch
    import ceng795_amd
    xml = scene_xml(scene_dir, "hf33")
    ref, _ = oracle_frame(xml, SPLIT)
    frames = diag_counts(scene_dir)[len(FRAMES)]["frames"]
    print(json.dumps(frames))
    assert frames[0]["waves"] == frames[0]["packets"]
    assert max(f["waves"] for f in frames[1:]) > frames[0]["packets"]  # quadrant waves ran
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        st = torch.cuda.Stream()
        buf = torch.empty(ref.shape, dtype=torch.float32, device="cuda")
        for k in range(3):
            buf.fill_(-1.0)
            torch.cuda.synchronize()
            s.render_device(SPLIT, buf.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            assert assert_parity(buf.cpu().numpy(), ref, f"split frame {k}") == 0
        s.release_stream(st.cuda_stream)
