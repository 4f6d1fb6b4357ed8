"""The primary hit stays on chip across the frame kernel's three phases (rt_kernels.hip
primary_packet / shadow_packet / shade_pixel): the leaf waits in the low word of the lane's key in the
wave's LDS block (-1 a miss, -2 a lane outside the image or the packet), the shadow walks keep
their any-hit flag in the key's high word, and no hit record goes through memory.  Every frame
must be the oracle's, bit for bit, in both traversals.

Cases (tools/gen_scene.py specs):
  * the soup at 8x8, 9x7 and 17x9 — whole tiles, and ragged ones whose outside lanes carry -2 —
    without and with spheres; single packets mix hits and misses (asserted on the oracle's hits);
  * 1, 2 and 33 lights (33: two occlusion words, the flag word cleared per light while the leaf
    must survive), the soup's own occluders shadowing some pixels from some lights only (asserted
    on the pixel records' light bits);
  * one 8x8 packet whose hit lanes use two materials, and one with a single material, phong
    exponents 7 and 17.5;
  * pixel records, row-major and tile-major, against the RGB frame resolved from them;
  * the pinned rt_render path (pair_rows) on a 16x8 frame;
  * a split launch: a dense soup behind one tile of a 64x40 frame, background elsewhere, three
    frames on one stream from the RT_DIAG build (tools/split_frames.py counts the waves)."""
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
SIZES = [(8, 8), (9, 7), (17, 9)]
TRAVERSALS = ["fast", "reference"]


def soup_lights(n):
    """The soup's own lights first (the last of them below the floor), then more around it."""
    own = G.soup_scene(12, 8, 8).lights
    pool = [own[0], own[3], own[1], own[2]]
    rng = random.Random(1495)
    while len(pool) < n:
        pool.append(((round(rng.uniform(-3, 3), 3), round(rng.uniform(-1, 4), 3),
                      round(rng.uniform(-6, 0), 3)),
                     (rng.choice([30, 60, 100]), rng.choice([30, 60, 100]), 50)))
    return pool[:n]


def soup_spec(w, h, spheres, lights):
    spec = G.soup_scene(12, w, h, n_spheres=6 if spheres else 0)
    spec.lights = soup_lights(lights)
    return spec


def quad_spec(two_materials):
    """One 8x8 packet: a quad of two triangles over the lower left of the view (the rest misses),
    the triangles of two materials or of one, and a small occluder between it and the lights."""
    mats = [G.Material(ambient=(0.2, 0.3, 0.4), diffuse=(0.7, 0.5, 0.3), specular=(0.9, 0.8, 0.7),
                       phong=7),
            G.Material(ambient=(0.5, 0.1, 0.2), diffuse=(0.2, 0.6, 0.9), specular=(0.4, 0.9, 0.5),
                       phong=17.5)]
    other = 2 if two_materials else 1
    verts = ["-1.5 -1.5 -1.6", "0.8 -1.5 -1.7", "0.8 0.6 -1.65", "-1.5 0.6 -1.55",
             "-0.4 -0.2 -1.2", "0.1 -0.2 -1.2", "-0.15 0.2 -1.25"]
    return G.SceneSpec(
        cameras=[G.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), (-1, 1, -1, 1), 1, 8, 8, "quad.png")],
        ambient=(20, 25, 30), background=(5, 6, 7),
        lights=[((0.5, 1.5, 0), (90, 80, 70)), ((-1, 0.2, -0.5), (40, 50, 60))],
        materials=mats, vertex_text="\n".join(verts),
        triangles=[(1, (1, 2, 3)), (other, (1, 3, 4)), (other, (5, 6, 7))])


def heavy_tile_spec():
    """64x40: 1,500 small triangles behind tile (3, 2) — the view's x in [-0.2, 0], y in
    [-0.1, 0.1] at the near plane — and background everywhere else."""
    rng = random.Random(14)
    verts, tris = [], []
    for _ in range(1500):
        z = rng.uniform(-5.0, -3.6)
        cx, cy = rng.uniform(-0.19, -0.01) * -z, rng.uniform(-0.09, 0.09) * -z
        for _ in range(3):
            verts.append("%.6f %.6f %.6f" % (cx + rng.uniform(-0.04, 0.04),
                                             cy + rng.uniform(-0.04, 0.04),
                                             z + rng.uniform(-0.04, 0.04)))
        tris.append((1 + len(tris) % 2, (len(verts) - 2, len(verts) - 1, len(verts))))
    return G.SceneSpec(
        cameras=[G.Camera((0, 0, 0), (0, 0, -1), (0, 1, 0), (-0.8, 0.8, -0.5, 0.5), 1, 64, 40,
                          "heavy.png")],
        ambient=(20, 20, 20), background=(3, 5, 8),
        lights=[((1, 2, 0), (300, 300, 300)), ((-2, -1, -1), (200, 150, 100))],
        materials=[G.Material(ambient=(1, 1, 1), diffuse=(1, 1, 1), specular=(1, 1, 1), phong=3),
                   G.Material(ambient=(0.3, 0.2, 0.1), diffuse=(0.2, 0.5, 0.8),
                              specular=(0.5, 0.5, 0.5), phong=1)],
        vertex_text="\n".join(verts), triangles=tris)


def write_xml(directory, name, make):
    path = os.path.join(directory, f"handoff_{name}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(make().to_xml())
    return path


@functools.lru_cache(maxsize=None)
def oracle_of(xml):
    """Per camera: the oracle's frame and its primary hit mask (computed once per scene)."""
    from oracle.cpu_ref import OracleScene
    o = OracleScene(xml)
    return [(o.render(c, threads=THREADS)[0], o.primary_records(c)[..., 7] > 0)
            for c in range(o.num_cameras)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def mixed_packets(hit):
    """8x8 tiles of the frame that hold both a hit and a miss."""
    h, w = hit.shape
    tiles = [hit[y:y + 8, x:x + 8] for y in range(0, h, 8) for x in range(0, w, 8)]
    return sum(1 for t in tiles if t.any() and not t.all())


def check_frames(xml, what, min_mixed=1):
    """Every camera in both traversals, cold and then twice warm on one stream."""
    import torch
    import ceng795_amd
    refs = oracle_of(xml)
    assert sum(mixed_packets(hit) for _, hit in refs) >= min_mixed, what
    with ceng795_amd.Scene(xml) as s:
        st = torch.cuda.Stream()
        for mode in TRAVERSALS:
            s.set_traversal(mode)
            for cam, (ref, _) in enumerate(refs):
                bufs = [torch.full(ref.shape, -7.0, dtype=torch.float32, device="cuda")
                        for _ in range(3)]
                st.wait_stream(torch.cuda.current_stream())  # the fills come first
                for b in bufs:
                    s.render_device(cam, b.data_ptr(), stream=st.cuda_stream)
                torch.cuda.synchronize()
                for k, b in enumerate(bufs):
                    assert same_bits(b.cpu().numpy(), ref), (what, mode, cam, k)
        s.release_stream(st.cuda_stream)


@pytest.mark.parametrize("spheres", [False, True], ids=["triangles", "spheres"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_sizes(scene_dir, size, spheres):
    w, h = size
    name = f"soup_{w}x{h}_{int(spheres)}_2"
    check_frames(write_xml(scene_dir, name, lambda: soup_spec(w, h, spheres, 2)), name)


@pytest.mark.parametrize("lights", [1, 2, 33])
def test_light_counts(scene_dir, lights):
    name = f"soup_17x9_1_{lights}"
    check_frames(write_xml(scene_dir, name, lambda: soup_spec(17, 9, True, lights)), name)


@pytest.mark.parametrize("two", [True, False], ids=["two_materials", "one_material"])
def test_materials_of_one_packet(scene_dir, two):
    name = f"quad_{int(two)}"
    xml = write_xml(scene_dir, name, lambda: quad_spec(two))
    check_frames(xml, name)
    if two:  # both materials are among the packet's hit lanes: against the one-material frame
        # some hit pixels change colour (the second material's) and some do not (the first's)
        ref, hit = oracle_of(xml)[0]
        one = oracle_of(write_xml(scene_dir, "quad_0", lambda: quad_spec(False)))[0][0]
        changed = (ref.view(np.uint32) != one.view(np.uint32)).any(-1)
        assert (hit & changed).any() and (hit & ~changed).any() and not hit.all()


def test_pixel_records(scene_dir):
    """render_device(records=True), row-major and tile-major, and the frames resolved from them."""
    import torch
    import ceng795_amd
    xml = write_xml(scene_dir, "soup_17x9_1_2", lambda: soup_spec(17, 9, True, 2))
    refs = oracle_of(xml)
    stream = torch.cuda.current_stream().cuda_stream
    partly = 0  # hit pixels in the shadow of exactly one of the two lights
    with ceng795_amd.Scene(xml) as s:
        for mode in TRAVERSALS:
            s.set_traversal(mode)
            for cam, (ref, hit) in enumerate(refs):
                assert s.records_ok(cam)
                h, w, _ = ref.shape
                tiles = s.num_tiles(cam)
                rows = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
                major = torch.full((1, tiles, 64), -1, dtype=torch.int32, device="cuda")
                frames = [torch.full(ref.shape, -7.0, dtype=torch.float32, device="cuda")
                          for _ in range(2)]
                s.render_device(cam, rows.data_ptr(), records=True, stream=stream)
                s.render_device(cam, major.data_ptr(), tile_major=True, records=True,
                                stream=stream)
                s.resolve_rows(cam, 0, h, rows.data_ptr(), frames[0].data_ptr(), stream=stream)
                s.resolve_device(cam, 1, tiles, major.data_ptr(), frames[1].data_ptr(),
                                 stream=stream)
                torch.cuda.synchronize()
                rec = rows.cpu().numpy().view(np.uint32)
                assert np.array_equal(rec >> 30 == 0, hit), (mode, cam)  # rt_internal.h kRec*
                bits = (rec[hit] >> 26) & 15
                assert bits.max(initial=0) <= 3
                partly += int(((bits == 1) | (bits == 2)).sum())
                tx = (w + 7) // 8
                got = major.cpu().numpy().view(np.uint32).reshape(tiles, 8, 8)
                for t in range(tiles):
                    y0, x0 = (t // tx) * 8, (t % tx) * 8
                    part = rec[y0:y0 + 8, x0:x0 + 8]
                    assert np.array_equal(got[t, :part.shape[0], :part.shape[1]], part), \
                        (mode, cam, t)
                for k, f in enumerate(frames):
                    assert same_bits(f.cpu().numpy(), ref), \
                        (mode, cam, "rows" if k == 0 else "tiles")
    assert partly > 0, "no pixel is shadowed from one light only"


def test_pinned_pair_rows_frame(scene_dir):
    """rt_render into pinned host memory: a 16x8 frame is one workgroup's two tiles, written as
    whole 16-pixel rows from the colours staged in the waves' LDS."""
    import torch
    import ceng795_amd
    xml = write_xml(scene_dir, "soup_16x8_1_2", lambda: soup_spec(16, 8, True, 2))
    refs = oracle_of(xml)
    with ceng795_amd.Scene(xml) as s:
        for mode in TRAVERSALS:
            s.set_traversal(mode)
            for cam, (ref, _) in enumerate(refs):
                buf = torch.full(ref.shape, -7.0, dtype=torch.float32).pin_memory()
                for k in range(2):
                    got, _ = s.render_image(cam, buf.numpy())
                    assert same_bits(got, ref), (mode, cam, k)


def test_split_tile_frames(scene_dir, tmp_path):
    """Warm frames of a scene with one tile far heavier than the rest run that tile as four
    quadrant waves (lanes 0..15 hold pixels, the rest -2); the frames kept are those very frames."""
    xml = write_xml(scene_dir, "heavy_tile", heavy_tile_spec)
    ref, hit = oracle_of(xml)[0]
    assert hit[16:24, 24:32].any() and not hit[:8].any() and not hit[32:].any()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "split_frames.py"),
                        str(tmp_path), f"{xml}:0:3"],
                       env=dict(os.environ, CENG795_LIB="diag"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    per = json.loads(r.stdout.strip().splitlines()[-1])[0]
    print(json.dumps(per))
    waves = per["waves"]
    for f in range(len(waves)):
        got = np.load(os.path.join(str(tmp_path), f"0_{f}.npy"))
        assert same_bits(got, ref), (f, waves[f])
    assert waves[0] == per["packets"]  # cold: one wave per packet
    if max(waves[1:]) <= per["packets"]:
        pytest.skip(f"the order kernel split no tile of the warm frames (waves {waves})")
