"""The frame kernel's packet index arithmetic on the GPU: which tile, pixel and quadrant a wave
takes (rt_internal.h packet_sel / sel_tile / order_slot by host-computed multipliers, the tile
coordinates kept in the wave's LDS block, rt_kernels.hip wave_pixel) under every branch of it,
against the CPU oracle bit for bit — 0 differing channels — with the oracle's ray counts.

Frames of 1x1, 8x8, 9x7, 17x23, 64x40 and 136x72 pixels: one tile, tiles_x = 1, an odd
tiles_x, ragged right and bottom edges, an odd number of tile rows for the 2x1 workgroup units;
and 32x16, a second size (beside 64x40) whose whole frame and row subsets into pinned memory meet
launch_variant's pair_rows conditions (width a multiple of 16, an even tiles_x, block order), so
that pair_write, which takes the unit's left tile from the wave's kept coordinates, runs on
frames of 4 and 8 tiles across, one and several tile rows.
Two scenes carry all seven as cameras: `soup` (meshes, loose triangles, spheres: the SPHERES
kernels; 4 lights) and `hf` (a height field under one light, the kernel variant of the
benchmark's frame, with a wide near plane so that the sky tiles cost next to nothing and warm
frames split the heavy ones).  Each is rendered as a whole frame cold and warm (cold order, then
the previous frame's order), as row subsets, tile ranges with tile_step > 1, tile-major, as the
2x2 block deal, as pixel records (their ray counts too), into a pinned host buffer (pair_rows at
64x40 and 32x16: the pinned cases of test_row_subsets for cameras 4 and 6; every other size
fails a pair_rows condition and each wave writes its own tile) and, `hf`, warm on a stream of
its own where heavy tiles run as quadrant waves.  `soup2` (2 lights) and `soup33`
(33 lights, two occlusion words) compare the light loop's later iterations with the oracle.

Ray counts of a partial render are the oracle's over the pixels rendered: one primary ray per
pixel, one hit per pixel whose primary record is a hit, and one shadow ray per hit and light.

Quadrant waves: whether a warm frame splits depends on the tile times the frame before it
measured, and the library has no entry that reads a stream's order lists back.  So the frames
whose split is asserted are rendered by the RT_DIAG build of the same kernels in one child
process (tools/split_frames.py), which keeps each of three consecutive frames of the 64x40 and
136x72 `hf` cameras together with the number of waves that rendered it: a warm frame with more
waves than packets dispatched split entries, and those very frames, and their ray counts, must
be the oracle's.  (A frame of one tile cannot split: its only tile is the median.)
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

pytestmark = pytest.mark.gpu

THREADS = 8
SIZES = [(1, 1), (8, 8), (9, 7), (17, 23), (64, 40), (136, 72), (32, 16)]
ROW_SUBSETS = [(0, 1), (2, 1), (0, 3), (2, 3)]
RANGES = [(0, 1), (1, 3), (2, 4), (0, 2)]


def cameras(pose, near, sizes):
    return [G.Camera(*pose, near, 1, w, h, f"{w}x{h}.png") for w, h in sizes]


def soup_spec(seed, n_lights, sizes):
    spec = G.soup_scene(seed, 8, 8, n_lights=n_lights)
    spec.cameras = cameras(((0.2, 0.4, 0.5), (0, -0.15, -1), (0, 1, 0)), (-0.8, 0.8, -0.8, 0.8),
                           sizes)
    return spec


def hf_spec():
    spec = G.heightfield_scene(33, 32, 32)
    spec.cameras = cameras(((0, 1.5, -5), (0, -1, 0), (0, 0, -1)), (-2, 2, -2, 2), SIZES)
    return spec


SPECS = {"soup": lambda: soup_spec(31, 3, SIZES), "hf": hf_spec,
         "soup2": lambda: soup_spec(32, 1, [(17, 23), (64, 40)]),
         "soup33": lambda: soup_spec(33, 32, [(9, 7), (17, 23)])}
LIGHTS = {"soup": 4, "hf": 1, "soup2": 2, "soup33": 33}
FRAMES = [(n, c) for n in ("soup", "hf") for c in range(len(SIZES))]


def scene_xml(directory, name):
    path = os.path.join(directory, f"coords_{name}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(SPECS[name]().to_xml())
    return path


@pytest.fixture(scope="module")
def world(scene_dir):
    """name -> (the GPU scene, oracle(camera) -> (frame, stats, hit mask)), opened once."""
    import ceng795_amd
    from oracle.cpu_ref import OracleScene
    opened = {}

    def get(name):
        if name not in opened:
            xml = scene_xml(scene_dir, name)
            o = OracleScene(xml)

            @functools.lru_cache(maxsize=None)
            def oracle(camera):
                frame, st = o.render(camera, threads=THREADS)
                hit = o.primary_records(camera)[..., 7] == 1.0
                frame.setflags(write=False)
                return frame, st, hit
            s = ceng795_amd.Scene(xml, traversal="fast")
            assert s.num_lights == LIGHTS[name]
            opened[name] = (s, oracle, o)
        return opened[name][:2]
    yield get
    for s, _, o in opened.values():
        s.close()
        o.close()


def same_counts(got, pixels, hit, lights, what):
    """`got` (rt_stats) = the oracle's counts over the boolean pixel mask `pixels`."""
    print(what, got.primary_rays, got.primary_hits, got.shadow_rays)
    hits = int((hit & pixels).sum())
    assert got.primary_rays == int(pixels.sum()), what
    assert got.primary_hits == hits, what
    assert got.shadow_rays == hits * lights, what


def stream_of():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name,camera", FRAMES + [("soup2", 0), ("soup2", 1), ("soup33", 0),
                                                  ("soup33", 1)])
def test_whole_frame_cold_and_warm(world, name, camera):
    """rt_render twice (the cold order, then the order the first frame left), then three frames
    on a stream of this test's own (cold, warm, warm: split entries where the costs call for
    them)."""
    import torch
    s, oracle = world(name)
    ref, st, hit = oracle(camera)
    everything = np.ones(hit.shape, bool)
    assert st.primary_rays == hit.size and st.primary_hits == int(hit.sum())
    assert st.shadow_rays == int(hit.sum()) * LIGHTS[name]
    for k in range(2):
        got, gst = s.render_image(camera)
        assert assert_parity(got, ref, f"{name}:{camera} rt_render {k}") == 0
        same_counts(gst, everything, hit, LIGHTS[name], f"{name}:{camera} rt_render {k}")
    stream = torch.cuda.Stream()
    buf = torch.empty(ref.shape, dtype=torch.float32, device="cuda")
    s.collect_stats()
    for k in range(3):
        buf.fill_(-1.0)
        torch.cuda.synchronize()
        s.render_device(camera, buf.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert assert_parity(buf.cpu().numpy(), ref, f"{name}:{camera} frame {k}") == 0
        same_counts(s.collect_stats(), everything, hit, LIGHTS[name], f"{name}:{camera} frame {k}")
    s.release_stream(stream.cuda_stream)


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("name,camera", FRAMES)
def test_row_subsets(world, name, camera, pinned):
    """render_image(cam, px, starting_row, height_increase) writes exactly those rows; into
    page-locked memory the frame kernel writes the caller's buffer itself (64x40 and 32x16: pair_rows,
    two tiles' rows per workgroup)."""
    import torch
    s, oracle = world(name)
    ref, _, hit = oracle(camera)
    for start, stride in ROW_SUBSETS:
        if start >= ref.shape[0]:
            continue  # (a 1-row frame has no row 2)
        buf = torch.full(ref.shape, -7.0, dtype=torch.float32)
        if pinned:
            buf = buf.pin_memory()
        for k in range(2):  # cold, then warm
            got, gst = s.render_image(camera, buf.numpy(), start, stride)
            rows = np.arange(ref.shape[0])
            sel = (rows >= start) & ((rows - start) % stride == 0)
            what = f"{name}:{camera} rows {start}+{stride}k pinned={pinned} {k}"
            assert np.array_equal(got[sel].view(np.uint32), ref[sel].view(np.uint32)), what
            assert np.all(got[~sel] == -7.0), what
            same_counts(gst, np.broadcast_to(sel[:, None], hit.shape), hit, LIGHTS[name], what)


def tile_of(ref, x, y):
    """Tile (x, y) of the frame as the tile-major layout holds it: zeros outside the frame."""
    exp = np.zeros((8, 8, 3), np.float32)
    blk = ref[y * 8:y * 8 + 8, x * 8:x * 8 + 8]
    exp[:blk.shape[0], :blk.shape[1]] = blk
    return exp


def tile_mask(shape, tiles):
    m = np.zeros(shape, bool)
    for x, y in tiles:
        m[y * 8:y * 8 + 8, x * 8:x * 8 + 8] = True
    return m


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("name,camera", FRAMES)
def test_tile_ranges_tile_major(world, name, camera, blocks):
    """Deal units tile_begin + k tile_step, tile-major: tiles, or 2x2 blocks of tiles in deal
    order (RT_TILE_BLOCKS; tiles of a block outside the tile grid are zeros)."""
    import torch
    from ceng795_amd import dist_tiles
    s, oracle = world(name)
    ref, _, hit = oracle(camera)
    h, w, _ = ref.shape
    tx, ty = (w + 7) // 8, (h + 7) // 8
    total = ((tx + 1) // 2) * ((ty + 1) // 2) if blocks else s.num_tiles(camera)
    assert blocks or total == tx * ty
    for begin, step in RANGES:
        units = list(range(begin, total, step))
        if not units:
            continue  # (the range starts past the frame's last unit)
        if blocks:
            tiles = [dist_tiles.deal_block_tile(tx, u, k) for u in units for k in range(4)]
        else:
            tiles = [(t % tx, t // tx) for t in units]
        out = torch.full((len(tiles) * 64 * 3,), -1.0, dtype=torch.float32, device="cuda")
        s.collect_stats()
        for k in range(2):  # cold, then warm
            s.render_device(camera, out.data_ptr(), tile_begin=begin, tile_step=step,
                            tile_major=True, blocks=blocks, stream=stream_of())
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(len(tiles), 8, 8, 3)
            what = f"{name}:{camera} units {begin}+{step}k blocks={blocks} {k}"
            for i, (x, y) in enumerate(tiles):
                exp = tile_of(ref, x, y) if x < tx and y < ty else np.zeros((8, 8, 3), np.float32)
                assert np.array_equal(got[i].view(np.uint32), exp.view(np.uint32)), (what, x, y)
            same_counts(s.collect_stats(), tile_mask(hit.shape, tiles), hit, LIGHTS[name], what)


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("name,camera", FRAMES)
def test_pixel_records(world, name, camera, blocks):
    """RT_TILE_RECORDS: the frame kernel writes one 32-bit record per pixel, rt_resolve_device
    shades them into the frame."""
    import torch
    s, oracle = world(name)
    ref, _, hit = oracle(camera)
    everything = np.ones(hit.shape, bool)  # (the deal's padding tiles hold no pixel)
    h, w, _ = ref.shape
    tx, ty = (w + 7) // 8, (h + 7) // 8
    slot = 4 * ((tx + 1) // 2) * ((ty + 1) // 2) if blocks else tx * ty
    assert s.records_ok(camera)
    gathered = torch.full((1, slot, 64), -1.0, dtype=torch.float32, device="cuda")
    frame = torch.full(ref.shape, -1.0, dtype=torch.float32, device="cuda")
    s.collect_stats()
    for k in range(2):
        s.render_device(camera, gathered.data_ptr(), tile_major=True, blocks=blocks, records=True,
                        stream=stream_of())
        torch.cuda.synchronize()
        same_counts(s.collect_stats(), everything, hit, LIGHTS[name],
                    f"{name}:{camera} records blocks={blocks} {k}")
        s.resolve_device(camera, 1, slot, gathered.data_ptr(), frame.data_ptr(), blocks=blocks,
                         stream=stream_of())
        torch.cuda.synchronize()
        assert assert_parity(frame.cpu().numpy(), ref, f"{name}:{camera} records {blocks} {k}") == 0


SPLIT_CAMERAS = [4, 5]  # 64x40 and 136x72


def test_warm_frames_dispatch_split_entries(world, scene_dir, tmp_path):
    args = [f"{scene_xml(scene_dir, 'hf')}:{c}:3" for c in SPLIT_CAMERAS]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "split_frames.py"),
                        str(tmp_path), *args],
                       env=dict(os.environ, CENG795_LIB="diag"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _, oracle = world("hf")
    for k, per in enumerate(json.loads(r.stdout.strip().splitlines()[-1])):
        print(json.dumps(per))
        ref, st, _ = oracle(per["camera"])
        waves = per["waves"]
        assert waves[0] == per["packets"]  # cold: one wave per packet
        assert min(waves[1:]) > per["packets"]  # every warm frame dispatched split entries
        for f in range(len(waves)):
            got = np.load(os.path.join(str(tmp_path), f"{k}_{f}.npy"))
            assert assert_parity(got, ref, f"hf:{per['camera']} frame {f}, {waves[f]} waves") == 0
            assert per["ray counts"][f] == [st.primary_rays, st.primary_hits, st.shadow_rays]
