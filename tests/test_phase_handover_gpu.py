"""What the frame kernel's phases hand to each other (rt_kernels.hip): the
hit point parked in the wave's LDS block where the primary walk ends, the last light's direction
taken from its shadow ray, a lone occlusion word kept in a register, and the divisions of a
normalize and of a light's terms sharing one reciprocal.  Every frame must stay the oracle's, bit
for bit.

Cases (tools/gen_scene.py specs with their `lights` replaced):
  * the soup at 75 x 53 (ragged tiles, lanes outside the image, spheres, misses) with 0, 1, 2, 4,
    32 and 33 lights — no shadow phase at all, one word of occlusion bits, and with 33 two words
    (the bits then go through memory, the last light's direction still comes from its ray);
  * heightfield_scene(32, 64, 48) with 1 and 3 lights (64 wide: pinned frames take pair_rows);
  * single_triangle and single_sphere: the root is a primitive.
Each case: every camera cold and then twice warm on one stream (ordered dispatch, split tiles),
camera 0 as two tile subsets and into a pinned host buffer, its pixel records where the scene has
at most four lights, and on the soups camera 0's rays as radiance queries (the shared shade_hit).
The last test runs the device's own check of the shared-reciprocal forms against `/`."""
import functools
import os
import random
import sys

import numpy as np
import pytest

import rq_util
from conftest import ROOT, assert_parity
from test_gpu_records import assembled

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
HF_LIGHTS = [((0, 4, -5), (1000, 1000, 1000)), ((-4, 2, -3), (600, 500, 400)),
             ((3, 1, -7), (300, 500, 700))]


def soup_lights(n):
    """The soup's own four lights (the second one below the floor: back-lit faces), then lights
    drawn around the scene the way soup_scene draws its own."""
    own = G.soup_scene(12, 75, 53).lights
    pool = [own[0], own[3], own[1], own[2]]
    rng = random.Random(795)
    while len(pool) < n:
        pool.append(((round(rng.uniform(-3, 3), 3), round(rng.uniform(-1, 4), 3),
                      round(rng.uniform(-6, 0), 3)),
                     (rng.choice([30, 60, 100]), rng.choice([30, 60, 100]), 50)))
    return pool[:n]


def spec_of(case):
    kind, n = case
    if kind == "soup":
        spec = G.soup_scene(12, 75, 53)
        spec.lights = soup_lights(n)
    elif kind == "hf":
        spec = G.heightfield_scene(32, 64, 48)
        spec.lights = HF_LIGHTS[:n]
    elif kind == "triangle":
        spec = G.single_triangle_scene(64, 64)
    else:
        spec = G.single_sphere_scene(64, 64)
    assert n is None or len(spec.lights) == n
    return spec


SOUPS = [("soup", n) for n in (0, 1, 2, 4, 32, 33)]
CASES = SOUPS + [("hf", 1), ("hf", 3), ("triangle", None), ("sphere", None)]
RECORD_CASES = [c for c in CASES if c[1] is None or c[1] <= 4]


def case_id(case):
    return case[0] if case[1] is None else f"{case[0]}{case[1]}"


def scene_xml(directory, case):
    path = os.path.join(directory, f"handover_{case_id(case)}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(spec_of(case).to_xml())
    return path


@functools.lru_cache(maxsize=None)
def oracle_frames(xml):
    from oracle.cpu_ref import OracleScene
    o = OracleScene(xml)
    return [o.render(c, threads=THREADS)[0] for c in range(o.num_cameras)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                          np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def rt():
    import ceng795_amd
    return ceng795_amd


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cold_and_warm_frames_match_oracle(rt, scene_dir, case):
    import torch
    xml = scene_xml(scene_dir, case)
    refs = oracle_frames(xml)
    with rt.Scene(xml) as s:
        assert s.num_lights == len(spec_of(case).lights)
        st = torch.cuda.Stream()
        for cam, ref in enumerate(refs):
            bufs = [torch.full(ref.shape, -7.0, dtype=torch.float32, device="cuda")
                    for _ in range(3)]
            st.wait_stream(torch.cuda.current_stream())  # the fills come first
            for b in bufs:
                s.render_device(cam, b.data_ptr(), stream=st.cuda_stream)
            torch.cuda.synchronize()
            for k, b in enumerate(bufs):
                assert same_bits(b.cpu().numpy(), ref), (case, cam, "cold" if k == 0 else "warm")
        s.release_stream(st.cuda_stream)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tile_subsets_match_oracle(rt, scene_dir, case):
    import torch
    xml = scene_xml(scene_dir, case)
    ref = oracle_frames(xml)[0]
    h, w, _ = ref.shape
    tx = (w + 7) // 8
    with rt.Scene(xml) as s:
        total = s.num_tiles(0)
        for begin in (0, 1):
            sel = list(range(begin, total, 2))
            out = torch.full((len(sel) * 64 * 3,), -1.0, dtype=torch.float32, device="cuda")
            s.render_device(0, out.data_ptr(), tile_begin=begin, tile_step=2, tile_major=True,
                            stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            tiles = out.cpu().numpy().reshape(len(sel), 8, 8, 3)
            for k, t in enumerate(sel):
                y0, x0 = (t // tx) * 8, (t % tx) * 8
                part = ref[y0:y0 + 8, x0:x0 + 8]
                assert same_bits(tiles[k, :part.shape[0], :part.shape[1]], part), (case, begin, t)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pinned_host_frame_matches_oracle(rt, scene_dir, case):
    import torch
    xml = scene_xml(scene_dir, case)
    ref = oracle_frames(xml)[0]
    with rt.Scene(xml) as s:
        buf = torch.full(ref.shape, -7.0, dtype=torch.float32).pin_memory()
        for k in range(2):
            got, _ = s.render_image(0, buf.numpy())
            assert same_bits(got, ref), (case, k)


@pytest.mark.parametrize("case", RECORD_CASES, ids=case_id)
def test_pixel_records_match_oracle(rt, scene_dir, case):
    xml = scene_xml(scene_dir, case)
    refs = oracle_frames(xml)
    with rt.Scene(xml) as s:
        assert all(s.records_ok(c) for c in range(s.num_cameras))
        for world in (1, 3):
            for inplace in (False, True):
                got = assembled(s, world, root_inplace=inplace)
                for c, (g, ref) in enumerate(zip(got, refs)):
                    what = f"{case_id(case)}/cam{c}/world{world}/inplace{inplace}"
                    assert assert_parity(g, ref, what) == 0, what


@pytest.mark.parametrize("case", SOUPS, ids=case_id)
def test_radiance_queries_give_the_frame(rt, scene_dir, case):
    xml = scene_xml(scene_dir, case)
    ref = oracle_frames(xml)[0]
    b = rq_util.oracle_batch(xml, cameras=[0])
    with rt.Scene(xml) as s:
        frame, _ = s.render_image(0)
        rad = s.shade_rays(b.o, b.d)
    assert same_bits(frame, ref), case
    assert same_bits(rad["rgb"], frame.reshape(-1, 3)), case


def test_shared_reciprocal_forms_are_ieee(rt):
    """normalize_shared and light_quotients give the bits of `/` on 2^22 random cases per seed
    (zero components, components below 2^-49, lengths and divisors outside [2^-40, 2^40], all-ones
    mantissas), and both their shared-reciprocal path and their `/` path were taken.  Mode 0 is
    the triangle test's check and reports no path counts."""
    import ctypes as C
    from ceng795_amd import _lib
    out = (C.c_longlong * 4)()
    n = 1 << 22
    for seed in (1, 2, 3):
        _lib.check(_lib.lib().rt_debug_quotient_check_mode(0, 1, seed, n, out))
        print(f"seed {seed}: mismatches {out[0]}, cases {out[1]}, shared {out[2]}, plain {out[3]}")
        assert out[1] == n
        assert out[0] == 0, f"seed {seed}: {out[0]} cases differ from IEEE division"
        assert out[2] + out[3] == 2 * n  # a normalize and a light's terms per case
        assert out[2] > n // 8 and out[3] > n // 8, list(out)
    _lib.check(_lib.lib().rt_debug_quotient_check_mode(0, 0, 1, 1 << 16, out))
    assert list(out) == [0, 1 << 16, 0, 0]
