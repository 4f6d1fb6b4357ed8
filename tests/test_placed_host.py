"""Scenes far from the origin and off unit scale (scenes.PLACED, tests/placed.py), CPU only.

Three things are held here, so that tests/test_gpu_placed.py can compare the kernels with the
oracle on these scenes:
  * the oracle is pinned to the reference on them: every frame, ray count and BVH dump equals
    what the unmodified reference produced (tests/golden/make_golden_placed.py);
  * the inputs are not vacuous: frames finite, camera 0 sees geometry, a placement that is not
    an exact rescaling is a different computation, and an exact rescaling of a triangle scene
    is the same one bit for bit (which validates placed());
  * the library's host side is sound on them: its BVH equals the reference's and its culling
    tree passes check_accel, whose containment test is exact.  At scales
    2^-31 .. 2^-34 the encoder used to round `guard plane - margin` to nearest, into the box it
    must contain.

Cameras dropped from a case because the oracle's frame is not finite: none.  Combinations left
out of the table for that reason (camera 0 itself is not finite): scenes.PLACED_LEFT_OUT."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import scenes
from ceng795_amd import _lib
from ceng795_amd.scene import host_dump_bvh
from oracle.cpu_ref import OracleScene

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden_placed.json")))
ARRAYS = np.load(os.path.join(HERE, "golden", "golden_placed.npz"))
THREADS = min(8, os.cpu_count() or 1)
MSAA_SEED = 1

BASES = list(scenes.PLACED_BASE_SCENES)
NAMES = BASES + list(scenes.PLACED)
# name -> the one camera left out (never camera 0); empty: every oracle frame is finite
DROPPED = {}


def kept_cameras(name, count):
    return [c for c in range(count) if c != DROPPED.get(name)]


def is_msaa(name):
    return scenes.placed_parts(name)[0] == "msaa"


@functools.lru_cache(maxsize=None)
def oracle_scene(xml):
    return OracleScene(xml)


@functools.lru_cache(maxsize=None)
def oracle_frame(xml, cam, msaa):
    o = oracle_scene(xml)
    if msaa:
        return o.render_msaa(cam, seed=MSAA_SEED, threads=THREADS)
    return o.render(cam, threads=THREADS)


def frame(scene_dir, name, cam):
    return oracle_frame(scenes.write(name, scene_dir), cam, is_msaa(name))


def centre_rays(scene_dir, name, cam):
    """(rays, hits) of the pixel-centre rays: what the harness counts, MSAA camera or not."""
    o = oracle_scene(scenes.write(name, scene_dir))
    hits = int((o.primary_records(cam)[..., 7] == 1.0).sum())
    return hits, hits * o.num_lights + o.camera(cam).width * o.camera(cam).height


def test_table_is_base_times_placement():
    assert set(GOLDEN) - {"_about"} == set(NAMES)
    assert not set(DROPPED) - set(NAMES) and 0 not in DROPPED.values()
    per_base = {b: [n for n in scenes.PLACED if scenes.placed_parts(n)[0] == b]
                for b in scenes.PLACED_BASES}
    assert len(per_base["soup"]) == len(per_base["hf"]) == len(scenes.PLACEMENTS) == 11
    assert sorted(scenes.placed_parts(n)[1] for n in per_base["msaa"]) == ["small", "t1e5"]
    # left out: the reference's own depth-3 frame is not finite (scale 2^20; and scale 1234.5
    # at offsets of 2e6 .. 9e6, camera 0 included)
    assert scenes.PLACED_LEFT_OUT == {("depth3", "s2p20"), ("depth3", "big")}
    assert len(per_base["depth3"]) == 9
    for name in NAMES:
        spec = {**scenes.PLACED, **scenes.PLACED_BASE_SCENES}[name][0]()
        assert all(c.width <= 48 and c.height <= 48 for c in spec.cameras), name


@pytest.mark.parametrize("name", NAMES)
def test_scene_text_matches_golden(scene_dir, name):
    """The generator and placed() still write the exact XML the fixture was made from."""
    xml = scenes.write(name, scene_dir)
    assert hashlib.sha256(open(xml, "rb").read()).hexdigest() == GOLDEN[name]["xml_sha256"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_reference_frames(scene_dir, name):
    g = GOLDEN[name]
    o = oracle_scene(scenes.write(name, scene_dir))
    assert o.num_cameras == len(g["cameras"])
    recursive = scenes.placed_parts(name)[0] == "depth3"
    for cam in kept_cameras(name, o.num_cameras):
        gc = g["cameras"][cam]
        assert gc["finite"], (name, cam)
        img, st = frame(scene_dir, name, cam)
        assert img.shape == (gc["height"], gc["width"], 3)
        assert centre_rays(scene_dir, name, cam)[1] == gc["rays"]
        if is_msaa(name):
            # the reference seeds MSAA pixels from the wall clock: test_msaa_oracle.py's pin, the
            # oracle as close to two reference frames as they are to each other
            ref0, ref1 = ARRAYS[f"{name}__{cam}__ref0"], ARRAYS[f"{name}__{cam}__ref1"]
            floor = np.abs(ref0 - ref1).mean()
            err = 0.5 * (np.abs(img - ref0).mean() + np.abs(img - ref1).mean())
            assert err <= 1.3 * floor + 0.05, (name, cam, err, floor)
            assert abs(float((img - 0.5 * (ref0 + ref1)).mean())) <= 0.25 * floor + 0.05
            continue
        y0, x0 = gc["crop_origin"]
        crop = ARRAYS[f"{name}__{cam}__crop"]
        assert np.array_equal(img[y0:y0 + crop.shape[0], x0:x0 + crop.shape[1]].view(np.uint32),
                              crop.view(np.uint32)), (name, cam)
        assert hashlib.sha256(img.tobytes()).hexdigest() == gc["frame_sha256"], (name, cam)
        if not recursive:  # the harness counts depth-0 rays only
            assert st.primary_rays + st.shadow_rays == gc["rays"]


@pytest.mark.parametrize("name", NAMES)
def test_bvh_dumps_match_reference(scene_dir, tmp_path, name):
    """The oracle's and the library's BVH (boxes as fp32 bits, leaf order) equal the reference's."""
    xml = scenes.write(name, scene_dir)
    out = tmp_path / "oracle.txt"
    oracle_scene(xml).dump_bvh(str(out))
    text = "\n".join(ln for ln in out.read_text().splitlines() if ln != "M") + "\n"
    assert hashlib.sha256(text.encode()).hexdigest() == GOLDEN[name]["bvh_sha256"]
    assert text.count("\n") == GOLDEN[name]["bvh_lines"]
    lib_out = tmp_path / "library.txt"
    host_dump_bvh(xml, str(lib_out))
    assert hashlib.sha256(lib_out.read_bytes()).hexdigest() == GOLDEN[name]["bvh_sha256"]


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_culling_tree_holds_its_invariants(scene_dir, name, K):
    """check_accel: no slot test culls a treelet the reference enters (containment with the
    margin, decided exactly)."""
    xml = scenes.write(name, scene_dir)
    st = (C.c_longlong * 4)()
    rc = _lib.lib().rt_host_check_accel_xml(xml.encode(), K, st)
    assert rc == 0, _lib.lib().rt_last_error().decode()
    treelets, nodes, depth, lone = list(st)
    assert treelets >= 2 and nodes >= 1 and depth >= 1 and lone <= treelets


# ------------------------------------------------------------------ the inputs say something
@pytest.mark.parametrize("name", NAMES)
def test_frames_are_finite_and_camera_0_sees_geometry(scene_dir, name):
    o = oracle_scene(scenes.write(name, scene_dir))
    kept = kept_cameras(name, o.num_cameras)
    assert 0 in kept and len(kept) >= o.num_cameras - 1
    for cam in kept:
        assert np.isfinite(frame(scene_dir, name, cam)[0]).all(), (name, cam)
    info = o.camera(0)
    cover = centre_rays(scene_dir, name, 0)[0] / (info.width * info.height)
    print(f"{name}: camera 0 hits geometry on {100 * cover:.1f} % of its pixels")
    if scenes.placed_parts(name)[0] == "hf":
        assert cover >= 0.90, (name, cover)
    else:
        assert 0.10 <= cover <= 0.90, (name, cover)


def bits_differing(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


@pytest.mark.parametrize("name", [n for n in scenes.PLACED
                                  if scenes.placed_parts(n)[1] not in scenes.POWER_OF_TWO])
def test_inexact_placement_is_another_computation(scene_dir, name):
    base = scenes.placed_parts(name)[0] + "@base"
    o = oracle_scene(scenes.write(name, scene_dir))
    for cam in kept_cameras(name, o.num_cameras):
        n = bits_differing(frame(scene_dir, name, cam)[0], frame(scene_dir, base, cam)[0])
        assert n >= 100, (name, cam, n)


@pytest.mark.parametrize("placement", ["s2m20", "s2p20"])
def test_exact_rescaling_of_triangles_keeps_every_bit(scene_dir, placement):
    """Triangles only and a power-of-two scale: every operation of the reference scales
    exactly, its absolute constants aside, so the frame is the base's.  This holds placed() to
    transforming everything that has a length, and by the right power."""
    got, gst = frame(scene_dir, f"hf@{placement}", 0)
    ref, rst = frame(scene_dir, "hf@base", 0)
    assert bits_differing(got, ref) == 0
    assert (gst.primary_hits, gst.shadow_rays) == (rst.primary_hits, rst.shadow_rays)


# ------------------------------------------------------------------ rays built from the root box
@pytest.mark.parametrize("family", ["interior", "surface"])
@pytest.mark.parametrize("name", ["soup@t1e5", "soup@s2m20"])
def test_ray_family_mix_conditions(scene_dir, name, family):
    """tests/ray_batches.py's `interior` and `surface` derive their rays from the scene's root
    box, hit points and epsilon: on the far and the tiny soup each still forces its branches both
    ways (check_mix, from the oracle alone), so test_gpu_placed.py runs both on both."""
    import ray_batches as rb
    xml = scenes.write(name, scene_dir)
    info = rb.scene_info(xml, name)
    b = rb.family(info, family)
    assert b.o.dtype == b.d.dtype == np.float32 and len(b) <= 8192
    assert np.isfinite(b.o).all() and np.isfinite(b.d).all()
    rec, shape = oracle_scene(xml).intersect_rays(b.o, b.d)
    print(name, family, rb.check_mix(info, b, rec, shape))
    assert not np.isnan(rec[:, 3]).any()
