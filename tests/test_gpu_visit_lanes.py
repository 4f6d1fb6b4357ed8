"""Lanes outside a wide-node visit's mask (rt_kernels.hip visit_wide).

The visit folds its lane mask `m` into the slab test: a lane outside `m` gets an exit plane at
-inf and a finite scale on axis 0, so its compare fails whatever its registers hold — 1/0 of a
zero direction component, a skipped axis's infinities, the ray of a pixel past the image's edge
or of another octant's sub-walk, a shadow ray that has already found its occluder.  Every frame
and query below is compared with the CPU oracle bit for bit, and the CPU part of each test
asserts that the case it is written for occurs and that hits and misses are both present:

  * partial packets: a height field of n = 24 and a 400-triangle soup with spheres and three
    lights at 13x11 and 70x9 pixels (tiles cut at the right and bottom edges);
  * a zero direction component: a 17x17 top-down camera with one pixel column at d_x = 0 exactly
    (skipped and unskipped lanes in one packet), and the same camera shifted so that the column
    of u = 0 is the tile column 20, past the image's 17;
  * all sign octants: two cameras inside the soup, gazing -z and +z, 16x16 pixels, with d_x and
    d_y changing sign inside the first tile: each sub-walk leaves the other octants' live rays
    outside `m`;
  * the `alive` mask: in the soup's shadow phase some packet has both occluded and unoccluded
    shadow rays towards one light, so lanes leave `alive` during the walk;
  * the per-lane (not COHERENT) instantiations: closest-hit and occlusion queries of
    64 * 3 + 37 rays of which every third has a zero or negative-zero component.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_scene as G  # noqa: E402
from rq_util import bits, occlusion, trace  # noqa: E402

F = np.float32
THREADS = 8
SIZES = [(13, 11), (70, 9)]
N_RAYS = 64 * 3 + 37


# ---------------------------------------------------------------- scenes
def soup():
    """400 mesh triangles, 12 loose ones, 6 spheres, three lights (two above, one below)."""
    return G.soup_scene(31, 16, 16, n_mesh_tris=400, n_lights=2)


def partial_spec(kind):
    if kind == "hf24":
        spec = G.heightfield_scene(24, 13, 11)
        pose = ((0, 1.5, -5), (0, -1, 0), (0, 0, -1))
        # the field spans u in (-0.86, 0.86): the wider plane leaves sky at the frame's sides
        plane = (-1.25, 1.25, -1.25, 1.25)
    else:
        spec = soup()
        pose = ((0.2, 0.4, 0.5), (0, -0.15, -1), (0, 1, 0))
        plane = (-0.8, 0.8, -0.8, 0.8)
        assert len(spec.lights) == 3 and len(spec.spheres) == 6
    spec.cameras = [G.Camera(*pose, plane, 1, w, h, f"{kind}_{w}x{h}.png") for w, h in SIZES]
    return spec


def zero_spec():
    """Top-down over the height field, pixels 1.5 wide on a near plane 8.5 away (every number of
    l + (i + 0.5) * (r - l) / 17 is a multiple of 0.25: exact in fp32 in any order; the field
    ends at |u| = 8.5, inside the frame): camera 0 has u = 0 at column 8, camera 1 — the plane
    shifted by 12 pixels — at column 20."""
    spec = G.heightfield_scene(24, 17, 17)
    pose = ((0, 1.5, -5), (0, -1, 0), (0, 0, -1))
    spec.cameras = [G.Camera(*pose, (-12.75, 12.75, -12.75, 12.75), 8.5, 17, 17, "zero_in.png"),
                    G.Camera(*pose, (-30.75, -5.25, -12.75, 12.75), 8.5, 17, 17, "zero_out.png")]
    return spec


def octant_spec():
    spec = soup()
    at = (0.1, 0.1, -4.0)
    # (left, right, bottom, top): u = 0 and v = 0 after 6 of 16 pixels, inside tile (0, 0)
    plane = (-1.5, 2.5, -2.5, 1.5)
    spec.cameras = [G.Camera(at, (0, 0, -1), (0, 1, 0), plane, 1, 16, 16, "oct_back.png"),
                    G.Camera(at, (0, 0, 1), (0, 1, 0), plane, 1, 16, 16, "oct_front.png")]
    return spec


SPECS = {"hf24": lambda: partial_spec("hf24"), "soup": lambda: partial_spec("soup"),
         "zero": zero_spec, "octant": octant_spec}


def scene_xml(directory, name):
    path = os.path.join(directory, f"visit_lanes_{name}.xml")
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(SPECS[name]().to_xml())
    return path


# ---------------------------------------------------------------- the oracle, once per frame
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


def octant(v):
    s = np.signbit(np.asarray(v, F)).astype(np.int64)
    return s[..., 0] | s[..., 1] << 1 | s[..., 2] << 2


def check_frame(xml, camera, what):
    """GPU frame == oracle frame in every bit, and the ray counts agree."""
    import ceng795_amd
    ref, st, _ = oracle_frame(xml, camera)
    hit = hit_mask(xml, camera)
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, gst = s.render_image(camera)
    differ = int((bits(got) != bits(ref)).any(axis=-1).sum())
    print(f"{what}: {hit.size} pixels, {int(hit.sum())} hit, {st.shadow_rays} shadow rays, "
          f"{differ} pixels differ")
    assert got.shape == ref.shape and differ == 0, what
    assert gst.primary_rays == st.primary_rays and gst.primary_hits == st.primary_hits, what
    assert gst.shadow_rays == st.shadow_rays, what


# ---------------------------------------------------------------- the cases, from the CPU alone
def hit_mask(xml, camera):
    hit = oracle_frame(xml, camera)[2][..., 7] == 1.0
    assert hit.any() and not hit.all(), (xml, camera)  # a pixel that hits and one that misses
    return hit


def case_partial(directory, name, camera):
    w, h = SIZES[camera]
    assert w % 8 and h % 8  # tiles cut on both edges
    xml = scene_xml(directory, name)
    _, st, rec = oracle_frame(xml, camera)
    assert rec.shape[:2] == (h, w) and st.shadow_rays > 0
    hit_mask(xml, camera)
    return xml


def case_zero_inside(directory):
    xml = scene_xml(directory, "zero")
    d = oracle_frame(xml, 0)[2][..., 0:3]
    assert (d[:, 8, 0] == 0).all() and (np.delete(d[..., 0], 8, axis=1) != 0).all()
    # the column's packets hold skipped (|d_x| < 1e-6) and unskipped lanes
    assert (np.abs(d[:, 9, 0]) > 1e-6).all()
    hit_mask(xml, 0)
    return xml


def case_zero_outside(directory):
    xml = scene_xml(directory, "zero")
    d = oracle_frame(xml, 1)[2][..., 0:3]
    assert (d[..., 0] != 0).all()  # no pixel of the image has d_x = 0 ...
    # ... and u = l + (i + 0.5) * (r - l) / 17 = 0 at i = 20: a lane of the last tile column
    cam = SPECS["zero"]().cameras[1]
    lo, hi = F(cam.near_plane[0]), F(cam.near_plane[1])
    assert lo + (F(20) + F(0.5)) * (hi - lo) / F(17) == 0 and 17 <= 20 < 24
    hit_mask(xml, 1)
    return xml


def case_octants(directory):
    xml = scene_xml(directory, "octant")
    seen = set()
    for camera in (0, 1):
        octs = octant(oracle_frame(xml, camera)[2][..., 0:3])
        first = set(octs[0:8, 0:8].ravel().tolist())
        assert len(first) == 4, (camera, first)  # d_x and d_y flip inside tile (0, 0)
        seen |= set(octs.ravel().tolist())
        hit_mask(xml, camera)
    assert seen == set(range(8))
    return xml


@functools.lru_cache(maxsize=None)
def shadow_mix(xml, camera):
    """Per light, the number of 8x8 packets whose hit pixels have both occluded and unoccluded
    shadow rays (built as the shading builds them: from the hit point, eps along the unit
    light vector, up to the light's distance less eps; fp32)."""
    from oracle.cpu_ref import OracleScene
    spec = SPECS["soup"]()
    rec = oracle_frame(xml, camera)[2]
    hit = rec[..., 7] == 1.0
    e = np.array(spec.cameras[camera].position, F)
    p = (e + rec[..., 0:3] * rec[..., 3:4]).astype(F)[hit]
    ys, xs = np.nonzero(hit)
    packet = (ys // 8) * 64 + xs // 8
    eps = F(spec.shadow_eps)
    o = OracleScene(xml)
    mixed = []
    for pos, _ in spec.lights:
        ld = (np.array(pos, F) - p).astype(F)
        dist = np.sqrt((ld * ld).sum(axis=1, dtype=F)).astype(F)
        wi = (ld / dist[:, None]).astype(F)
        srec, _ = o.intersect_rays((p + wi * eps).astype(F), wi)
        occ = (srec[:, 7] == 1.0) & (srec[:, 3] > 0) & (srec[:, 3] < dist - eps)
        mixed.append(sum(1 for k in np.unique(packet)
                         if occ[packet == k].any() and not occ[packet == k].all()))
    o.close()
    return tuple(mixed)


def case_alive(directory):
    xml = scene_xml(directory, "soup")
    mixed = shadow_mix(xml, 1)
    print("packets with occluded and unoccluded shadow rays, per light:", mixed)
    assert max(mixed) >= 2
    hit_mask(xml, 1)
    return xml


@functools.lru_cache(maxsize=None)
def query_rays(xml):
    """N_RAYS rays from points inside the soup's box; every third has one component set to 0.0
    or -0.0 (in turn, on a cycling axis).  Returns (o, d, the oracle's records, tmax, occluded):
    tmax is twice and half the oracle's t in turn and +inf on a miss."""
    from oracle.cpu_ref import OracleScene
    rng = np.random.default_rng(795)
    o = rng.uniform((-1.5, -0.5, -5.5), (1.5, 1.0, -2.5), (N_RAYS, 3)).astype(F)
    d = rng.normal(size=(N_RAYS, 3)).astype(F)
    d[:, 1] -= F(0.5)  # towards the mesh patch: more hits
    third = np.arange(0, N_RAYS, 3)
    d[third, (third // 3) % 3] = np.where((third // 9) % 2 == 0, F(0.0), F(-0.0))
    orc = OracleScene(xml)
    rec, _ = orc.intersect_rays(o, d)
    orc.close()
    hit, t = rec[:, 7] == 1.0, rec[:, 3]
    tmax = np.where(hit, np.where(np.arange(N_RAYS) % 2 == 0, t * F(2), t * F(0.5)),
                    F(np.inf)).astype(F)
    occ = (hit & (t > 0) & (t < tmax)).astype(np.uint8)
    for a in (o, d, rec, tmax, occ):
        a.setflags(write=False)
    return o, d, rec, tmax, occ


def case_rays(directory):
    xml = scene_xml(directory, "soup")
    o, d, rec, tmax, occ = query_rays(xml)
    hit, z = rec[:, 7] == 1.0, (d == 0).any(axis=1)
    assert len(o) == N_RAYS and z[::3].all() and not z[1::3].any() and not z[2::3].any()
    zeros = d[z][d[z] == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert hit.any() and not hit.all() and hit[z].any() and not hit[z].all()
    assert occ.any() and not occ.all() and occ[z].any() and not occ[z].all()
    return xml


def test_cases_occur(scene_dir):
    """No GPU: every scene and batch below holds the case it is there for."""
    for name in ("hf24", "soup"):
        for camera in range(len(SIZES)):
            case_partial(scene_dir, name, camera)
    case_zero_inside(scene_dir)
    case_zero_outside(scene_dir)
    case_octants(scene_dir)
    case_alive(scene_dir)
    case_rays(scene_dir)


# ---------------------------------------------------------------- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("camera", range(len(SIZES)))
@pytest.mark.parametrize("name", ["hf24", "soup"])
def test_partial_packets(scene_dir, name, camera):
    check_frame(case_partial(scene_dir, name, camera), camera, f"{name} {SIZES[camera]}")


@pytest.mark.gpu
def test_zero_component_inside_the_image(scene_dir):
    check_frame(case_zero_inside(scene_dir), 0, "zero column 8")


@pytest.mark.gpu
def test_zero_component_outside_the_image(scene_dir):
    check_frame(case_zero_outside(scene_dir), 1, "zero column 20")


@pytest.mark.gpu
@pytest.mark.parametrize("camera", [0, 1])
def test_all_sign_octants(scene_dir, camera):
    check_frame(case_octants(scene_dir), camera, f"octants camera {camera}")


@pytest.mark.gpu
def test_shadow_rays_leave_alive_mid_walk(scene_dir):
    check_frame(case_alive(scene_dir), 1, "soup 70x9 shadows")


@pytest.mark.gpu
def test_per_lane_closest_hit(scene_dir):
    import ceng795_amd
    xml = case_rays(scene_dir)
    o, d, rec, _, _ = query_rays(xml)
    hit = rec[:, 7] == 1.0
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        hits, _ = trace(s, o, d)
    got_hit = hits["leaf"] >= 0
    print(f"closest hit: {N_RAYS} rays, {int(hit.sum())} hit, "
          f"{int((got_hit != hit).sum())} differ in hit")
    assert np.array_equal(got_hit, hit)
    assert np.array_equal(bits(hits["t"][hit]), bits(rec[hit, 3]))
    assert np.array_equal(bits(hits["normal"][hit]), bits(rec[hit, 4:7]))
    assert (bits(hits["t"][~hit]) == bits(F(np.inf))).all()


@pytest.mark.gpu
def test_per_lane_occlusion(scene_dir):
    import ceng795_amd
    xml = case_rays(scene_dir)
    o, d, _, tmax, want = query_rays(xml)
    with ceng795_amd.Scene(xml, traversal="fast") as s:
        got, _ = occlusion(s, o, d, tmax)
    print(f"occlusion: {N_RAYS} rays, {int(want.sum())} occluded, "
          f"{int((got != want).sum())} differ")
    assert np.array_equal(got, want)
