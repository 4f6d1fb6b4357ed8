#!/usr/bin/env python3
"""Ray-query throughput on the C3 scene (not bench.py): camera 0's 1920x1080 primary rays put
to rt_trace_rays_device / rt_occluded_device in three orders — row-major, the frame kernel's
8x8-tile order, a seeded shuffle — each with and without RT_QUERY_REORDER.

Per case: device-event time of every call over --calls rounds after --warmup rounds, the
cases alternated within each round (one process), median and quartiles, Mrays/s from the
median.  For scale, the frame kernel's own time on the same scene in the same rounds
(rt_set_kernel_timing): it traces the same primary rays in tile order, plus shadow rays and
shading.  Writes profiles/ray_query.json, keyed to the sha256 of the library that ran.

--radiance: the same three orders put to rt_shade_rays_device instead (the radiance query does
the frame kernel's whole work for the caller's rays), every case checked bit for bit against the
tile-order result and the frame in the same run; writes profiles/radiance_query.json.

--radiance --lights: what the caller's own light records cost (rt_shade_rays_lit_device; DESIGN.md
§4.14).  Camera 0's rays in tile order through four cases — LIGHT_CASES below — of which the
first three do the same work through three paths; every case checked bit for bit against the
first; writes profiles/radiance_lights.json.  --dry-run (needs no GPU) writes the case list only.

--smooth (with or without --radiance): what smooth shading costs.  The C3 scene
twice, as it is and with its mesh smooth (shadingMode="smooth", Scene(..., smooth=True)), camera 0's rays in tile
order through SMOOTH_CASES — closest hits, radiance and rt_hit_attributes_device on both scenes,
alternated within every round; the flat scene's results checked against the frame, the smooth
scene's hits against the flat one's in everything but the normal; writes profiles/smooth_query.json.
--dry-run (needs no GPU) writes the case list only.

usage: ray_query_bench.py [--calls 50] [--warmup 3] [--n 708] [--out PATH] [--check] [--radiance]
                          [--lights] [--smooth] [--dry-run]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_scene  # noqa: E402


def file_sha256(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 20), b""):
            h.update(b)
    return h.hexdigest()


def primary_rays(cam):
    """o = e, d = normalize((top_left + (x + 0.5) s_u) - (y + 0.5) s_v - e) in fp32 (the
    camera's rays, Camera.h:30-35), row-major."""
    f = np.float32
    e, tl = np.array(cam.e, f), np.array(cam.top_left, f)
    su, sv = np.array(cam.s_u, f), np.array(cam.s_v, f)
    x = (np.arange(cam.width, dtype=f) + f(0.5))[None, :, None]
    y = (np.arange(cam.height, dtype=f) + f(0.5))[:, None, None]
    s = (tl + x * su) - y * sv
    d = s - e
    d = d / np.sqrt((d * d).sum(-1, dtype=f))[..., None]
    d = np.ascontiguousarray(d.reshape(-1, 3), f)
    return np.broadcast_to(e, d.shape), d


def orders(width: int, height: int, seed: int):
    n = width * height
    idx = np.arange(n, dtype=np.int64).reshape(height, width)
    th, tw = -(-height // 8), -(-width // 8)
    padded = np.full((th * 8, tw * 8), -1, np.int64)
    padded[:height, :width] = idx
    tiles = padded.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(-1)
    return {"row_major": idx.reshape(-1), "tile_8x8": tiles[tiles >= 0],
            "shuffled": np.random.default_rng(seed).permutation(n)}


def quartiles(ms):
    q = np.percentile(np.array(ms), [25, 50, 75])
    return {"ms_q1": float(q[0]), "ms_median": float(q[1]), "ms_q3": float(q[2])}


# --radiance --lights: name -> (what runs, light records per ray, shared, scene lights)
LIGHT_CASES = {
    "a_plain": ("rt_shade_rays_device: the scene's one light", 0, False, True),
    "b_shared": ("RT_QUERY_NO_SCENE_LIGHTS, the scene's light as one shared record", 1, True, False),
    "c_per_ray": ("RT_QUERY_NO_SCENE_LIGHTS, the scene's light as each ray's own record, k = 1",
                  1, False, False),
    "d_per_ray_k4": ("RT_QUERY_NO_SCENE_LIGHTS, k = 4 per-ray records of which one is active "
                     "(slot i % 4 of ray i), the rest NaN", 4, False, False),
}


# --smooth: name -> (scene, what runs)
SMOOTH_CASES = {
    "flat/closest": ("flat", "rt_trace_rays_device"),
    "smooth/closest": ("smooth", "rt_trace_rays_device"),
    "flat/radiance": ("flat", "rt_shade_rays_device"),
    "smooth/radiance": ("smooth", "rt_shade_rays_device"),
    "flat/attributes": ("flat", "rt_hit_attributes_device"),
    "smooth/attributes": ("smooth", "rt_hit_attributes_device"),
}


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--n", type=int, default=708, help="height-field grid (708: the C3 mesh)")
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--seed", type=int, default=795)
    p.add_argument("--out", default=None,
                   help="default: profiles/ray_query.json (profiles/radiance_query.json)")
    p.add_argument("--radiance", action="store_true",
                   help="radiance queries (rt_shade_rays_device) instead of hits and occlusion")
    p.add_argument("--lights", action="store_true",
                   help="with --radiance: the cost of caller light records (LIGHT_CASES)")
    p.add_argument("--smooth", action="store_true",
                   help="C3 flat against C3 with its mesh smooth (SMOOTH_CASES)")
    p.add_argument("--instances", type=int, default=0, metavar="K",
                   help="a generated mesh (--n grid) placed K times as instances against the same "
                        "geometry baked to world space in a flat scene: closest hit, occlusion and radiance")
    p.add_argument("--moving", action="store_true",
                   help="with --instances K: a third scene, the instances each with a velocity "
                        "(rt_scene_create_moving), traced with every ray at time 0 — the static "
                        "scene's geometry through the motion kernels' per-ray inverses")
    p.add_argument("--dry-run", action="store_true",
                   help="with --radiance --lights or --smooth: write the case list and stop (no GPU)")
    p.add_argument("--check", action="store_true",
                   help="also compare every case's results with the row-major ones, bit for bit")
    a = p.parse_args(argv)
    if a.lights and not a.radiance:
        p.error("--lights goes with --radiance")
    if a.lights and a.smooth:
        p.error("--lights and --smooth are separate runs")
    if a.moving and not a.instances:
        p.error("--moving goes with --instances K")
    if a.dry_run and not (a.lights or a.smooth or (a.instances and a.moving)):
        p.error("--dry-run goes with --radiance --lights, with --smooth or with --instances K --moving")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles",
                             "smooth_query.json" if a.smooth else
                             "radiance_lights.json" if a.lights else
                             "radiance_query.json" if a.radiance else "ray_query.json")
    if a.instances:
        if a.out.endswith("ray_query.json"):
            a.out = os.path.join(ROOT, "profiles", f"instances_k{a.instances}.json")
        return instances_main(a)
    if a.smooth:
        return smooth_main(a)
    if a.lights:
        return lights_main(a)
    if a.radiance:
        return radiance_main(a)

    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_bench: no GPU")

    with tempfile.TemporaryDirectory() as d:
        xml = os.path.join(d, "c3.xml")
        with open(xml, "w") as f:
            f.write(gen_scene.heightfield_scene(a.n, a.width, a.height, name="c3.png").to_xml())
        scene = ceng795_amd.Scene(xml, device=0)
    cam = scene.camera(0)
    o, dirs = primary_rays(cam)
    n = len(dirs)
    order = orders(cam.width, cam.height, a.seed)
    rays = {}
    for name, idx in order.items():
        r = ceng795_amd.pack_rays(o[idx], dirs[idx], np.inf)
        rays[name] = torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda()
    hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    frame = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    cases = [(kind, name, flag) for kind in ("closest", "occluded") for name in order
             for flag in (False, True)]

    def run(kind, name, flag):
        if kind == "closest":
            scene.trace_rays_device(rays[name].data_ptr(), n, hits.data_ptr(), reorder=flag,
                                    stream=stream)
        else:
            scene.occluded_device(rays[name].data_ptr(), n, occ.data_ptr(), reorder=flag,
                                  stream=stream)

    checks = {}
    if a.check:
        want = {}
        for kind, name, flag in cases:
            run(kind, name, flag)
            torch.cuda.synchronize()
            out = (hits if kind == "closest" else occ).cpu().numpy()
            out = out.reshape(n, -1)
            back = np.empty_like(out)
            back[order[name]] = out  # to row-major positions
            if (kind, "row_major", False) == (kind, name, flag):
                want[kind] = back
            checks[f"{kind}/{name}/{'reorder' if flag else 'plain'}"] = bool(
                np.array_equal(back, want[kind]))
        hit_share = float((want["closest"].view(np.int32)[:, 1] >= 0).mean())
    else:
        hit_share = None

    times = {c: [] for c in cases}
    scene.set_kernel_timing(False)
    for rnd in range(a.warmup + a.calls):
        timed = rnd >= a.warmup
        if rnd == a.warmup:
            torch.cuda.synchronize()
            scene.set_kernel_timing(True)
        marks = []
        for c in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(*c)
            e1.record()
            marks.append((c, e0, e1))
        scene.render_device(0, frame.data_ptr(), stream=stream)  # the frame kernel, same rounds
        torch.cuda.synchronize()
        if timed:
            for c, e0, e1 in marks:
                times[c].append(e0.elapsed_time(e1))
    kt, launches = scene.read_kernel_times()
    frame_ms = kt["frame"] / max(1, launches)

    result = {"lib_sha256": file_sha256(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
              "scene": f"C3: height field {a.n}, camera 0 {cam.width}x{cam.height}",
              "rays": n, "calls": a.calls, "warmup": a.warmup,
              "timing": "device events around each call; cases alternated within every round",
              "frame_kernel_ms": frame_ms, "frame_kernel_launches": launches,
              "frame_kernel_note": "rt_set_kernel_timing mean over the same rounds: primary + "
                                   "shadow rays + shading of the same pixels in tile order",
              "hit_share": hit_share, "cases": {}}
    for (kind, name, flag), ms in times.items():
        q = quartiles(ms)
        q["mrays_per_s"] = n / q["ms_median"] / 1e3
        result["cases"][f"{kind}/{name}/{'reorder' if flag else 'plain'}"] = q
    c = result["cases"]
    result["ratios"] = {
        "closest_tile_plain_over_frame_kernel": c["closest/tile_8x8/plain"]["ms_median"] / frame_ms,
        "closest_shuffled_reorder_over_plain":
            c["closest/shuffled/reorder"]["ms_median"] / c["closest/shuffled/plain"]["ms_median"],
        "closest_tile_reorder_over_plain":
            c["closest/tile_8x8/reorder"]["ms_median"] / c["closest/tile_8x8/plain"]["ms_median"],
        "occluded_shuffled_reorder_over_plain":
            c["occluded/shuffled/reorder"]["ms_median"] / c["occluded/shuffled/plain"]["ms_median"],
    }
    if a.check:
        result["bit_identical_to_row_major"] = checks
    scene.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0 if all(checks.values()) else 1


def radiance_main(a) -> int:
    """The radiance cases: orders x flag, alternated with a frame in every round."""
    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_bench: no GPU")

    with tempfile.TemporaryDirectory() as d:
        xml = os.path.join(d, "c3.xml")
        with open(xml, "w") as f:
            f.write(gen_scene.heightfield_scene(a.n, a.width, a.height, name="c3.png").to_xml())
        scene = ceng795_amd.Scene(xml, device=0)
    cam = scene.camera(0)
    o, dirs = primary_rays(cam)
    n = len(dirs)
    order = orders(cam.width, cam.height, a.seed)
    rays = {}
    for name, idx in order.items():
        r = ceng795_amd.pack_rays(o[idx], dirs[idx])
        rays[name] = torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda()
    rad = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    frame = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    cases = [(name, flag) for name in ("tile_8x8", "row_major", "shuffled")
             for flag in (False, True)]

    def run(name, flag):
        scene.shade_rays_device(rays[name].data_ptr(), n, rad.data_ptr(), reorder=flag,
                                stream=stream)

    # every case against the tile-order result, and that against the frame, bit for bit
    scene.render_device(0, frame.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    frame_rgb = frame.cpu().numpy().reshape(n, 3)
    checks, want = {}, None
    for name, flag in cases:
        rad.zero_()
        run(name, flag)
        torch.cuda.synchronize()
        out = rad.cpu().numpy().reshape(n, 16)
        back = np.empty_like(out)
        back[order[name]] = out  # to row-major positions
        if want is None:
            want = back
        checks[f"radiance/{name}/{'reorder' if flag else 'plain'}"] = bool(
            np.array_equal(back, want))
    got = want.view(ceng795_amd.RADIANCE_DTYPE).reshape(n)
    checks["tile_order_equals_frame"] = bool(
        np.array_equal(got["rgb"].view(np.uint32), frame_rgb.view(np.uint32)))
    hit_share = float(np.isfinite(got["t"]).mean())

    times = {c: [] for c in cases}
    scene.set_kernel_timing(False)
    for rnd in range(a.warmup + a.calls):
        timed = rnd >= a.warmup
        if rnd == a.warmup:
            torch.cuda.synchronize()
            scene.set_kernel_timing(True)
        marks = []
        for c in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(*c)
            e1.record()
            marks.append((c, e0, e1))
        scene.render_device(0, frame.data_ptr(), stream=stream)  # the frame kernel, same rounds
        torch.cuda.synchronize()
        if timed:
            for c, e0, e1 in marks:
                times[c].append(e0.elapsed_time(e1))
    kt, launches = scene.read_kernel_times()
    frame_ms = kt["frame"] / max(1, launches)

    result = {"lib_sha256": file_sha256(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
              "scene": f"C3: height field {a.n}, camera 0 {cam.width}x{cam.height}",
              "rays": n, "calls": a.calls, "warmup": a.warmup,
              "timing": "device events around each call; cases alternated within every round",
              "frame_kernel_ms": frame_ms, "frame_kernel_launches": launches,
              "frame_kernel_note": "rt_set_kernel_timing mean over the same rounds: the same rays "
                                   "in tile order, heavy-first dispatch, 12 B out per pixel",
              "hit_share": hit_share, "cases": {}}
    for (name, flag), ms in times.items():
        q = quartiles(ms)
        q["mrays_per_s"] = n / q["ms_median"] / 1e3
        result["cases"][f"radiance/{name}/{'reorder' if flag else 'plain'}"] = q
    c = result["cases"]
    result["ratios"] = {
        "tile_plain_over_frame_kernel": c["radiance/tile_8x8/plain"]["ms_median"] / frame_ms,
        "row_major_plain_over_tile_plain":
            c["radiance/row_major/plain"]["ms_median"] / c["radiance/tile_8x8/plain"]["ms_median"],
        "shuffled_reorder_over_plain":
            c["radiance/shuffled/reorder"]["ms_median"] / c["radiance/shuffled/plain"]["ms_median"],
        "tile_reorder_over_plain":
            c["radiance/tile_8x8/reorder"]["ms_median"] / c["radiance/tile_8x8/plain"]["ms_median"],
    }
    result["bit_identical_to_tile_order"] = checks
    scene.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0 if all(checks.values()) else 1


def instances_main(a) -> int:
    """--instances K: a height field of --n x --n vertices placed K times on a square grid, each
    copy scaled, turned about z and moved; the same rays (from a shell around the grid toward
    points on it, shuffled) through the instanced scene's two-level walk and through a flat scene
    of the same geometry baked to world space (fp32 vertices: its bits differ, its hits agree up
    to rounding).  Device bytes: what creating each scene took from the device's free memory."""
    k, g = a.instances, a.n
    names = ["instanced", "baked"] + (["moving"] if a.moving else [])
    cases = [(sc, kind, flag) for kind in ("closest", "occluded", "radiance")
             for flag in (False, True) for sc in names]
    if a.dry_run:  # the case list, on a machine without a GPU
        print(f"instances={k} grid={g} moving={int(a.moving)} rays={a.width * a.height}")
        for sc, kind, flag in cases:
            print(f"{sc}/{kind}/{'reorder' if flag else 'plain'}")
        return 0
    import ctypes as C
    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_bench: no GPU")
    f = np.float32
    rng = np.random.default_rng(a.seed)
    xs = np.linspace(-1, 1, g, dtype=f)
    vx, vy = np.meshgrid(xs, xs)
    base = np.stack([vx, vy, (0.15 * rng.random((g, g))).astype(f)], -1).reshape(-1, 3).astype(f)
    i, j = np.meshgrid(np.arange(g - 1), np.arange(g - 1))
    q = (j * g + i).reshape(-1)
    faces = np.stack([q, q + 1, q + g + 1, q, q + g + 1, q + g], 1).reshape(-1, 3).astype(np.int32)
    side = int(np.ceil(np.sqrt(k)))
    xf = np.zeros((k, 4, 4), f)
    for c in range(k):
        ang, sc = rng.uniform(0, 2 * np.pi), rng.uniform(0.7, 1.1)
        m = np.eye(4)
        m[:2, :2] = sc * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        m[2, 2] = rng.uniform(0.5, 2.0)
        m[:3, 3] = (2.4 * (c % side - (side - 1) / 2), 2.4 * (c // side - (side - 1) / 2), rng.uniform(-0.2, 0.2))
        xf[c] = m.astype(f)
    material = _lib.rt_material()
    material.ambient = (C.c_float * 3)(1.0, 1.0, 1.0)
    material.diffuse = (C.c_float * 3)(0.8, 0.6, 0.4)
    material.specular = (C.c_float * 3)(0.2, 0.2, 0.2)
    material.phong_exponent = 4.0
    material.refraction_index = 1.0
    light = _lib.rt_point_light((C.c_float * 3)(0.3 * side, 0.5 * side, 3.0 * side),
                                (C.c_float * 3)(*[200.0 * side * side] * 3))

    def desc_of(verts, counts, all_faces):
        d = _lib.rt_scene_desc()
        keep = [np.ascontiguousarray(verts, f), np.array(counts, np.int32),
                np.ascontiguousarray(all_faces, np.int32), np.zeros(len(counts), np.int32), material]
        d.vertices = keep[0].ctypes.data_as(C.POINTER(C.c_float))
        d.num_vertices = len(keep[0])
        d.materials, d.num_materials = C.pointer(material), 1
        d.lights, d.num_lights = C.pointer(light), 1
        d.ambient_light = (C.c_float * 3)(20.0, 20.0, 20.0)
        d.num_meshes = len(counts)
        d.mesh_material = keep[3].ctypes.data_as(C.POINTER(C.c_int))
        d.mesh_face_count = keep[1].ctypes.data_as(C.POINTER(C.c_int))
        d.mesh_faces = keep[2].ctypes.data_as(C.POINTER(C.c_int))
        d.shadow_ray_epsilon = 1e-3
        return d, keep

    def created(make):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        s = make()
        torch.cuda.synchronize()
        return s, int(free0 - torch.cuda.mem_get_info()[0])

    d_inst, keep1 = desc_of(base, [len(faces)], faces)
    # (a first scene, closed again: the runtime's own first allocations are not the scene's)
    created(lambda: ceng795_amd.Scene.create(d_inst, device=0))[0].close()
    inst, inst_bytes = created(lambda: ceng795_amd.Scene.create(
        d_inst, instance_mesh=np.zeros(k, np.int32), instance_material=np.zeros(k, np.int32),
        instance_transform=xf, device=0))
    world = np.concatenate([(base @ m[:3, :3].T + m[:3, 3]).astype(f) for m in xf])
    baked_faces = np.concatenate([faces + c * len(base) for c in range(k)])
    d_flat, keep2 = desc_of(world, [len(faces)] * k, baked_faces)
    flat, flat_bytes = created(lambda: ceng795_amd.Scene.create(d_flat, device=0))

    n = a.width * a.height
    half = 1.2 * side
    o = (rng.normal(size=(n, 3)) * (half, half, 0.3 * half) + (0, 0, 1.5 * half)).astype(f)
    target = (rng.uniform(-1, 1, size=(n, 3)) * (half, half, 0.1)).astype(f)
    packed = ceng795_amd.pack_rays(o, (target - o).astype(f), np.inf)
    rays = torch.from_numpy(packed.view(np.uint8).reshape(-1)).cuda()
    hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rad = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    scenes = {"instanced": inst, "baked": flat}
    moving_bytes = 0
    if a.moving:  # every instance with a velocity; the rays' times (pad) are 0
        vel = rng.uniform(0.2, 0.6, size=(k, 3)).astype(f)
        scenes["moving"], moving_bytes = created(lambda: ceng795_amd.Scene.create(
            d_inst, instance_mesh=np.zeros(k, np.int32), instance_material=np.zeros(k, np.int32),
            instance_transform=xf, instance_velocity=vel, device=0))
        assert scenes["moving"].has_motion

    def run(sc, kind, flag):
        kw = dict(reorder=flag, stream=stream, ray_time=sc == "moving")
        if kind == "closest":
            scenes[sc].trace_rays_device(rays.data_ptr(), n, hits.data_ptr(), **kw)
        elif kind == "radiance":  # one point light: a shadow ray per hit
            scenes[sc].shade_rays_device(rays.data_ptr(), n, rad.data_ptr(), **kw)
        else:
            scenes[sc].occluded_device(rays.data_ptr(), n, occ.data_ptr(), **kw)

    got = {}
    for sc in scenes:
        run(sc, "closest", False)
        torch.cuda.synchronize()
        got[sc] = hits.cpu().numpy().view(ceng795_amd.HIT_DTYPE).copy()
    if a.moving:  # at time 0 the moving scene's hits are the static scene's (the boxes are larger)
        same_t = got["moving"]["t"].view(np.uint32) == got["instanced"]["t"].view(np.uint32)
        same_object = got["moving"]["object"] == got["instanced"]["object"]
        moving_same = float((same_t & same_object).mean())
    hit_i, hit_b = got["instanced"]["object"] >= 0, got["baked"]["object"] >= 0
    both = hit_i & hit_b
    # the baked scene numbers instance c's faces from c * faces on
    same = ((got["instanced"]["object"][both] == got["baked"]["object"][both] % len(faces)) &
            (got["instanced"]["pad"][both] == got["baked"]["object"][both] // len(faces)))
    agree = {"hit_share_instanced": float(hit_i.mean()), "hit_share_baked": float(hit_b.mean()),
             "same_hit_or_miss": float((hit_i == hit_b).mean()),
             "same_face_and_instance_where_both_hit": float(same.mean()),
             "max_rel_t_diff_where_same_face": float(np.max(np.abs(
                 got["instanced"]["t"][both] / got["baked"]["t"][both] - 1)[same], initial=0.0))}

    times = {c: [] for c in cases}
    for rnd in range(a.warmup + a.calls):
        marks = []
        for c in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(*c)
            e1.record()
            marks.append((c, e0, e1))
        torch.cuda.synchronize()
        if rnd >= a.warmup:
            for c, e0, e1 in marks:
                times[c].append(e0.elapsed_time(e1))
    result = {"lib_sha256": file_sha256(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
              "scene": f"height field {g}x{g} ({len(faces)} faces) x {k} instances on a "
                       f"{side}x{side} grid; baked: {len(baked_faces)} world-space faces",
              "rays": n, "calls": a.calls, "warmup": a.warmup,
              "timing": "device events around each call; cases alternated within every round",
              "device_bytes": {"instanced": inst_bytes, "baked": flat_bytes},
              "agreement": agree, "cases": {}}
    if a.moving:
        result["device_bytes"]["moving"] = moving_bytes
        result["agreement"]["moving_equals_instanced_at_time_0"] = moving_same
    for (sc, kind, flag), ms in times.items():
        qq = quartiles(ms)
        qq["mrays_per_s"] = n / qq["ms_median"] / 1e3
        result["cases"][f"{sc}/{kind}/{'reorder' if flag else 'plain'}"] = qq
    c = result["cases"]
    result["ratios"] = {f"instanced_over_baked/{kind}/{fl}":
                        c[f"instanced/{kind}/{fl}"]["ms_median"] / c[f"baked/{kind}/{fl}"]["ms_median"]
                        for kind in ("closest", "occluded", "radiance") for fl in ("plain", "reorder")}
    if a.moving:
        result["ratios"].update({
            f"moving_over_instanced/{kind}/{fl}":
            c[f"moving/{kind}/{fl}"]["ms_median"] / c[f"instanced/{kind}/{fl}"]["ms_median"]
            for kind in ("closest", "occluded", "radiance") for fl in ("plain", "reorder")})
        scenes["moving"].close()
    inst.close()
    flat.close()
    write_result(a.out, result)
    return 0


def write_result(path: str, result: dict) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def lights_main(a) -> int:
    """LIGHT_CASES on camera 0's rays in tile order, alternated within every round."""
    spec = gen_scene.heightfield_scene(a.n, a.width, a.height, name="c3.png")
    assert len(spec.lights) == 1
    result = {"scene": f"C3: height field {a.n}, camera 0 {a.width}x{a.height}",
              "rays": a.width * a.height, "order": "tile_8x8", "calls": a.calls,
              "warmup": a.warmup,
              "timing": "device events around each call; cases alternated within every round",
              "case_list": {k: {"what": v[0], "records_per_ray": v[1], "shared": v[2],
                                "scene_lights": v[3],
                                "light_bytes": 48 * v[1] * (1 if v[2] else a.width * a.height)}
                            for k, v in LIGHT_CASES.items()}}
    if a.dry_run:
        result["dry_run"] = True
        write_result(a.out, result)
        return 0

    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_bench: no GPU")
    with tempfile.TemporaryDirectory() as d:
        xml = os.path.join(d, "c3.xml")
        with open(xml, "w") as f:
            f.write(spec.to_xml())
        scene = ceng795_amd.Scene(xml, device=0)
    cam = scene.camera(0)
    o, dirs = primary_rays(cam)
    n = len(dirs)
    idx = orders(cam.width, cam.height, a.seed)["tile_8x8"]
    r = ceng795_amd.pack_rays(o[idx], dirs[idx])
    rays = torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda()
    pos, inten = (np.array(v, np.float32) for v in spec.lights[0])
    lights = {}
    for name, (_, k, shared, _) in LIGHT_CASES.items():
        if k == 0:
            lights[name] = torch.zeros(48, dtype=torch.uint8, device="cuda")
            continue
        rec = np.zeros((1 if shared else n, k), ceng795_amd.LIGHT_SAMPLE_DTYPE)
        rec["position"] = np.nan
        slot = np.arange(len(rec)) % k
        rec["position"][np.arange(len(rec)), slot] = pos
        rec["intensity"][np.arange(len(rec)), slot] = inten
        lights[name] = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    rad = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(name):
        _, k, shared, scene_lights = LIGHT_CASES[name]
        if k == 0:
            scene.shade_rays_device(rays.data_ptr(), n, rad.data_ptr(), stream=stream)
        else:
            scene.shade_rays_lit_device(rays.data_ptr(), n, lights[name].data_ptr(), k,
                                        rad.data_ptr(), shared=shared, scene_lights=scene_lights,
                                        stream=stream)

    checks, want = {}, None
    for name in LIGHT_CASES:
        rad.zero_()
        run(name)
        torch.cuda.synchronize()
        out = rad.cpu().numpy().copy()
        if want is None:
            want = out
        checks[name] = bool(np.array_equal(out, want))
    times = {c: [] for c in LIGHT_CASES}
    for rnd in range(a.warmup + a.calls):
        marks = []
        for c in LIGHT_CASES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(c)
            e1.record()
            marks.append((c, e0, e1))
        torch.cuda.synchronize()
        if rnd >= a.warmup:
            for c, e0, e1 in marks:
                times[c].append(e0.elapsed_time(e1))
    result.update({"lib_sha256": file_sha256(_lib.LIB_PATH),
                   "device": torch.cuda.get_device_name(0), "cases": {}})
    for name, ms in times.items():
        q = quartiles(ms)
        q["mrays_per_s"] = n / q["ms_median"] / 1e3
        result["cases"][name] = q
    c = result["cases"]
    result["ratios"] = {f"{k}_over_a_plain": c[k]["ms_median"] / c["a_plain"]["ms_median"]
                        for k in LIGHT_CASES if k != "a_plain"}
    result["bit_identical_to_a_plain"] = checks
    scene.close()
    write_result(a.out, result)
    return 0 if all(checks.values()) else 1


def smooth_main(a) -> int:
    """SMOOTH_CASES on camera 0's rays in tile order, alternated within every round."""
    spec = gen_scene.heightfield_scene(a.n, a.width, a.height, name="c3.png")
    assert len(spec.meshes) == 1
    result = {"scene": f"C3: height field {a.n}, camera 0 {a.width}x{a.height}; smooth: the same "
                       "scene with its one mesh smooth",
              "rays": a.width * a.height, "order": "tile_8x8", "calls": a.calls,
              "warmup": a.warmup,
              "timing": "device events around each call; cases alternated within every round",
              "case_list": {k: {"scene": v[0], "entry": v[1]} for k, v in SMOOTH_CASES.items()}}
    if a.dry_run:
        result["dry_run"] = True
        write_result(a.out, result)
        return 0

    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_bench: no GPU")
    text = spec.to_xml()
    assert text.count('<Mesh id="1">') == 1
    with tempfile.TemporaryDirectory() as d:
        xml, xml_smooth = os.path.join(d, "c3.xml"), os.path.join(d, "c3_smooth.xml")
        with open(xml, "w") as f:
            f.write(text)
        with open(xml_smooth, "w") as f:
            f.write(text.replace('<Mesh id="1">', '<Mesh id="1" shadingMode="smooth">'))
        scenes = {"flat": ceng795_amd.Scene(xml, device=0),
                  "smooth": ceng795_amd.Scene(xml_smooth, device=0, smooth=True)}
    assert scenes["smooth"].has_smooth and not scenes["flat"].has_smooth
    cam = scenes["flat"].camera(0)
    o, dirs = primary_rays(cam)
    n = len(dirs)
    idx = orders(cam.width, cam.height, a.seed)["tile_8x8"]
    r = ceng795_amd.pack_rays(o[idx], dirs[idx])
    rays = torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda()
    hits = {k: torch.zeros(n * 32, dtype=torch.uint8, device="cuda") for k in scenes}
    rad = {k: torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for k in scenes}
    attr = {k: torch.zeros(n * 48, dtype=torch.uint8, device="cuda") for k in scenes}
    frame = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(name):
        which, entry = SMOOTH_CASES[name]
        s = scenes[which]
        if entry == "rt_trace_rays_device":
            s.trace_rays_device(rays.data_ptr(), n, hits[which].data_ptr(), stream=stream)
        elif entry == "rt_shade_rays_device":
            s.shade_rays_device(rays.data_ptr(), n, rad[which].data_ptr(), stream=stream)
        else:  # (the hits of the scene's own closest-hit case)
            s.hit_attributes_device(rays.data_ptr(), hits[which].data_ptr(), n,
                                    attr[which].data_ptr(), stream=stream)

    for name in SMOOTH_CASES:
        run(name)
    scenes["flat"].render_device(0, frame.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    H = {k: hits[k].cpu().numpy().view(ceng795_amd.HIT_DTYPE) for k in scenes}
    R = {k: rad[k].cpu().numpy().view(ceng795_amd.RADIANCE_DTYPE) for k in scenes}
    A = {k: attr[k].cpu().numpy().view(ceng795_amd.HIT_ATTR_DTYPE) for k in scenes}
    back = np.empty((n, 3), np.float32)
    back[idx] = R["flat"]["rgb"]
    hit = H["flat"]["leaf"] >= 0
    checks = {
        "flat_radiance_equals_frame": bool(np.array_equal(
            back.view(np.uint32), frame.cpu().numpy().reshape(n, 3).view(np.uint32))),
        "same_t_and_leaf": bool(np.array_equal(H["flat"]["t"].view(np.uint32),
                                               H["smooth"]["t"].view(np.uint32)) and
                                np.array_equal(H["flat"]["leaf"], H["smooth"]["leaf"])),
        "smooth_hit_normal_is_the_attribute": bool(np.array_equal(
            H["smooth"]["normal"].view(np.uint32), A["smooth"]["shading_normal"].view(np.uint32))),
        "flat_hit_normal_is_the_geometric_normal": bool(np.array_equal(
            H["flat"]["normal"].view(np.uint32), A["smooth"]["geometric_normal"].view(np.uint32))),
        "same_barycentrics": bool(np.array_equal(A["flat"][["beta", "gamma"]],
                                                 A["smooth"][["beta", "gamma"]])),
    }
    differing = float((np.abs(H["flat"]["normal"][hit] - H["smooth"]["normal"][hit]).max(axis=1)
                       > 1e-3).mean())
    times = {c: [] for c in SMOOTH_CASES}
    for rnd in range(a.warmup + a.calls):
        marks = []
        for c in SMOOTH_CASES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(c)
            e1.record()
            marks.append((c, e0, e1))
        torch.cuda.synchronize()
        if rnd >= a.warmup:
            for c, e0, e1 in marks:
                times[c].append(e0.elapsed_time(e1))
    result.update({"lib_sha256": file_sha256(_lib.LIB_PATH),
                   "device": torch.cuda.get_device_name(0), "hit_share": float(hit.mean()),
                   "hits_whose_normals_differ_by_1e-3": differing, "cases": {}})
    for name, ms in times.items():
        q = quartiles(ms)
        q["mrays_per_s"] = n / q["ms_median"] / 1e3
        result["cases"][name] = q
    c = result["cases"]
    result["ratios"] = {f"smooth_over_flat_{k}": c[f"smooth/{k}"]["ms_median"] /
                        c[f"flat/{k}"]["ms_median"] for k in ("closest", "radiance", "attributes")}
    result["checks"] = checks
    for s in scenes.values():
        s.close()
    write_result(a.out, result)
    return 0 if all(checks.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
