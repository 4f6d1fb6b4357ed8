#!/usr/bin/env python3
"""Film timings on the C3 scene (not bench.py), camera 0 set to NumSamples 4.

Frame routes, the same samples both ways, outputs compared bit for bit in the same run:
  A  rt_render_device of the MSAA frame (the existing route: sample passes + msaa_resolve_kernel)
  B  rt_film_shade_rays_device of the reference's samples (rebuilt on the host, uploaded untimed)
     + rt_film_resolve_device
Splat alone (the colours of B's rays kept on the device), with the per-stage events of
rt_film_set_stage_timing (bin / scan / scatter / order / gather): the batch in pixel order, and
shuffled across pixels (stable within each pixel, so the film must not change).
Random positions: 1, 4 and 16 uniformly random samples per pixel.

One process; per round every case once, alternated; device events; median and quartiles over
--calls rounds after --warmup.  Writes profiles/film.json, keyed to the sha256 of the library.

usage: film_bench.py [--calls 20] [--warmup 3] [--n 708] [--width 1920] [--height 1080] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_scene  # noqa: E402
from ray_query_bench import file_sha256, quartiles  # noqa: E402

f32, f64, u64 = np.float32, np.float64, np.uint64
MINSTD_M = u64(2147483647)


def msaa_draws(seed: int, pixels: int, count: int) -> np.ndarray:
    """(pixels, count) draws of uniform_real_distribution<float>(0, 1) over the per-pixel
    minstd_rand0 generators of rt_set_msaa_seed(seed) (splitmix64 of (seed, pixel))."""
    with np.errstate(over="ignore"):
        z = u64(seed) + u64(0x9E3779B97F4A7C15) * (np.arange(pixels, dtype=u64) + u64(1))
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        z = z ^ (z >> u64(31))
    x = z % MINSTD_M
    x[x == 0] = 1
    out = np.empty((pixels, count), f32)
    for k in range(count):
        x = (x * u64(16807)) % MINSTD_M
        r = (x - u64(1)).astype(f32) / f32(2147483646.0)
        out[:, k] = np.minimum(r, np.nextafter(f32(1), f32(0)))
    return out


def msaa_samples(cam, seed: int):
    """The camera's MSAA samples (HW2/Scene.cpp:32-50), pixel-major: rt_ray records and xy."""
    import ceng795_amd
    w, h, n = cam.width, cam.height, cam.num_samples
    S = n * n
    draws = msaa_draws(seed, w * h, 2 * S)
    k = np.arange(S)
    smx = ((k // n).astype(f32)[None, :] + draws[:, 0::2]) / f32(n)
    smy = ((k % n).astype(f32)[None, :] + draws[:, 1::2]) / f32(n)
    p = np.arange(w * h)
    x = ((p % w).astype(f32)[:, None] + smx).reshape(-1)
    y = ((p // w).astype(f32)[:, None] + smy).reshape(-1)
    fx = ((x.astype(f64) - 0.5).astype(f32).astype(f64) + 0.5).astype(f32)
    fy = ((y.astype(f64) - 0.5).astype(f32).astype(f64) + 0.5).astype(f32)
    e, tl = np.array(cam.e, f32), np.array(cam.top_left, f32)
    su, sv = np.array(cam.s_u, f32), np.array(cam.s_v, f32)
    s = (tl[None, :] + su[None, :] * fx[:, None]) - sv[None, :] * fy[:, None]
    v = s - e[None, :]
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    d = v / ln[:, None]
    rays = ceng795_amd.pack_rays(np.broadcast_to(e, d.shape), d)
    return rays, np.ascontiguousarray(np.stack([x, y], 1), f32)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--n", type=int, default=708, help="height-field grid (708: the C3 mesh)")
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--seed", type=int, default=795)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "film.json"))
    a = p.parse_args(argv)

    import torch
    import ceng795_amd
    from ceng795_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("film_bench: no GPU")

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()

    with tempfile.TemporaryDirectory() as d:
        xml = os.path.join(d, "c3_msaa.xml")
        spec = gen_scene.heightfield_scene(a.n, a.width, a.height, name="c3.png")
        spec.cameras[0].num_samples = 4
        with open(xml, "w") as f:
            f.write(spec.to_xml())
        scene = ceng795_amd.Scene(xml, device=0)
    scene.set_msaa_seed(a.seed)
    cam = scene.camera(0)
    w, h = cam.width, cam.height
    rays, xy = msaa_samples(cam, a.seed)
    n = len(xy)
    rng = np.random.default_rng(a.seed)
    # shuffled across pixels, stable within each pixel (so the film is the same)
    pix = np.floor(xy[:, 1]).astype(np.int64) * w + np.floor(xy[:, 0]).astype(np.int64)
    perm = rng.permutation(n)
    shuffled = np.empty(n, np.int64)
    shuffled[np.argsort(pix[perm], kind="stable")] = np.argsort(pix, kind="stable")

    d_rays, d_xy = dev(rays), dev(xy)
    d_rad = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    frame_a = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    frame_b = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    film = ceng795_amd.Film(scene, w, h)
    side = ceng795_amd.Film(scene, w, h)  # the splat-alone cases

    # the checks: B's frame is A's, and the shuffled batch leaves the ordered batch's film
    scene.render_device(0, frame_a.data_ptr(), stream=stream)
    film.shade_rays_device(d_rays.data_ptr(), d_xy.data_ptr(), n, stream=stream)
    film.resolve_device(frame_b.data_ptr(), stream=stream)
    scene.shade_rays_device(d_rays.data_ptr(), n, d_rad.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    # x = (float)i + sample_x rounds up to i + 1 for sample_x within half an ulp of i below 1 (at
    # i ~ 1000 about 3 samples in 10^5): such a sample's source pixel is the next one by the
    # film's rule (or none, at the right and bottom edges) while the MSAA frame keeps it with pixel
    # i, so the two frames are compared away from those samples' neighbourhoods
    own = np.repeat(np.arange(w * h), n // (w * h))
    valid = (xy[:, 0] < f32(w)) & (xy[:, 1] < f32(h))
    moved = ~valid | (pix != own)
    near = np.zeros((h, w), bool)
    for dj in range(-2, 3):
        for di in range(-2, 3):
            jj = np.clip(own[moved] // w + dj, 0, h - 1)
            ii = np.clip(own[moved] % w + di, 0, w - 1)
            near[jj, ii] = True
    fa = frame_a.cpu().numpy().reshape(h, w, 3).view(np.uint32)
    fb = frame_b.cpu().numpy().reshape(h, w, 3).view(np.uint32)
    differ = (fa != fb).any(-1)
    checks = {"film_frame_equals_msaa_frame_away_from_moved_samples": not bool(differ[~near].any()),
              "counts": list(film.counts()) == [int(valid.sum()), int((~valid).sum())]}
    moved_info = {"samples_in_another_source_pixel": int(moved.sum()),
                  "samples_outside_the_film": int((~valid).sum()),
                  "pixels_near_them": int(near.sum()), "pixels_differing": int(differ.sum())}
    rad = d_rad.cpu().numpy().view(ceng795_amd.RADIANCE_DTYPE)
    batches = {"pixel_order": (d_xy, d_rad, n),
               "shuffled": (dev(xy[shuffled]), dev(rad[shuffled]), n)}
    for spp in (1, 4, 16):
        m = w * h * spp
        rxy = (rng.random((m, 2), dtype=f32) * np.array([w, h], f32)).astype(f32)
        np.minimum(rxy, np.nextafter(np.array([w, h], f32), f32(0)), out=rxy)
        rrad = np.zeros(m, ceng795_amd.RADIANCE_DTYPE)
        rrad["rgb"] = rng.random((m, 3), dtype=f32) * f32(255)
        batches[f"random_{spp}spp"] = (dev(rxy), dev(rrad), m)
    torch.cuda.synchronize()
    films = {}
    for name in ("pixel_order", "shuffled"):
        side.clear_device(stream=stream)
        bx, br, m = batches[name]
        side.splat_device(bx.data_ptr(), br.data_ptr(), m, stream=stream)
        films[name] = side.accumulators()
    checks["shuffled_film_equals_ordered_film"] = bool(
        np.array_equal(films["pixel_order"].view(np.uint32), films["shuffled"].view(np.uint32)))
    checks["splat_film_equals_fused_film"] = bool(
        np.array_equal(films["pixel_order"].view(np.uint32), film.accumulators().view(np.uint32)))

    cases = ["A_msaa_render", "B_film_shade_resolve"] + [f"splat/{b}" for b in batches]
    times = {c: [] for c in cases}
    stages = {b: [] for b in batches}
    side.set_stage_timing(True)

    def run(case):
        if case == "A_msaa_render":
            scene.render_device(0, frame_a.data_ptr(), stream=stream)
        elif case == "B_film_shade_resolve":
            film.clear_device(stream=stream)
            film.shade_rays_device(d_rays.data_ptr(), d_xy.data_ptr(), n, stream=stream)
            film.resolve_device(frame_b.data_ptr(), stream=stream)
        else:
            bx, br, m = batches[case.split("/", 1)[1]]
            side.splat_device(bx.data_ptr(), br.data_ptr(), m, stream=stream)

    for rnd in range(a.warmup + a.calls):
        for c in cases:
            if c.startswith("splat/"):
                side.clear_device(stream=stream)  # (outside the timed span)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(c)
            e1.record()
            torch.cuda.synchronize()
            if rnd >= a.warmup:
                times[c].append(e0.elapsed_time(e1))
                if c.startswith("splat/"):
                    stages[c.split("/", 1)[1]].append(side.stage_times())

    result = {"lib_sha256": file_sha256(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
              "scene": f"C3: height field {a.n}, camera 0 {w}x{h}, NumSamples 4",
              "samples": n, "calls": a.calls, "warmup": a.warmup,
              "timing": "device events around each case; cases alternated within every round; "
                        "stages: the events of rt_film_set_stage_timing",
              "checks": checks, "rounded_up_samples": moved_info, "cases": {},
              "stages_ms_median": {}}
    for c, ms in times.items():
        q = quartiles(ms)
        if c.startswith("splat/"):
            q["samples"] = batches[c.split("/", 1)[1]][2]
            q["msamples_per_s"] = q["samples"] / q["ms_median"] / 1e3
        result["cases"][c] = q
    for b, rows in stages.items():
        result["stages_ms_median"][b] = {k: float(np.median([r[k] for r in rows]))
                                         for k in rows[0]}
    result["ratios"] = {"B_over_A": result["cases"]["B_film_shade_resolve"]["ms_median"] /
                        result["cases"]["A_msaa_render"]["ms_median"]}
    film.close()
    side.close()
    scene.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0 if all(checks.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
