"""Helpers of the film tests: the contract of rt_film_* restated as a plain loop, and the
reference's MSAA samples rebuilt from the oracle's generator.

The restatement is the checker: numpy fp32 scalars (one rounding per operation), math.exp for
the reference's double exp, a double division by 2 pi sigma, narrowed.  test_film_host.py pins it
(with the sample reconstruction and OracleScene.shade_rays) to OracleScene.render_msaa bit for
bit, on the CPU."""
from __future__ import annotations

import math

import numpy as np

import desc_xml

f32 = np.float32
f64 = np.float64


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- the contract
def valid_mask(xy, width: int, height: int) -> np.ndarray:
    """0 <= x < width and 0 <= y < height as fp32 comparisons (NaN fails; -0.0 passes)."""
    xy = np.asarray(xy, f32)
    with np.errstate(invalid="ignore"):
        return ((xy[:, 0] >= f32(0)) & (xy[:, 0] < f32(width)) &
                (xy[:, 1] >= f32(0)) & (xy[:, 1] < f32(height)))


def source_pixels(xy, width: int) -> np.ndarray:
    """Row-major index of (floor x, floor y) of VALID positions."""
    xy = np.asarray(xy, f32)
    return np.floor(xy[:, 1]).astype(np.int64) * width + np.floor(xy[:, 0]).astype(np.int64)


def gaussian_filter(dx, dy, sigma) -> np.float32:
    """HW2/Scene.cpp:12-14 with fp32 arguments."""
    arg = -(dx * dx + dy * dy) / (f32(2) * sigma * sigma)
    return f32(math.exp(float(arg)) / (2 * math.pi * float(sigma)))


def splat(acc: np.ndarray, xy, rgb, filter: str = "gaussian", sigma=None, valid=None):
    """One splat call restated: `acc` (h, w, 4) float32 {r, g, b, weight}, updated in place by the
    call's valid samples taken in (source row, source column, batch index) order.  `valid`: the
    caller's own mask instead of valid_mask.  Returns (added, dropped)."""
    h, w = acc.shape[:2]
    xy = np.asarray(xy, f32)
    rgb = np.asarray(rgb, f32)
    ok = valid_mask(xy, w, h) if valid is None else np.asarray(valid, bool)
    idx = np.nonzero(ok)[0]
    src = source_pixels(xy[idx], w)
    order = idx[np.argsort(src, kind="stable")]
    sigma = f32(1.0) / f32(3.0) if sigma is None else f32(sigma)
    half = f32(0.5)
    for k in order:
        x, y = xy[k]
        r, g, b = rgb[k]
        i, j = int(math.floor(x)), int(math.floor(y))
        if filter == "box":
            p = acc[j, i]
            one = f32(1)
            p[0] = p[0] + r * one
            p[1] = p[1] + g * one
            p[2] = p[2] + b * one
            p[3] = p[3] + one
            continue
        for aj in range(j - 1, j + 2):
            if aj < 0 or aj >= h:
                continue
            dy = y - (f32(aj) + half)
            for ai in range(i - 1, i + 2):
                if ai < 0 or ai >= w:
                    continue
                wt = gaussian_filter(x - (f32(ai) + half), dy, sigma)
                p = acc[aj, ai]
                p[0] = p[0] + r * wt
                p[1] = p[1] + g * wt
                p[2] = p[2] + b * wt
                p[3] = p[3] + wt
    return len(idx), len(xy) - len(idx)


def new_film(width: int, height: int) -> np.ndarray:
    return np.zeros((height, width, 4), f32)


def resolve(acc: np.ndarray) -> np.ndarray:
    """Pixel::get_color: color / weight, 0 0 0 where weight == 0."""
    out = np.zeros(acc.shape[:2] + (3,), f32)
    hit = acc[..., 3] != 0
    with np.errstate(all="ignore"):
        out[hit] = acc[hit][:, :3] / acc[hit][:, 3:4]
    return out


# ---------------------------------------------------------------- cameras and MSAA samples
def camera(xml: str, cam: int = 0):
    """(e, top_left, s_u, s_v, width, height, n) of camera `cam`, vectors as float32 — the
    library's host-side precompute (rt_camera_from_view; tests/test_host.py pins it to the
    reference's)."""
    c = desc_xml.Desc(xml).cams[cam]
    v = lambda a: np.array(list(a), f32)  # noqa: E731
    return v(c.e), v(c.top_left), v(c.s_u), v(c.s_v), c.width, c.height, c.num_samples


def rays_through(cam, fx: np.ndarray, fy: np.ndarray):
    """Camera::calculate_ray_at for float32 plane coordinates fx, fy (already + 0.5): origins
    and normalised directions, one fp32 rounding per operation."""
    e, tl, su, sv = cam[:4]
    s = (tl[None, :] + su[None, :] * fx[:, None]) - sv[None, :] * fy[:, None]
    v = s - e[None, :]
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    d = v / ln[:, None]
    return np.broadcast_to(e, d.shape).copy(), np.ascontiguousarray(d, f32)


def pixel_centre_samples(cam):
    """One ray per pixel through its centre, row-major: (origins, directions, xy = (i + 0.5, j + 0.5))."""
    w, h = cam[4], cam[5]
    i = np.tile(np.arange(w, dtype=f32), h)
    j = np.repeat(np.arange(h, dtype=f32), w)
    fx = (i.astype(f64) + 0.5).astype(f32)
    fy = (j.astype(f64) + 0.5).astype(f32)
    o, d = rays_through(cam, fx, fy)
    return o, d, np.stack([fx, fy], axis=1)


def msaa_samples(xml: str, cam_index: int, seed: int):
    """Every MSAA sample of the camera as the reference draws them (HW2/Scene.cpp:32-50), pixel-major
    and within a pixel k = x * n + y: (origins, directions, xy, (width, height, samples per pixel)),
    xy = (i + sample_x, j + sample_y)."""
    from oracle import cpu_ref
    cam = camera(xml, cam_index)
    w, h, n = cam[4], cam[5], cam[6]
    S = n * n
    L = cpu_ref.lib()
    draws = np.stack([cpu_ref.minstd_uniform(L.cpuref_msaa_seed(seed, p), 2 * S)
                      for p in range(w * h)])              # (pixels, 2S)
    k = np.arange(S)
    ex, ey = draws[:, 0::2], draws[:, 1::2]
    smx = (f32(1) * (k // n).astype(f32)[None, :] + ex) / f32(n)
    smy = (f32(1) * (k % n).astype(f32)[None, :] + ey) / f32(n)
    i = (np.arange(w * h) % w).astype(f32)[:, None]
    j = (np.arange(w * h) // w).astype(f32)[:, None]
    x = (i + smx).astype(f32).reshape(-1)
    y = (j + smy).astype(f32).reshape(-1)
    # (float)((double)(i + smx) - 0.5), then calculate_ray_at's (float)((double)x + 0.5)
    fx = ((x.astype(f64) - 0.5).astype(f32).astype(f64) + 0.5).astype(f32)
    fy = ((y.astype(f64) - 0.5).astype(f32).astype(f64) + 0.5).astype(f32)
    o, d = rays_through(cam, fx, fy)
    return o, d, np.stack([x, y], axis=1), (w, h, S)
