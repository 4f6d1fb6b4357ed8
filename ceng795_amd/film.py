"""Film: filtered accumulation of the caller's own samples (rt_film_*, include/ceng795_rt.h)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, lib
from .scene import RADIANCE_DTYPE, Scene, _aligned, pack_lights, pack_rays

FILTERS = {"gaussian": _lib.RT_FILM_GAUSSIAN, "box": _lib.RT_FILM_BOX}
STAGES = ("bin", "scan", "scatter", "order", "gather")


def _positions(xy, n: Optional[int] = None) -> np.ndarray:
    """(n, 2) film positions as a 16-byte aligned C-contiguous float32 array."""
    a = np.asarray(xy, np.float32)
    if a.ndim != 2 or a.shape[1] != 2 or (n is not None and len(a) != n):
        raise ValueError("xy must be an (n, 2) array, one position per sample")
    out = _aligned(len(a) * 2, np.float32).reshape(len(a), 2)
    out[...] = a
    return out


class Film:
    """``width x height`` Pixels (colour, weight) on the scene's GPU: the second half of the
    reference's MSAA branch (HW2/Scene.cpp:51-63) for samples the caller chose.

    A sample is a film position ``(x, y)`` in pixel units (pixel (i, j) covers
    ``[i, i+1) x [j, j+1)``) and an rgb.  ``filter="gaussian"`` splats it over the 3x3
    neighbourhood of its pixel with the reference's Gaussian (``sigma`` None: 1/3);
    ``filter="box"`` adds it to its own pixel with weight 1.  After a call the film holds what
    one thread would leave that took the call's valid samples sorted by (source row, source
    column, index in the batch); samples outside the film, and in ``shade_rays`` those of
    invalid rays, are dropped and counted.  ``resolve()`` is ``color / weight``.

    Close films before their scene.
    """

    def __init__(self, scene: Scene, width: int, height: int, filter: str = "gaussian",
                 sigma: Optional[float] = None):
        if filter not in FILTERS:
            raise ValueError(f"filter must be one of {sorted(FILTERS)}")
        h = C.c_void_p()
        check(lib().rt_film_create(scene.handle, int(width), int(height), FILTERS[filter],
                                   0.0 if sigma is None else float(sigma), C.byref(h)))
        self._h = h
        self._scene = scene  # the film needs its scene alive
        self.width, self.height, self.filter = int(width), int(height), filter

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            lib().rt_film_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # ------------------------------------------------------------------ host entries
    def clear(self) -> None:
        check(lib().rt_film_clear(self._h))

    def splat(self, xy, rgb) -> None:
        """Adds samples: ``xy`` (n, 2) positions, ``rgb`` (n, 3) colours or a RADIANCE_DTYPE
        array (what ``Scene.shade_rays`` returns; ``t`` is ignored)."""
        rgb = np.asarray(rgb)
        if rgb.dtype == RADIANCE_DTYPE:
            src = rgb["rgb"]
        else:
            src = np.asarray(rgb, np.float32)
        if src.ndim != 2 or src.shape[1] != 3:
            raise ValueError("rgb must be an (n, 3) array or a RADIANCE_DTYPE array")
        pos = _positions(xy, len(src))
        rad = _aligned(len(src), RADIANCE_DTYPE)
        rad["rgb"] = src
        check(lib().rt_film_splat(self._h, pos.ctypes.data, rad.ctypes.data, len(src)))

    def shade_rays(self, origins, directions, xy, *, depth: Optional[int] = None,
                   in_medium: bool = False, reorder: bool = False, stats: bool = False,
                   time=None):
        """``Scene.shade_rays`` of the rays, splatted at ``xy`` without leaving the GPU.  With
        ``stats`` returns the call's rt_stats.  ``time``: the rays' times (motion blur: one
        sample per ray, each at its own time)."""
        rays = pack_rays(origins, directions, time=time)
        pos = _positions(xy, len(rays))
        st = _lib.rt_stats()
        check(lib().rt_film_shade_rays(self._h, rays.ctypes.data, pos.ctypes.data, len(rays),
                                       -1 if depth is None else int(depth),
                                       Scene._radiance_flags(in_medium, reorder, time is not None),
                                       C.byref(st)))
        return st if stats else None

    def shade_rays_lit(self, origins, directions, xy, lights, *, shared: bool = False,
                       scene_lights: bool = True, depth: Optional[int] = None,
                       in_medium: bool = False, reorder: bool = False, stats: bool = False,
                       time=None):
        """``Scene.shade_rays_lit`` of the rays (``lights``: (n, k) LIGHT_SAMPLE_DTYPE records,
        or (k,) with ``shared``), splatted at ``xy`` without leaving the GPU."""
        rays = pack_rays(origins, directions, time=time)
        pos = _positions(xy, len(rays))
        lit, k = pack_lights(lights, len(rays), shared)
        st = _lib.rt_stats()
        check(lib().rt_film_shade_rays_lit(
            self._h, rays.ctypes.data, pos.ctypes.data, len(rays),
            -1 if depth is None else int(depth), lit.ctypes.data, k,
            Scene._lit_flags(in_medium, reorder, shared, scene_lights, time is not None),
            C.byref(st)))
        return st if stats else None

    def resolve(self) -> np.ndarray:
        """The frame: (height, width, 3) float32, ``color / weight``; 0 where no sample reached."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        check(lib().rt_film_resolve(self._h, out.ctypes.data))
        return out

    def accumulators(self) -> np.ndarray:
        """The raw Pixels: (height, width, 4) float32 {r, g, b, weight} (waits for the GPU)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        check(lib().rt_film_read(self._h, out.ctypes.data))
        return out

    def counts(self):
        """(samples added, samples dropped) since creation or the last clear (waits)."""
        c = (C.c_longlong * 2)()
        check(lib().rt_film_counts(self._h, c))
        return int(c[0]), int(c[1])

    # ------------------------------------------------------------------ device entries
    def clear_device(self, *, stream: int = 0) -> None:
        check(lib().rt_film_clear_device(self._h, C.c_void_p(stream)))

    def splat_device(self, xy_ptr: int, rad_ptr: int, n: int, *, stream: int = 0) -> None:
        """rt_film_splat_device: n x 2 floats at ``xy_ptr`` and n rt_radiance records at
        ``rad_ptr`` in device memory, asynchronously on HIP stream ``stream``."""
        check(lib().rt_film_splat_device(self._h, C.c_void_p(xy_ptr), C.c_void_p(rad_ptr), n,
                                         C.c_void_p(stream)))

    def shade_rays_device(self, rays_ptr: int, xy_ptr: int, n: int, *,
                          depth: Optional[int] = None, in_medium: bool = False,
                          reorder: bool = False, stream: int = 0, ray_time: bool = False) -> None:
        """rt_film_shade_rays_device: n rt_ray records and their n x 2 positions in device
        memory; the ray counts go to the scene's collect_stats()."""
        check(lib().rt_film_shade_rays_device(self._h, C.c_void_p(rays_ptr), C.c_void_p(xy_ptr), n,
                                              -1 if depth is None else int(depth),
                                              Scene._radiance_flags(in_medium, reorder, ray_time),
                                              C.c_void_p(stream)))

    def shade_rays_lit_device(self, rays_ptr: int, xy_ptr: int, n: int, lights_ptr: int, k: int, *,
                              shared: bool = False, scene_lights: bool = True,
                              depth: Optional[int] = None, in_medium: bool = False,
                              reorder: bool = False, stream: int = 0,
                              ray_time: bool = False) -> None:
        """rt_film_shade_rays_lit_device: as shade_rays_device, with the rays' n x k (shared: k)
        rt_light_sample records in device memory at ``lights_ptr``."""
        check(lib().rt_film_shade_rays_lit_device(
            self._h, C.c_void_p(rays_ptr), C.c_void_p(xy_ptr), n,
            -1 if depth is None else int(depth), C.c_void_p(lights_ptr), int(k),
            Scene._lit_flags(in_medium, reorder, shared, scene_lights, ray_time),
            C.c_void_p(stream)))

    def resolve_device(self, out_ptr: int, *, stream: int = 0) -> None:
        """rt_film_resolve_device: width*height*3 floats at ``out_ptr``."""
        check(lib().rt_film_resolve_device(self._h, C.c_void_p(out_ptr), C.c_void_p(stream)))

    # ------------------------------------------------------------------ measurement
    def set_stage_timing(self, enable: bool) -> None:
        check(lib().rt_film_set_stage_timing(self._h, int(enable)))

    def stage_times(self) -> dict:
        """HIP-event ms of the last timed splat's stages (waits for it)."""
        ms = (C.c_double * 5)()
        check(lib().rt_film_stage_times(self._h, ms))
        return dict(zip(STAGES, list(ms)))
