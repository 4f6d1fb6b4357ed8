"""Scene: the reference's Scene interface (HW2/Scene.h) over the C ABI."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, lib

# rt_render_device tile_major flags (include/ceng795_rt.h)
RT_TILE_MAJOR, RT_TILE_BLOCKS, RT_TILE_RECORDS = 1, 2, 4
RT_UNTILE_BLOCKS, RT_UNTILE_SKIP_ROOT = 1, 2  # rt_untile_device flags

# rt_ray / rt_ray_hit (include/ceng795_rt.h), 32 bytes each
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("tmax", np.float32), ("d", np.float32, 3),
                      ("pad", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("object", np.int32), ("material", np.int32),
                      ("leaf", np.int32), ("normal", np.float32, 3), ("pad", np.int32)])
# rt_hit_attr, 48 bytes; flags: RT_ATTR_HIT 1, RT_ATTR_TRIANGLE 2, RT_ATTR_SMOOTH 4
HIT_ATTR_DTYPE = np.dtype([("beta", np.float32), ("gamma", np.float32), ("uv", np.float32, 2),
                           ("shading_normal", np.float32, 3), ("flags", np.int32),
                           ("geometric_normal", np.float32, 3), ("pad", np.int32)])
# rt_tex_query, 16 bytes
TEX_QUERY_DTYPE = np.dtype([("texture", np.int32), ("u", np.float32), ("v", np.float32),
                            ("pad", np.int32)])
# rt_radiance, 16 bytes
RADIANCE_DTYPE = np.dtype([("rgb", np.float32, 3), ("t", np.float32)])
# rt_light_sample, 48 bytes: a non-finite position = no light; normal 0 0 0 = a point light
LIGHT_SAMPLE_DTYPE = np.dtype([("position", np.float32, 3), ("pad0", np.float32),
                               ("intensity", np.float32, 3), ("pad1", np.float32),
                               ("normal", np.float32, 3), ("pad2", np.float32)])


def _aligned(n: int, dtype) -> np.ndarray:
    """n zeroed records of `dtype` at a 16-byte aligned address (the queries' pointer rule)."""
    dtype = np.dtype(dtype)
    raw = np.zeros(n * dtype.itemsize + 16, np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + n * dtype.itemsize].view(dtype)


def pack_rays(origins, directions, tmax=None, time=None) -> np.ndarray:
    """(n, 3) origins and directions (and per-ray tmax; ``time``: the rays' times, in ``pad``, read
    by calls with RT_QUERY_RAY_TIME) as a 16-byte aligned RAY_DTYPE array."""
    o = np.asarray(origins, np.float32)
    d = np.asarray(directions, np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
        raise ValueError("origins and directions must both be (n, 3) arrays")
    rays = _aligned(len(o), RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    if tmax is not None:
        rays["tmax"] = np.broadcast_to(np.asarray(tmax, np.float32), (len(o),))
    if time is not None:
        rays["pad"] = np.broadcast_to(np.asarray(time, np.float32), (len(o),))
    return rays


def _time_flag(time) -> int:
    return _lib.RT_QUERY_RAY_TIME if time is not None else 0


def texture_desc(textures, mesh_texture=None, triangle_texture=None, sphere_texture=None, counts=None):
    """An ``rt_texture_desc`` for ``textures``, a list of dicts ``rgb8`` ((h, w, 3) uint8),
    ``interpolation``, ``decal``, ``appearance`` (RT_TEX_* values; defaults bilinear, blend_kd,
    clamp: the reference's) and ``normalizer`` (255), and the three per-object id lists (None:
    no object of that kind has a texture).  ``counts``: the description's (meshes, triangles,
    spheres), checked against the lists.  Returns (desc, the arrays it points into)."""
    keep = []
    recs = (_lib.rt_texture * max(1, len(textures)))()
    for k, t in enumerate(textures):
        px = np.ascontiguousarray(t["rgb8"], np.uint8)
        if px.ndim != 3 or px.shape[2] != 3:
            raise ValueError("rgb8 must be an (h, w, 3) uint8 array")
        keep.append(px)
        recs[k].rgb8 = px.ctypes.data_as(C.POINTER(C.c_ubyte))
        recs[k].height, recs[k].width = int(px.shape[0]), int(px.shape[1])
        recs[k].interpolation = int(t.get("interpolation", _lib.RT_TEX_BILINEAR))
        recs[k].decal = int(t.get("decal", _lib.RT_TEX_BLEND_KD))
        recs[k].appearance = int(t.get("appearance", _lib.RT_TEX_CLAMP))
        recs[k].normalizer = float(t.get("normalizer", 255.0))
    keep.append(recs)
    d = _lib.rt_texture_desc()
    d.struct_size = C.sizeof(_lib.rt_texture_desc)
    d.num_textures = len(textures)
    d.textures = recs
    for i, (name, ids) in enumerate((("mesh_texture", mesh_texture),
                                     ("triangle_texture", triangle_texture),
                                     ("sphere_texture", sphere_texture))):
        if ids is None:
            continue
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if counts is not None and a.size != counts[i]:
            raise ValueError(f"{name} must hold {counts[i]} ids")
        keep.append(a)
        setattr(d, name, a.ctypes.data_as(C.POINTER(C.c_int)))
    return d, keep


def _texture_images(images: dict):
    """rt_texture_image records for {name: (h, w, 3) uint8 array}, and what they point into."""
    keep = []
    recs = (_lib.rt_texture_image * max(1, len(images)))()
    for k, (name, px) in enumerate(images.items()):
        px = np.ascontiguousarray(px, np.uint8)
        if px.ndim != 3 or px.shape[2] != 3:
            raise ValueError("an image must be an (h, w, 3) uint8 array")
        keep.append(px)
        recs[k].name = str(name).encode()
        recs[k].rgb8 = px.ctypes.data_as(C.POINTER(C.c_ubyte))
        recs[k].height, recs[k].width = int(px.shape[0]), int(px.shape[1])
    return recs, keep


def host_textures_xml(xml_path: str) -> dict:
    """Host-only (rt_host_textures_xml): what the textured loader read from a scene file —
    ``textures`` (a list of dicts: name, interpolation, decal, appearance, normalizer),
    ``mesh_texture`` / ``triangle_texture`` / ``sphere_texture`` (0-based ids, -1: none) and ``uv``
    (the <TexCoordData> pairs, (n, 2) float32)."""
    path = str(xml_path).encode()
    counts = (C.c_int * 5)()
    check(lib().rt_host_textures_xml(path, None, None, None, 0, None, None, None, 0, None, 0,
                                     counts))
    nt, nm, ntri, ns, nuv = list(counts)
    names = C.create_string_buffer(256 * max(1, nt))
    modes = np.zeros((max(1, nt), 3), np.int32)
    norm = np.zeros(max(1, nt), np.float32)
    cap = max(1, nm, ntri, ns)
    ids = [np.full(cap, -9, np.int32) for _ in range(3)]
    uv = np.zeros((max(1, nuv), 2), np.float32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    check(lib().rt_host_textures_xml(path, names, ip(modes), fp(norm), nt, ip(ids[0]), ip(ids[1]),
                                     ip(ids[2]), cap, fp(uv), nuv, counts))
    textures = [dict(name=names.raw[256 * k:256 * (k + 1)].split(b"\0")[0].decode(),
                     interpolation=int(modes[k, 0]), decal=int(modes[k, 1]),
                     appearance=int(modes[k, 2]), normalizer=float(norm[k])) for k in range(nt)]
    return dict(textures=textures, mesh_texture=ids[0][:nm].copy(),
                triangle_texture=ids[1][:ntri].copy(), sphere_texture=ids[2][:ns].copy(),
                uv=uv[:nuv].copy())


def _tex_queries(texture, u, v) -> np.ndarray:
    u = np.asarray(u, np.float32).reshape(-1)
    v = np.asarray(v, np.float32).reshape(-1)
    if u.shape != v.shape:
        raise ValueError("u and v must hold the same number of values")
    q = _aligned(len(u), TEX_QUERY_DTYPE)
    q["texture"] = np.broadcast_to(np.asarray(texture, np.int32), (len(u),))
    q["u"], q["v"] = u, v
    return q


def host_texture_lookup(textures, texture, u, v) -> np.ndarray:
    """rt_host_texture_lookup_desc: Texture::get_color_at of ``textures[texture]`` (a list as
    ``Scene.create`` takes it) at (u, v) on the host, no GPU: (n, 3) float32 raw channel values;
    a texture id out of range gives zeros."""
    d, keep = texture_desc(textures)
    q = _tex_queries(texture, u, v)
    out = np.zeros((len(q), 3), np.float32)
    check(lib().rt_host_texture_lookup_desc(C.byref(d), q.ctypes.data, len(q), out.ctypes.data))
    return out


def pack_lights(lights, n: int, shared: bool):
    """The caller's LIGHT_SAMPLE_DTYPE records, shape (n, k) or shared (k,), as a 16-byte aligned
    array and k."""
    a = np.asarray(lights)
    if a.dtype != LIGHT_SAMPLE_DTYPE:
        raise ValueError("lights must be a LIGHT_SAMPLE_DTYPE array")
    if shared:
        if a.ndim != 1:
            raise ValueError("shared lights must have shape (k,)")
    elif a.ndim != 2 or a.shape[0] != n:
        raise ValueError("lights must have shape (n, k), one row per ray")
    out = _aligned(a.size, LIGHT_SAMPLE_DTYPE)
    out[...] = a.reshape(-1)
    return out, int(a.shape[-1])


@dataclass
class CameraInfo:
    width: int
    height: int
    num_samples: int
    image_name: str
    e: tuple
    top_left: tuple
    s_u: tuple
    s_v: tuple


class Scene:
    """HW2 ``Scene``: parse an XML scene and render its cameras on the GPU.

    ``render_image(camera_index, result, starting_row, height_increase)`` has the reference's
    argument meaning (HW2/Scene.cpp:16-31): rows ``starting_row + k*height_increase`` of
    ``result`` (an ``(h, w, 3)`` float32 array standing for ``Pixel[w*h]``) receive the fp32
    radiance ``Pixel::color``; other rows are untouched.  Errors raise ``RTError`` (the
    reference throws ``std::runtime_error`` from the loader, HW2/Scene.cpp:204,208).

    ``devices`` (a list of GPU ordinals) makes one scene over several GPUs of this process
    (rt_scene_load_xml_multi): every frame's tiles are dealt over them and gathered onto
    ``devices[0]`` with RCCL.
    """

    def __init__(self, file_name: str, device: int = -1, traversal: str = "fast",
                 devices: Optional[list] = None, smooth: bool = False, instanced: bool = False,
                 motion: bool = False, textured: bool = False, images: Optional[dict] = None):
        h = C.c_void_p()
        if textured:  # <Textures>, <TexCoordData>, <Texture> honoured (rt_scene_load_xml_textured)
            if instanced or motion or devices is not None:
                raise _lib.RTError(_lib.RT_E_UNSUPPORTED, "textured scenes are single-device, "
                                   "without instances and without motion")
            recs, keep = _texture_images(images or {})
            check(lib().rt_scene_load_xml_textured(str(file_name).encode(), recs, len(images or {}),
                                                   device, C.byref(h)))
        elif motion:  # rt_scene_load_xml_moving: also <MotionBlur> and a sphere's <Transformations>
            if smooth or devices is not None or not instanced:
                raise _lib.RTError(_lib.RT_E_UNSUPPORTED, "scenes with motion are instanced, "
                                   "single-device and flat-shaded")
            check(lib().rt_scene_load_xml_moving(str(file_name).encode(), device, C.byref(h)))
        elif instanced:  # <Transformations> / <MeshInstance> honoured (rt_scene_load_xml_instanced)
            if smooth or devices is not None:
                raise _lib.RTError(_lib.RT_E_UNSUPPORTED, "instanced scenes are single-device "
                                   "and flat-shaded")
            check(lib().rt_scene_load_xml_instanced(str(file_name).encode(), device, C.byref(h)))
        elif devices is not None:
            if smooth:
                raise _lib.RTError(_lib.RT_E_UNSUPPORTED,
                                   "smooth shading on multi-device scenes is not supported")
            arr = (C.c_int * len(devices))(*devices)
            check(lib().rt_scene_load_xml_multi(str(file_name).encode(), len(devices), arr,
                                                C.byref(h)))
        elif smooth:  # <Mesh shadingMode="smooth"> honoured (rt_scene_load_xml_surface)
            check(lib().rt_scene_load_xml_surface(str(file_name).encode(), device, C.byref(h)))
        else:
            check(lib().rt_scene_load_xml(str(file_name).encode(), device, C.byref(h)))
        self._h = h
        self.set_traversal(traversal)

    @classmethod
    def create(cls, desc, mesh_smooth=None, vertex_normals=None, vertex_uv=None,
               device: int = -1, instance_mesh=None, instance_material=None,
               instance_transform=None, instance_velocity=None, sphere_transform=None,
               sphere_velocity=None, textures=None, mesh_texture=None, triangle_texture=None,
               sphere_texture=None) -> "Scene":
        """A scene from an ``rt_scene_desc`` with surface data (rt_scene_create_surface):
        ``mesh_smooth`` one flag per mesh, ``vertex_normals`` (num_vertices, 3) used as given
        (None: the area-weighted normals of the HW3 loader), ``vertex_uv`` (num_vertices, 2).

        Or a scene made of instances (rt_scene_create_instanced): ``instance_mesh`` and
        ``instance_material`` (n,) and ``instance_transform`` (n, 4, 4) object -> world; the
        description's meshes are then bases only.  Not together with surface data.

        Or a scene with motion (rt_scene_create_moving): ``instance_velocity`` (n, 3),
        ``sphere_transform`` (num_spheres, 4, 4) and ``sphere_velocity`` (num_spheres, 3), each
        optional, with or without instances.

        ``textures`` (rt_scene_create_textured, with surface data or without): a list of dicts
        (``texture_desc``), and ``mesh_texture`` / ``triangle_texture`` / ``sphere_texture``, one
        texture id per object, -1 for none.  Not together with instances or motion."""
        textured = any(a is not None for a in (textures, mesh_texture, triangle_texture,
                                               sphere_texture))
        if textured and any(a is not None for a in (instance_mesh, instance_material,
                                                    instance_transform, instance_velocity,
                                                    sphere_transform, sphere_velocity)):
            raise _lib.RTError(_lib.RT_E_UNSUPPORTED,
                               "textures in instanced scenes or scenes with motion are not supported")
        given = [a is not None for a in (instance_mesh, instance_material, instance_transform)]
        if any(given) and not all(given):
            raise ValueError("instance_mesh, instance_material and instance_transform go together")
        if any(a is not None for a in (instance_velocity, sphere_transform, sphere_velocity)):
            if mesh_smooth is not None or vertex_normals is not None or vertex_uv is not None:
                raise _lib.RTError(_lib.RT_E_UNSUPPORTED,
                                   "surface data in scenes with motion is not supported")
            inst = keep = None
            if instance_mesh is not None:
                inst, keep = _instance_desc(instance_mesh, instance_material, instance_transform)
            mo, keep2 = _motion_desc(desc, inst, instance_velocity, sphere_transform, sphere_velocity)
            h = C.c_void_p()
            check(lib().rt_scene_create_moving(C.byref(desc), C.byref(inst) if inst else None,
                                               C.byref(mo), device, C.byref(h)))
            return cls._from_handle(h)
        if instance_mesh is not None:
            if mesh_smooth is not None or vertex_normals is not None or vertex_uv is not None:
                raise _lib.RTError(_lib.RT_E_UNSUPPORTED,
                                   "surface data in instanced scenes is not supported")
            inst, keep = _instance_desc(instance_mesh, instance_material, instance_transform)
            h = C.c_void_p()
            check(lib().rt_scene_create_instanced(C.byref(desc), C.byref(inst), device, C.byref(h)))
            return cls._from_handle(h)
        surf = _lib.rt_surface_desc()
        surf.struct_size = C.sizeof(_lib.rt_surface_desc)
        keep = []

        def arr(a, dtype, count, ctype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype).reshape(-1)
            if a.size != count:
                raise ValueError(f"{what} must hold {count} values")
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ctype))

        surf.mesh_smooth = arr(mesh_smooth, np.uint8, desc.num_meshes, C.c_ubyte, "mesh_smooth")
        surf.vertex_normals = arr(vertex_normals, np.float32, 3 * desc.num_vertices, C.c_float,
                                  "vertex_normals")
        surf.vertex_uv = arr(vertex_uv, np.float32, 2 * desc.num_vertices, C.c_float, "vertex_uv")
        h = C.c_void_p()
        if textured:
            td, keep_tex = texture_desc(textures or [], mesh_texture, triangle_texture,
                                        sphere_texture,
                                        (desc.num_meshes, desc.num_triangles, desc.num_spheres))
            check(lib().rt_scene_create_textured(C.byref(desc), C.byref(surf), C.byref(td), device,
                                                 C.byref(h)))
            return cls._from_handle(h)
        check(lib().rt_scene_create_surface(C.byref(desc), C.byref(surf), device, C.byref(h)))
        return cls._from_handle(h)

    @classmethod
    def _from_handle(cls, h: C.c_void_p) -> "Scene":
        s = cls.__new__(cls)
        s._h = h
        return s

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            lib().rt_scene_destroy(self._h)
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

    # ------------------------------------------------------------------ queries
    @property
    def handle(self) -> C.c_void_p:
        return self._h

    @property
    def num_cameras(self) -> int:
        return lib().rt_scene_num_cameras(self._h)

    @property
    def num_lights(self) -> int:
        return lib().rt_scene_num_lights(self._h)

    @property
    def device_count(self) -> int:
        return lib().rt_scene_device_count(self._h)

    @property
    def num_textures(self) -> int:
        """rt_scene_num_textures: 0 for an untextured scene."""
        return lib().rt_scene_num_textures(self._h)

    def texture_lookup(self, texture, u, v) -> np.ndarray:
        """rt_texture_lookup: Texture::get_color_at of the scene's texture ``texture`` (one id, or
        one per query) at (u, v) on the GPU: (n, 3) float32 raw channel values; a texture id out
        of range gives zeros."""
        q = _tex_queries(texture, u, v)
        out = np.zeros((len(q), 3), np.float32)
        check(lib().rt_texture_lookup(self._h, q.ctypes.data, len(q), out.ctypes.data))
        return out

    @property
    def bvh_depth(self) -> int:
        return lib().rt_scene_bvh_depth(self._h)

    def camera(self, i: int) -> CameraInfo:
        c = _lib.rt_camera()
        check(lib().rt_scene_camera(self._h, i, C.byref(c)))
        name = lib().rt_scene_image_name(self._h, i).decode()
        return CameraInfo(c.width, c.height, c.num_samples, name, tuple(c.e),
                          tuple(c.top_left), tuple(c.s_u), tuple(c.s_v))

    def set_traversal(self, mode: str) -> None:
        m = {"fast": _lib.RT_TRAVERSAL_FAST, "reference": _lib.RT_TRAVERSAL_REFERENCE}[mode]
        check(lib().rt_set_traversal(self._h, m))

    def set_msaa_seed(self, seed: int) -> None:
        """Seed of the per-pixel MSAA generators (the reference uses the wall clock)."""
        check(lib().rt_set_msaa_seed(self._h, int(seed)))

    def dump_bvh(self, path: str) -> None:
        check(lib().rt_scene_dump_bvh(self._h, str(path).encode()))

    # ------------------------------------------------------------------ rendering
    def new_image(self, camera_index: int) -> np.ndarray:
        c = self.camera(camera_index)
        return np.zeros((c.height, c.width, 3), np.float32)

    def render_image(self, camera_index: int, result: Optional[np.ndarray] = None,
                     starting_row: int = 0, height_increase: int = 1):
        """Scene::render_image (HW2/Scene.h:34-35).  Returns (result, rt_stats).

        NumSamples > 1: whole frames only; result is Pixel::color / Pixel::weight."""
        if result is None:
            result = self.new_image(camera_index)
        c = self.camera(camera_index)
        if result.dtype != np.float32 or not result.flags.c_contiguous or \
                result.size != c.width * c.height * 3:
            raise ValueError("result must be a C-contiguous float32 array of h*w*3 values")
        st = _lib.rt_stats()
        check(lib().rt_render(self._h, camera_index, starting_row, height_increase,
                              result.ctypes.data, C.byref(st)))
        return result, st

    def num_tiles(self, camera_index: int, starting_row: int = 0, row_stride: int = 1) -> int:
        return check(lib().rt_num_tiles(self._h, camera_index, starting_row, row_stride))

    def render_device(self, camera_index: int, out_ptr: int, *, starting_row: int = 0,
                      row_stride: int = 1, tile_begin: int = 0, tile_step: int = 1,
                      tile_major: bool = False, blocks: bool = False, stream: int = 0,
                      tile_count: int = -1, records: bool = False) -> None:
        """Asynchronous render into device memory at ``out_ptr`` on HIP stream ``stream``
        (deal units tile_begin + k*tile_step, k < tile_count; tile_count < 0: all of them; a
        unit is a tile, or with ``blocks`` a 2x2 block of tiles in deal order —
        RT_TILE_BLOCKS of include/ceng795_rt.h).  ``records`` (with ``tile_major``): 64
        32-bit pixel records per tile instead of RGB (RT_TILE_RECORDS)."""
        flags = ((RT_TILE_MAJOR if tile_major else 0) | (RT_TILE_BLOCKS if blocks else 0) |
                 (RT_TILE_RECORDS if records else 0))
        check(lib().rt_render_device_range(self._h, camera_index, starting_row, row_stride,
                                           tile_begin, tile_step, tile_count, flags,
                                           C.c_void_p(out_ptr), C.c_void_p(stream)))

    def untile_device(self, camera_index: int, devices: int, slot: int, gathered_ptr: int,
                      out_ptr: int, *, tile_offset: int = 0, blocks: bool = False,
                      skip_root: bool = False, stream: int = 0) -> None:
        """rt_untile_device: the gathered [devices][slot][64][3] tile shares of a round-robin
        deal (unit u to rank (u + tile_offset) mod devices; units are tiles, or 2x2 blocks in
        deal order with ``blocks``) into the row-major frame; ``skip_root``: rank 0's units
        are left as they are (rendered in place)."""
        flags = (RT_UNTILE_BLOCKS if blocks else 0) | (RT_UNTILE_SKIP_ROOT if skip_root else 0)
        check(lib().rt_untile_device(self._h, camera_index, 0, 1, devices, slot, tile_offset,
                                     flags, C.c_void_p(gathered_ptr), C.c_void_p(out_ptr),
                                     C.c_void_p(stream)))

    def tile_costs(self, stream: int, capacity: int) -> "np.ndarray":
        """rt_tile_costs: every tile's measured time (100 MHz ticks) in the last frame enqueued on
        HIP stream ``stream``, in that call's selection order (waits for the stream)."""
        out = np.zeros(max(1, capacity), dtype=np.uint32)
        n = check(lib().rt_tile_costs(self._h, C.c_void_p(stream),
                                      out.ctypes.data_as(C.c_void_p), capacity))
        return out[:n]

    def resolve_rows(self, camera_index: int, row_begin: int, row_end: int, records_ptr: int,
                     out_ptr: int, *, stream: int = 0) -> None:
        """rt_resolve_rows: row-major pixel records (one 32-bit word per pixel of the frame)
        shaded into rows [row_begin, row_end) of the row-major frame at ``out_ptr``."""
        check(lib().rt_resolve_rows(self._h, camera_index, row_begin, row_end,
                                    C.c_void_p(records_ptr), C.c_void_p(out_ptr),
                                    C.c_void_p(stream)))

    def records_ok(self, camera_index: int) -> bool:
        """rt_scene_records_ok: may this camera's shares travel as pixel records?"""
        return bool(check(lib().rt_scene_records_ok(self._h, camera_index)))

    def resolve_device(self, camera_index: int, devices: int, slot: int, gathered_ptr: int,
                       out_ptr: int, *, tile_offset: int = 0, blocks: bool = False,
                       skip_root: bool = False, stream: int = 0) -> None:
        """rt_resolve_device: gathered pixel records [devices][slot][64] (RT_TILE_RECORDS
        shares) shaded into the row-major frame (the layout and flags of untile_device)."""
        flags = (RT_UNTILE_BLOCKS if blocks else 0) | (RT_UNTILE_SKIP_ROOT if skip_root else 0)
        check(lib().rt_resolve_device(self._h, camera_index, 0, 1, devices, slot, tile_offset,
                                      flags, C.c_void_p(gathered_ptr), C.c_void_p(out_ptr),
                                      C.c_void_p(stream)))

    # ------------------------------------------------------------------ ray queries
    def trace_rays(self, origins, directions, *, reorder: bool = False, time=None) -> np.ndarray:
        """Closest hit of each ray o + t d (rt_trace_rays): a HIT_DTYPE array with the
        reference's Hit_data::t and normal, the object / material / DFS leaf hit; a miss has
        t = +inf and object = material = leaf = -1.  ``reorder``: group similar rays before
        tracing (RT_QUERY_REORDER; same results).  ``time``: the rays' times, a scalar or (n,)
        (RT_QUERY_RAY_TIME; a scene with motion meets its moving objects where they are then)."""
        rays = pack_rays(origins, directions, time=time)
        hits = _aligned(len(rays), HIT_DTYPE)
        check(lib().rt_trace_rays(self._h, rays.ctypes.data, len(rays), hits.ctypes.data,
                                  (_lib.RT_QUERY_REORDER if reorder else 0) | _time_flag(time)))
        return hits

    def occluded(self, origins, directions, tmax, *, reorder: bool = False,
                 time=None) -> np.ndarray:
        """uint8[n]: 1 where something lies at 0 < t < tmax along the ray (rt_occluded)."""
        rays = pack_rays(origins, directions, tmax, time)
        occ = np.zeros(len(rays), np.uint8)
        check(lib().rt_occluded(self._h, rays.ctypes.data, len(rays), occ.ctypes.data,
                                (_lib.RT_QUERY_REORDER if reorder else 0) | _time_flag(time)))
        return occ

    def trace_rays_device(self, rays_ptr: int, n: int, hits_ptr: int, *, reorder: bool = False,
                          stream: int = 0, ray_time: bool = False) -> None:
        """rt_trace_rays_device: n rt_ray records in device memory at ``rays_ptr`` (e.g. a torch
        tensor's ``data_ptr()``) to n rt_ray_hit records at ``hits_ptr``, asynchronously on HIP
        stream ``stream``."""
        check(lib().rt_trace_rays_device(self._h, C.c_void_p(rays_ptr), n, C.c_void_p(hits_ptr),
                                         (_lib.RT_QUERY_REORDER if reorder else 0) |
                                         (_lib.RT_QUERY_RAY_TIME if ray_time else 0),
                                         C.c_void_p(stream)))

    def occluded_device(self, rays_ptr: int, n: int, occ_ptr: int, *, reorder: bool = False,
                        stream: int = 0, ray_time: bool = False) -> None:
        """rt_occluded_device: one byte (0 / 1) per ray at ``occ_ptr``."""
        check(lib().rt_occluded_device(self._h, C.c_void_p(rays_ptr), n, C.c_void_p(occ_ptr),
                                       (_lib.RT_QUERY_REORDER if reorder else 0) |
                                       (_lib.RT_QUERY_RAY_TIME if ray_time else 0),
                                       C.c_void_p(stream)))

    # ------------------------------------------------------------------ hit attributes
    @property
    def num_instances(self) -> int:
        """Instances of the scene (rt_scene_num_instances); 0: a flat scene."""
        return lib().rt_scene_num_instances(self._h)

    @property
    def has_motion(self) -> bool:
        """The scene has a moving object or a transformed sphere (rt_scene_has_motion)."""
        return bool(lib().rt_scene_has_motion(self._h))

    @property
    def has_smooth(self) -> bool:
        """Some mesh of the scene is smooth-shaded (rt_scene_has_smooth)."""
        return bool(lib().rt_scene_has_smooth(self._h))

    def hit_attributes(self, origins, directions, hits) -> np.ndarray:
        """Where each ray hit its primitive (rt_hit_attributes): ``hits`` is the HIT_DTYPE array
        ``trace_rays`` gave for these rays; returns a HIT_ATTR_DTYPE array with the triangle's
        ``beta`` / ``gamma``, the interpolated ``uv``, the shading normal (smooth on a smooth
        mesh) and the geometric normal.  A miss or an invalid ray: the all-zero record."""
        rays = pack_rays(origins, directions)
        h = np.asarray(hits)
        if h.dtype != HIT_DTYPE or h.shape != (len(rays),):
            raise ValueError("hits must be a HIT_DTYPE array with one record per ray")
        hin = _aligned(len(rays), HIT_DTYPE)
        hin[...] = h
        attr = _aligned(len(rays), HIT_ATTR_DTYPE)
        check(lib().rt_hit_attributes(self._h, rays.ctypes.data, hin.ctypes.data, len(rays),
                                      attr.ctypes.data))
        return attr

    def hit_attributes_device(self, rays_ptr: int, hits_ptr: int, n: int, attr_ptr: int, *,
                              stream: int = 0) -> None:
        """rt_hit_attributes_device: n rt_ray and n rt_ray_hit records in device memory to n
        rt_hit_attr records at ``attr_ptr``, asynchronously on HIP stream ``stream``."""
        check(lib().rt_hit_attributes_device(self._h, C.c_void_p(rays_ptr), C.c_void_p(hits_ptr), n,
                                             C.c_void_p(attr_ptr), C.c_void_p(stream)))

    # ------------------------------------------------------------------ radiance queries
    @staticmethod
    def _radiance_flags(in_medium: bool, reorder: bool, ray_time: bool = False) -> int:
        return ((_lib.RT_QUERY_IN_MEDIUM if in_medium else 0) |
                (_lib.RT_QUERY_REORDER if reorder else 0) |
                (_lib.RT_QUERY_RAY_TIME if ray_time else 0))

    def shade_rays(self, origins, directions, *, depth: Optional[int] = None,
                   in_medium: bool = False, reorder: bool = False, stats: bool = False,
                   time=None):
        """Scene::trace_ray of each ray o + t d (rt_shade_rays): a RADIANCE_DTYPE array with the
        colour ``rgb`` a frame would hold for that ray and the first hit's ``t`` (+inf on a
        miss).  ``depth``: the reference's current_recursion_depth, None = the scene's
        MaxRecursionDepth; a miss returns the background only at that maximum.  ``in_medium``:
        every ray starts inside a dielectric (no local shading at its first hit).  With
        ``stats`` returns (array, rt_stats of this call).  ``time``: the rays' times (a scalar or
        (n,)), which every ray of a ray's tree inherits (RT_QUERY_RAY_TIME)."""
        rays = pack_rays(origins, directions, time=time)
        out = _aligned(len(rays), RADIANCE_DTYPE)
        st = _lib.rt_stats()
        check(lib().rt_shade_rays(self._h, rays.ctypes.data, len(rays),
                                  -1 if depth is None else int(depth), out.ctypes.data,
                                  self._radiance_flags(in_medium, reorder, time is not None),
                                  C.byref(st)))
        return (out, st) if stats else out

    def shade_rays_device(self, rays_ptr: int, n: int, out_ptr: int, *,
                          depth: Optional[int] = None, in_medium: bool = False,
                          reorder: bool = False, stream: int = 0, ray_time: bool = False) -> None:
        """rt_shade_rays_device: n rt_ray records in device memory at ``rays_ptr`` to n
        rt_radiance records at ``out_ptr``, asynchronously on HIP stream ``stream``; the ray
        counts go to collect_stats()."""
        check(lib().rt_shade_rays_device(self._h, C.c_void_p(rays_ptr), n,
                                         -1 if depth is None else int(depth), C.c_void_p(out_ptr),
                                         self._radiance_flags(in_medium, reorder, ray_time),
                                         C.c_void_p(stream)))

    @staticmethod
    def _lit_flags(in_medium: bool, reorder: bool, shared: bool, scene_lights: bool,
                   ray_time: bool = False) -> int:
        return (Scene._radiance_flags(in_medium, reorder, ray_time) |
                (_lib.RT_QUERY_LIGHTS_SHARED if shared else 0) |
                (0 if scene_lights else _lib.RT_QUERY_NO_SCENE_LIGHTS))

    def shade_rays_lit(self, origins, directions, lights, *, shared: bool = False,
                       scene_lights: bool = True, depth: Optional[int] = None,
                       in_medium: bool = False, reorder: bool = False, stats: bool = False,
                       time=None):
        """``shade_rays`` with each ray's own light samples (rt_shade_rays_lit): ``lights`` is a
        LIGHT_SAMPLE_DTYPE array of shape (n, k), row i lighting ray i's whole tree after the
        scene's point lights — or, with ``shared``, of shape (k,) for every ray.  A record with
        a non-finite ``position`` is no light; ``normal`` 0 0 0 is a point light, any other
        normal an emitter sample whose terms carry dot(-w_i, normal).  ``scene_lights=False``
        leaves the scene's own lights out."""
        rays = pack_rays(origins, directions, time=time)
        lit, k = pack_lights(lights, len(rays), shared)
        out = _aligned(len(rays), RADIANCE_DTYPE)
        st = _lib.rt_stats()
        check(lib().rt_shade_rays_lit(self._h, rays.ctypes.data, len(rays),
                                      -1 if depth is None else int(depth), lit.ctypes.data, k,
                                      out.ctypes.data,
                                      self._lit_flags(in_medium, reorder, shared, scene_lights,
                                                      time is not None),
                                      C.byref(st)))
        return (out, st) if stats else out

    def shade_rays_lit_device(self, rays_ptr: int, n: int, lights_ptr: int, k: int, out_ptr: int, *,
                              shared: bool = False, scene_lights: bool = True,
                              depth: Optional[int] = None, in_medium: bool = False,
                              reorder: bool = False, stream: int = 0,
                              ray_time: bool = False) -> None:
        """rt_shade_rays_lit_device: n rt_ray records and their n x k (shared: k)
        rt_light_sample records in device memory, asynchronously on HIP stream ``stream``."""
        check(lib().rt_shade_rays_lit_device(
            self._h, C.c_void_p(rays_ptr), n, -1 if depth is None else int(depth),
            C.c_void_p(lights_ptr), int(k), C.c_void_p(out_ptr),
            self._lit_flags(in_medium, reorder, shared, scene_lights, ray_time),
            C.c_void_p(stream)))

    def set_radiance_scratch_limit(self, nbytes: int) -> None:
        """Bytes of ray-tree frames one chunk of a recursing radiance query may hold (0: the
        default, 256 MiB)."""
        check(lib().rt_set_radiance_scratch_limit(self._h, int(nbytes)))

    def stream_frame_scratch_bytes(self, stream: int) -> int:
        """Bytes of ray-tree frames the scene keeps for HIP stream ``stream`` (0: none)."""
        return check(lib().rt_stream_frame_scratch_bytes(self._h, C.c_void_p(stream)))

    def release_stream(self, stream: int) -> None:
        """Frees the scratch the library keeps for HIP stream ``stream`` (after waiting for it)."""
        check(lib().rt_release_stream_scratch(self._h, C.c_void_p(stream)))

    def set_kernel_timing(self, enable: bool) -> None:
        check(lib().rt_set_kernel_timing(self._h, int(enable)))

    def read_kernel_times(self):
        """(ms summed {frame kernel, order kernel, other, total}, launches) since the last read."""
        ms = (C.c_double * 4)()
        n = C.c_longlong()
        check(lib().rt_read_kernel_times(self._h, ms, C.byref(n)))
        keys = ("frame", "order", "other", "total")
        return dict(zip(keys, list(ms))), n.value

    DIAG_NAMES = ["primary_rays", "shadow_rays", "secondary_rays", "primary_hits",
                  "prim_node_visits", "prim_node_lanes", "prim_leaf_visits", "prim_leaf_lanes",
                  "shad_node_visits", "shad_node_lanes", "shad_leaf_visits", "shad_leaf_lanes",
                  "exact_box_fallbacks", "guard_tests", "prim_wide_visits",
                  "shad_wide_visits"]

    def debug_counters(self) -> dict:
        """All device counters (diagnostic columns only in the CENG795_LIB=diag build)."""
        arr = (C.c_longlong * 16)()
        diag = check(lib().rt_debug_counters(self._h, arr))
        d = dict(zip(self.DIAG_NAMES, list(arr)))
        d["diag_build"] = bool(diag)
        return d

    def collect_stats(self) -> "_lib.rt_stats":
        st = _lib.rt_stats()
        check(lib().rt_collect_stats(self._h, C.byref(st)))
        return st


def write_png(path: str, rgb: np.ndarray) -> None:
    """HW2/main.cpp:43-57: clamp(int(c), 0, 255) per channel."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    check(lib().rt_write_png(str(path).encode(), rgb.ctypes.data, w, h))


def host_dump_bvh(xml_path: str, out_path: str) -> None:
    """Host-only: parse + build + flatten the BVH and dump it (no GPU needed)."""
    check(lib().rt_host_dump_bvh_xml(str(xml_path).encode(), str(out_path).encode()))


def host_vertex_normals(desc) -> np.ndarray:
    """Host-only (rt_host_vertex_normals_desc): the (num_vertices, 3) area-weighted vertex normals
    a smooth scene made from ``desc`` (an ``rt_scene_desc``) uses when the caller gives none."""
    out = np.zeros((max(0, desc.num_vertices), 3), np.float32)
    check(lib().rt_host_vertex_normals_desc(C.byref(desc), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def _instance_desc(instance_mesh, instance_material, instance_transform):
    """An ``rt_instance_desc`` over the three arrays, and the arrays it points into."""
    mesh = np.ascontiguousarray(instance_mesh, np.int32).reshape(-1)
    mat = np.ascontiguousarray(instance_material, np.int32).reshape(-1)
    xf = np.ascontiguousarray(instance_transform, np.float32).reshape(-1)
    if mat.size != mesh.size or xf.size != 16 * mesh.size:
        raise ValueError("instance_material needs n values and instance_transform n x 4 x 4")
    inst = _lib.rt_instance_desc()
    inst.struct_size = C.sizeof(_lib.rt_instance_desc)
    inst.num_instances = mesh.size
    inst.instance_mesh = mesh.ctypes.data_as(C.POINTER(C.c_int))
    inst.instance_material = mat.ctypes.data_as(C.POINTER(C.c_int))
    inst.instance_transform = xf.ctypes.data_as(C.POINTER(C.c_float))
    return inst, (mesh, mat, xf)


def host_instance_info(desc, instance_mesh, instance_material, instance_transform):
    """Host-only (rt_host_instance_info_desc): per instance its inverse matrix (n, 4, 4), its world
    box (n, 6: min xyz, max xyz) and its DFS position among the top-level leaves (n,)."""
    inst, keep = _instance_desc(instance_mesh, instance_material, instance_transform)
    n = inst.num_instances
    inverse = np.zeros((n, 4, 4), np.float32)
    box = np.zeros((n, 6), np.float32)
    top = np.zeros(n, np.int32)
    check(lib().rt_host_instance_info_desc(C.byref(desc), C.byref(inst),
                                           inverse.ctypes.data_as(C.POINTER(C.c_float)),
                                           box.ctypes.data_as(C.POINTER(C.c_float)),
                                           top.ctypes.data_as(C.POINTER(C.c_int))))
    return inverse, box, top


def _motion_desc(desc, inst, instance_velocity, sphere_transform, sphere_velocity):
    """An ``rt_motion_desc`` over the three optional arrays, and the arrays it points into."""
    ni = inst.num_instances if inst is not None else 0
    ns = desc.num_spheres
    keep = []

    def arr(a, count, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        if a.size != count:
            raise ValueError(f"{what} must hold {count} values")
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_float))

    mo = _lib.rt_motion_desc()
    mo.struct_size = C.sizeof(_lib.rt_motion_desc)
    mo.num_instances, mo.num_spheres = ni, ns
    mo.instance_velocity = arr(instance_velocity, 3 * ni, "instance_velocity")
    mo.sphere_transform = arr(sphere_transform, 16 * ns, "sphere_transform")
    mo.sphere_velocity = arr(sphere_velocity, 3 * ns, "sphere_velocity")
    return mo, keep


def host_motion_info(desc, instance_mesh=None, instance_material=None, instance_transform=None,
                     instance_velocity=None, sphere_transform=None, sphere_velocity=None):
    """Host-only (rt_host_motion_info_desc): every instance's box, expanded by its velocity
    (ni, 6), every sphere's inverse matrix (ns, 4, 4) and box (ns, 6), and the top-level DFS
    position of every top-level object (instances, loose triangles, spheres)."""
    inst = keep = None
    if instance_mesh is not None:
        inst, keep = _instance_desc(instance_mesh, instance_material, instance_transform)
    mo, keep2 = _motion_desc(desc, inst, instance_velocity, sphere_transform, sphere_velocity)
    ni, ns = mo.num_instances, mo.num_spheres
    inst_box = np.zeros((ni, 6), np.float32)
    inverse = np.zeros((ns, 4, 4), np.float32)
    box = np.zeros((ns, 6), np.float32)
    top = np.zeros(ni + desc.num_triangles + ns, np.int32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    check(lib().rt_host_motion_info_desc(C.byref(desc), C.byref(inst) if inst else None,
                                         C.byref(mo), fp(inst_box), fp(inverse), fp(box),
                                         top.ctypes.data_as(C.POINTER(C.c_int))))
    return inst_box, inverse, box, top


def host_motion_xml(xml_path: str):
    """Host-only (rt_host_motion_xml): what the motion loader read beside host_instances_xml's
    arrays — (instance velocity (ni, 3), sphere transform (ns, 4, 4), sphere velocity (ns, 3))."""
    path = str(xml_path).encode()
    counts = (C.c_int * 2)()
    check(lib().rt_host_motion_xml(path, None, None, None, 0, counts))
    ni, ns = counts[0], counts[1]
    vel = np.zeros((ni, 3), np.float32)
    xf = np.zeros((ns, 4, 4), np.float32)
    svel = np.zeros((ns, 3), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    check(lib().rt_host_motion_xml(path, fp(vel), fp(xf), fp(svel), max(ni, ns), counts))
    return vel, xf, svel


def host_instances_xml(xml_path: str):
    """Host-only (rt_host_instances_xml): the scene file's instances as the instanced loader makes
    them — (mesh (n,), material (n,), transform (n, 4, 4)): every <Mesh> with its own
    transformation, then the <MeshInstance>s."""
    path = str(xml_path).encode()
    n = check(lib().rt_host_instances_xml(path, None, None, None, 0))
    mesh, mat = np.zeros(n, np.int32), np.zeros(n, np.int32)
    xf = np.zeros((n, 4, 4), np.float32)
    check(lib().rt_host_instances_xml(path, mesh.ctypes.data_as(C.POINTER(C.c_int)),
                                      mat.ctypes.data_as(C.POINTER(C.c_int)),
                                      xf.ctypes.data_as(C.POINTER(C.c_float)), n))
    return mesh, mat, xf


def host_mesh_smooth(xml_path: str) -> np.ndarray:
    """Host-only (rt_host_mesh_smooth_xml): uint8 per <Mesh>, 1 where shadingMode="smooth"."""
    n = check(lib().rt_host_mesh_smooth_xml(str(xml_path).encode(), None, 0))
    out = np.zeros(n, np.uint8)
    check(lib().rt_host_mesh_smooth_xml(str(xml_path).encode(),
                                        out.ctypes.data_as(C.POINTER(C.c_ubyte)), n))
    return out


def host_leaf_objects(desc) -> np.ndarray:
    """Host-only (rt_host_leaf_objects_desc): for each DFS leaf of the tree of ``desc`` (an
    ``rt_scene_desc``) its index in the object lists, the ``object`` a ray query reports."""
    n = check(lib().rt_host_leaf_objects_desc(C.byref(desc), None, 0))
    out = np.zeros(n, np.int32)
    check(lib().rt_host_leaf_objects_desc(C.byref(desc), out.ctypes.data_as(C.POINTER(C.c_int)), n))
    return out
