"""ceng795_amd — MI355X-native ray-trace hot path of kadircet/ceng795 HW2.

Python mirror of the reference's render interface (HW2/Scene.h:30-43):

    scene = Scene("scene.xml")                       # Scene::Scene(file_name)
    pixels = scene.new_image(camera_index)           # Pixel[w*h]  (fp32 RGB radiance)
    scene.render_image(camera_index, pixels, starting_row, height_increase)
    write_png(name, pixels)                          # HW2/main.cpp:43-57
    hits = scene.trace_rays(origins, directions)     # closest hit of the caller's own rays
    occ = scene.occluded(origins, directions, tmax)  # is the segment blocked?
    rad = scene.shade_rays(origins, directions)      # Scene::trace_ray of the caller's own rays
    rad = scene.shade_rays_lit(origins, directions, lights)  # ... with each ray's own light samples
    film = Film(scene, width, height)                # Pixel[w*h] on the GPU for the caller's samples
    film.shade_rays(origins, directions, xy)         # trace, shade and splat (Scene.cpp:51-62)
    image = film.resolve()                           # Pixel::get_color
    scene = Scene("scene.xml", smooth=True)          # <Mesh shadingMode="smooth"> honoured (HW3)
    attr = scene.hit_attributes(origins, directions, hits)  # beta, gamma, uv, both normals
    scene = Scene.create(desc, instance_mesh=..., instance_material=...,
                         instance_transform=...)      # transformed copies of the base meshes (HW3)
    scene = Scene.create(desc, vertex_uv=uv, textures=[dict(rgb8=image, ...)],
                         mesh_texture=[0, -1])        # image textures in the library's shading (HW4)
    scene = Scene("scene.xml", textured=True, images={"floor.png": image})

Rendering runs in libceng795_rt.so's gfx950 kernels; there is no CPU path.
"""
from .scene import (Scene, CameraInfo, write_png, RAY_DTYPE, HIT_DTYPE, RADIANCE_DTYPE,  # noqa: F401
                    LIGHT_SAMPLE_DTYPE, HIT_ATTR_DTYPE, pack_rays, host_leaf_objects,
                    host_vertex_normals, host_mesh_smooth, host_instance_info,
                    host_instances_xml, host_motion_info, host_motion_xml, TEX_QUERY_DTYPE,
                    host_texture_lookup, host_textures_xml)
from .film import Film  # noqa: F401
from ._lib import RTError, RT_TRAVERSAL_FAST, RT_TRAVERSAL_REFERENCE  # noqa: F401

__all__ = ["Scene", "Film", "CameraInfo", "write_png", "RTError", "RT_TRAVERSAL_FAST",
           "RT_TRAVERSAL_REFERENCE", "RAY_DTYPE", "HIT_DTYPE", "RADIANCE_DTYPE", "LIGHT_SAMPLE_DTYPE",
           "HIT_ATTR_DTYPE", "pack_rays", "host_leaf_objects", "host_vertex_normals",
           "host_mesh_smooth", "host_instance_info", "host_instances_xml",
           "host_motion_info", "host_motion_xml", "TEX_QUERY_DTYPE", "host_texture_lookup",
           "host_textures_xml"]
