// Scene assembly (host_scene.h): which kind of scene a set of descriptors denotes,
// the host build of that kind and the state derived from it; the scene files' way to the same
// descriptors; the flat scenes of the rt_host_* entries.  No HIP.
#include <algorithm>
#include <cstdio>
#include <stdexcept>

#include "host_scene.h"

namespace rt {

void check_instance_desc(const char* fn, const rt_instance_desc* in) {
  if (in && in->struct_size < sizeof(rt_instance_desc))
    throw std::invalid_argument(std::string(fn) + ": rt_instance_desc::struct_size too small");
  if (in && in->num_instances < 0)
    throw std::invalid_argument(std::string(fn) + ": num_instances < 0");
}

bool tree_deep(const HostScene& h) { return std::max(h.depth, h.accel_depth) > kLaneStack - 2; }

bool scene_entry_cuts_apply(const HostScene& h, int max_tree_depth) {
  return entry_cuts_apply(h, tree_deep(h) ? max_tree_depth : kLaneStack - 2);
}

namespace {

// The culling tree of K-leaf treelets; none when it would be deeper than the kernels' stacks.
void build_scene_accel(HostScene& h, int K, int max_tree_depth) {
  build_accel(h, K);
  if (h.accel_depth > max_tree_depth) build_accel(h, 0);
}

// The flat scene: tree, surface data, textures, culling tree; its limits and what it decides.
void assemble_flat(const SceneInputs& in, int max_tree_depth, SceneHost& out) {
  HostScene& h = out.host;
  build_host_scene(*in.desc, h);
  build_surface(*in.desc, in.surface, h);
  build_textures(*in.desc, in.surface, in.textures, h);
  build_scene_accel(h, kDefaultTreeletLeaves, max_tree_depth);
  if (h.prims.size() >= (size_t(1) << 26))  // leaf indices share a 32-bit queue word with a lane
    throw std::invalid_argument("scenes of 2^26 primitives or more are not supported");
  if (h.depth > max_tree_depth)
    throw std::invalid_argument("BVH deeper than " + std::to_string(max_tree_depth) +
                                " levels is not supported");
  out.deep = tree_deep(h);
  for (const DevPrim& p : h.prims) out.has_spheres |= p.kind == kPrimSphere;
  out.smooth = h.smooth;
  out.textured = !h.textures.empty();
}

}  // namespace

void assemble_scene(const SceneInputs& in, int max_tree_depth, SceneHost& out) {
  const std::string entry(in.entry);
  if (!in.desc) throw std::invalid_argument(entry + ": NULL argument");
  if (in.surface && in.surface->struct_size < sizeof(rt_surface_desc))
    throw std::invalid_argument(entry + ": rt_surface_desc::struct_size too small");
  check_instance_desc(in.entry, in.instances);
  const bool instanced = in.instances && in.instances->num_instances > 0;
  const bool moving = !motion_trivial(*in.desc, in.instances, in.motion);
  if (in.image_names) out.host.image_names = *in.image_names;
  if (!instanced && !moving) {
    assemble_flat(in, max_tree_depth, out);
  } else {
    if (in.surface || in.textures)
      throw std::domain_error(entry + ": instances and motion do not take surface data or textures");
    // no flat tree to cull, `deep` stays false (build_instanced refuses deeper trees)
    out.inst = std::make_unique<InstHost>();
    build_host_globals(*in.desc, out.host);
    if (moving)
      build_moving(*in.desc, in.instances, in.motion, kDefaultTreeletLeaves, *out.inst);
    else
      build_instanced(*in.desc, *in.instances, kDefaultTreeletLeaves, *out.inst);
    out.has_spheres = out.inst->has_spheres;
  }
  // what the materials and cameras decide: whether a ray tree can recurse, and the largest frame
  const HostScene& h = out.host;
  for (const DevMaterial& m : h.materials) {
    const bool mirror = m.mirror[0] != 0 || m.mirror[1] != 0 || m.mirror[2] != 0;
    const bool glass = m.transparency[0] != 0 || m.transparency[1] != 0 || m.transparency[2] != 0;
    if ((mirror || glass) && h.max_depth > 0) out.needs_recursion = true;
  }
  for (const rt_camera& c : h.cameras) {
    const size_t tiles = (size_t)((c.width + kTile - 1) / kTile) * ((c.height + kTile - 1) / kTile);
    out.most = std::max(out.most, tiles * kTile * kTile);
  }
}

void load_scene_file(const char* entry, const std::string& path, const SceneFileOptions& opt,
                     SceneFile& f) {
  f.in = SceneInputs{};
  f.in.entry = entry;
  f.in.desc = &f.desc;
  f.in.image_names = &f.st.image_names;
  if (!opt.instances) {
    load_scene_xml(path, f.st, f.desc);
  } else {
    load_instances_xml(path, f.st, f.desc, f.xi, opt.motion);
    // (no <Mesh>: an empty descriptor, rt_scene_load_xml's scene)
    f.instances = rt_instance_desc{sizeof(rt_instance_desc), (int)f.xi.mesh.size(), f.xi.mesh.data(),
                                   f.xi.material.data(), f.xi.transform.data()};
    f.in.instances = &f.instances;
  }
  if (opt.motion) {
    f.motion = rt_motion_desc{sizeof(rt_motion_desc), (int)f.xi.mesh.size(), f.desc.num_spheres,
                              f.xi.velocity.data(), f.xi.sphere_transform.data(),
                              f.xi.sphere_velocity.data()};
    f.in.motion = &f.motion;
  }
  if (opt.textures) {
    load_textures_xml(path, f.xt);
    textures_from_xml(f.xt, f.desc, opt.images, opt.num_images, f.records, f.uv, f.textures);
    f.in.textures = &f.textures;
  }
  if (opt.shading_mode || opt.textures) {  // the meshes' shadingMode, computed normals, the file's uv
    f.surface = rt_surface_desc{sizeof(rt_surface_desc), f.st.mesh_smooth.data(), nullptr,
                                opt.textures ? f.uv.data() : nullptr};
    f.in.surface = &f.surface;
  }
}

void load_flat_scene(const std::string& xml_path, HostScene& out) {
  XmlSceneStorage st;
  rt_scene_desc d;
  load_scene_xml(xml_path, st, d);
  build_host_scene(d, out);
}

void flat_host_scene(const std::string& xml_path, int treelet_leaves, int max_tree_depth,
                     long long stats4[4], HostScene& out) {
  load_flat_scene(xml_path, out);
  if (max_tree_depth > 0)
    build_scene_accel(out, treelet_leaves, max_tree_depth);
  else
    build_accel(out, treelet_leaves);
  if (!stats4) return;
  const std::string err = check_accel(out, treelet_leaves, stats4);
  if (!err.empty()) throw std::invalid_argument("culling tree: " + err);
}

bool write_text_file(const char* path, const std::string& text) {
  FILE* f = std::fopen(path, "w");
  if (!f) return false;
  std::fwrite(text.data(), 1, text.size(), f);
  std::fclose(f);
  return true;
}

}  // namespace rt
