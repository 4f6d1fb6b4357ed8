// Stand-alone host check of scene assembly, for sanitizer runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread \
//       tools/scene_assemble_check.cpp \
//       ceng795_amd/csrc/{scene_assemble,instances,instances_xml,scene_build,accel_build,entry_cuts,scene_xml,xml_dom}.cpp \
//       -o scene_assemble_check && ./scene_assemble_check [scene.xml ...]
// Builds a scene of 33 mesh triangles in two meshes, a loose triangle and a sphere and runs
// assemble_scene on it the way every creation entry does.  Inputs the header documents as
// equivalent must give scenes equal array for array and flag for flag; each bad descriptor must
// throw its documented exception type.  Every scene file named is taken by load_scene_file with
// each entry's options and compared with the same file through the loaders and hand-made
// descriptors.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ceng795_amd/csrc/host_scene.h"

using namespace rt;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const int kMaxDepth = 1024;  // the kernels' largest stack (rt_kernels.hip kDeepStack)

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same(const std::vector<std::string>& a, const std::vector<std::string>& b) { return a == b; }

static bool same_host(const HostScene& a, const HostScene& b) {
  return std::memcmp(a.background, b.background, sizeof a.background) == 0 &&
         std::memcmp(a.ambient, b.ambient, sizeof a.ambient) == 0 && a.eps == b.eps &&
         a.max_depth == b.max_depth && same(a.materials, b.materials) && same(a.lights, b.lights) &&
         same(a.cameras, b.cameras) && same(a.image_names, b.image_names) &&
         same(a.nodes, b.nodes) && same(a.prims, b.prims) && same(a.normals, b.normals) &&
         same(a.leaf_src, b.leaf_src) && same(a.leaf_object, b.leaf_object) &&
         a.root_kind == b.root_kind && a.root_ref == b.root_ref &&
         std::memcmp(a.root_box, b.root_box, sizeof a.root_box) == 0 && a.depth == b.depth &&
         a.accel_root == b.accel_root && a.accel_depth == b.accel_depth &&
         a.accel_items == b.accel_items && a.accel_stride == b.accel_stride &&
         std::memcmp(a.accel_box, b.accel_box, sizeof a.accel_box) == 0 &&
         std::memcmp(a.cull_margin, b.cull_margin, sizeof a.cull_margin) == 0 &&
         same(a.leaves, b.leaves) && same(a.ancestry, b.ancestry) && a.quot_ok == b.quot_ok &&
         a.smooth == b.smooth && same(a.leaf_tri, b.leaf_tri) &&
         same(a.vertex_normals, b.vertex_normals) && same(a.vertex_uv, b.vertex_uv) &&
         same(a.textures, b.textures) && same(a.texels, b.texels) &&
         a.blank_material == b.blank_material;
}

static bool same_inst(const InstHost& a, const InstHost& b) {
  if (a.meshes.size() != b.meshes.size()) return false;
  for (size_t m = 0; m < a.meshes.size(); m++)
    if (!same_host(a.meshes[m], b.meshes[m])) return false;
  return same(a.mesh_leaf_base, b.mesh_leaf_base) && same(a.mesh_object_base, b.mesh_object_base) &&
         same(a.accel_stats, b.accel_stats) && same(a.instances, b.instances) &&
         same(a.inverse, b.inverse) && same(a.inst_top_dfs, b.inst_top_dfs) &&
         same(a.top_nodes, b.top_nodes) && same(a.top_prims, b.top_prims) &&
         same(a.top_normals, b.top_normals) && same(a.top_info, b.top_info) &&
         a.top_root_kind == b.top_root_kind && a.top_depth == b.top_depth &&
         a.top_quot_ok == b.top_quot_ok && std::memcmp(a.top_box, b.top_box, sizeof a.top_box) == 0 &&
         a.has_spheres == b.has_spheres && a.leaves == b.leaves && a.has_motion == b.has_motion &&
         same(a.motion_instances, b.motion_instances) && same(a.motion_spheres, b.motion_spheres) &&
         same(a.sphere_inverse, b.sphere_inverse) && same(a.sphere_box, b.sphere_box) &&
         same(a.object_top_dfs, b.object_top_dfs);
}

static bool same_scene(const SceneHost& a, const SceneHost& b) {
  if (!same_host(a.host, b.host) || !a.inst != !b.inst) return false;
  if (a.inst && !same_inst(*a.inst, *b.inst)) return false;
  return a.deep == b.deep && a.needs_recursion == b.needs_recursion &&
         a.has_spheres == b.has_spheres && a.smooth == b.smooth && a.textured == b.textured &&
         a.most == b.most;
}

struct Geometry {
  std::vector<float> verts, uv;
  std::vector<int> faces, counts, tri, sphere_center, zero;
  std::vector<float> radius;
  std::vector<unsigned char> smooth;
  rt_material materials[2];
  rt_point_light light;
  rt_camera camera;
  rt_scene_desc desc;
};

static void make_geometry(Geometry& g) {
  const int n = 5;  // 32 faces
  for (int j = 0; j < n; j++)
    for (int i = 0; i < n; i++) {
      const float x = -1 + 2.0f * i / (n - 1), y = -1 + 2.0f * j / (n - 1);
      g.verts.insert(g.verts.end(), {x, y, 0.3f * std::sin(3 * x + 5 * y)});
    }
  for (int j = 0; j + 1 < n; j++)
    for (int i = 0; i + 1 < n; i++) {
      const int a = j * n + i, b = a + 1, c = a + n, e = c + 1;
      g.faces.insert(g.faces.end(), {a, b, e, a, e, c});
    }
  g.counts.push_back((int)g.faces.size() / 3);
  const int base = (int)g.verts.size() / 3;
  g.verts.insert(g.verts.end(), {-0.5f, -0.5f, 0, 0.5f, -0.5f, 0.1f, 0, 0.6f, 0.2f,
                                 -3, -2, -1, -2, -2, -1.2f, -2.5f, -1, -0.8f, 2.5f, -1.5f, -0.5f});
  g.faces.insert(g.faces.end(), {base, base + 1, base + 2});
  g.counts.push_back(1);
  g.tri = {base + 3, base + 4, base + 5};
  g.sphere_center = {base + 6};
  g.radius = {0.6f};
  g.zero = {0, 0};
  g.smooth = {1, 0};
  for (size_t v = 0; v < g.verts.size() / 3; v++)
    g.uv.insert(g.uv.end(), {0.5f + 0.25f * g.verts[3 * v], 0.5f + 0.25f * g.verts[3 * v + 1]});
  std::memset(g.materials, 0, sizeof g.materials);
  g.materials[0].diffuse[0] = 0.5f;
  g.materials[1].mirror[1] = 0.25f;  // the scene recurses
  const float pos[3] = {0, 0, 5}, gaze[3] = {0, 0, -1}, up[3] = {0, 1, 0}, np[4] = {-1, 1, -1, 1};
  camera_from_view(pos, gaze, up, np, 1.0f, 40, 24, 1, g.camera);
  g.light = rt_point_light{{0, 3, 4}, {100, 100, 100}};
  std::memset(&g.desc, 0, sizeof g.desc);
  rt_scene_desc& d = g.desc;
  d.shadow_ray_epsilon = 0.001f;
  d.max_recursion_depth = 2;
  d.vertices = g.verts.data();
  d.num_vertices = (int)g.verts.size() / 3;
  d.materials = g.materials;
  d.num_materials = 2;
  d.lights = &g.light;
  d.num_lights = 1;
  d.cameras = &g.camera;
  d.num_cameras = 1;
  d.num_meshes = 2;
  d.mesh_material = g.zero.data();
  d.mesh_face_count = g.counts.data();
  d.mesh_faces = g.faces.data();
  d.num_triangles = 1;
  d.triangle_indices = g.tri.data();
  d.triangle_material = g.zero.data();
  d.num_spheres = 1;
  d.sphere_center = g.sphere_center.data();
  d.sphere_radius = g.radius.data();
  d.sphere_material = g.zero.data();
}

static SceneInputs inputs(const char* entry, const rt_scene_desc* d, const rt_surface_desc* su = nullptr,
                          const rt_texture_desc* tx = nullptr, const rt_instance_desc* in = nullptr,
                          const rt_motion_desc* mo = nullptr) {
  SceneInputs s;
  s.entry = entry;
  s.desc = d;
  s.surface = su;
  s.textures = tx;
  s.instances = in;
  s.motion = mo;
  return s;
}

// 0: no exception, 1: std::invalid_argument, 2: std::domain_error, 3: anything else; `what` gets
// the message.
static int thrown(const SceneInputs& in, int max_depth, std::string* what = nullptr) {
  SceneHost s;
  try {
    assemble_scene(in, max_depth, s);
  } catch (const std::domain_error& e) {
    if (what) *what = e.what();
    return 2;
  } catch (const std::invalid_argument& e) {
    if (what) *what = e.what();
    return 1;
  } catch (const std::exception& e) {
    if (what) *what = e.what();
    return 3;
  }
  return 0;
}

static void check_equivalences(Geometry& g) {
  const rt_scene_desc* d = &g.desc;
  SceneHost plain;
  assemble_scene(inputs("rt_scene_create", d), kMaxDepth, plain);
  EXPECT(!plain.inst && plain.host.prims.size() == 35 && plain.has_spheres && plain.needs_recursion);
  const size_t tiles = (size_t)((40 + kTile - 1) / kTile) * ((24 + kTile - 1) / kTile);
  EXPECT(!plain.smooth && !plain.textured && !plain.deep && plain.most == tiles * kTile * kTile);
  EXPECT(plain.host.accel_root >= 0 && plain.host.image_names.size() == 1);

  {  // a NULL surface descriptor, and one that says nothing
    SceneHost a, b;
    assemble_scene(inputs("rt_scene_create_surface", d, nullptr), kMaxDepth, a);
    const unsigned char flat[2] = {0, 0};
    const rt_surface_desc none{sizeof(rt_surface_desc), flat, nullptr, nullptr};
    assemble_scene(inputs("rt_scene_create_surface", d, &none), kMaxDepth, b);
    EXPECT(same_scene(plain, a) && same_scene(plain, b));
  }
  {  // a NULL or empty instance descriptor
    SceneHost a, b;
    assemble_scene(inputs("rt_scene_create_instanced", d, nullptr, nullptr, nullptr), kMaxDepth, a);
    const rt_instance_desc empty{sizeof(rt_instance_desc), 0, nullptr, nullptr, nullptr};
    assemble_scene(inputs("rt_scene_create_instanced", d, nullptr, nullptr, &empty), kMaxDepth, b);
    EXPECT(same_scene(plain, a) && same_scene(plain, b));
  }
  const std::vector<int> mesh{0, 0, 1}, mat{0, 1, 0};
  const std::vector<float> xf{1, 0, 0, 0,    0, 1, 0, 0,    0, 0, 1, 0,     0, 0, 0, 1,
                              0.5f, 0, 0, 3, 0, 2, 0, 0.5f, 0, 0, -1, 0.2f, 0, 0, 0, 1,
                              1, 0, 0, -2,   0, 1, 0, 1,    0, 0, 1, 0,     0, 0, 0, 1};
  const rt_instance_desc in{sizeof(rt_instance_desc), 3, mesh.data(), mat.data(), xf.data()};
  const std::vector<float> zero3(9, 0.0f), identity{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  {  // trivial motion: none, all NULL, all zero with identity matrices — without instances ...
    const rt_motion_desc nulls{sizeof(rt_motion_desc), 0, 0, nullptr, nullptr, nullptr};
    const rt_motion_desc zeros{sizeof(rt_motion_desc), 0, 1, nullptr, identity.data(), zero3.data()};
    SceneHost a, b, c;
    assemble_scene(inputs("rt_scene_create_moving", d, nullptr, nullptr, nullptr, nullptr), kMaxDepth, a);
    assemble_scene(inputs("rt_scene_create_moving", d, nullptr, nullptr, nullptr, &nulls), kMaxDepth, b);
    assemble_scene(inputs("rt_scene_create_moving", d, nullptr, nullptr, nullptr, &zeros), kMaxDepth, c);
    EXPECT(same_scene(plain, a) && same_scene(plain, b) && same_scene(plain, c));
  }
  {  // ... and with them: rt_scene_create_instanced's scene
    const rt_motion_desc zeros{sizeof(rt_motion_desc), 3, 1, zero3.data(), identity.data(), zero3.data()};
    SceneHost two, a, b;
    assemble_scene(inputs("rt_scene_create_instanced", d, nullptr, nullptr, &in), kMaxDepth, two);
    assemble_scene(inputs("rt_scene_create_moving", d, nullptr, nullptr, &in, nullptr), kMaxDepth, a);
    assemble_scene(inputs("rt_scene_create_moving", d, nullptr, nullptr, &in, &zeros), kMaxDepth, b);
    EXPECT(two.inst && two.inst->instances.size() == 3 && !two.inst->has_motion && !two.deep);
    EXPECT(two.host.prims.empty() && two.has_spheres && two.needs_recursion && two.most == plain.most);
    EXPECT(same_scene(two, a) && same_scene(two, b) && !same_scene(two, plain));
    // a velocity: the scene with motion, another one
    std::vector<float> vel(9, 0.0f);
    vel[4] = 0.5f;
    const rt_motion_desc moves{sizeof(rt_motion_desc), 3, 0, vel.data(), nullptr, nullptr};
    SceneHost m;
    assemble_scene(inputs("rt_scene_create_moving", d, nullptr, nullptr, &in, &moves), kMaxDepth, m);
    EXPECT(m.inst && m.inst->has_motion && !same_scene(two, m));
    // ... and a moving sphere without any instance: a top level of the loose primitives
    vel.assign(3, 0.0f);
    vel[0] = 1.0f;
    const rt_motion_desc sphere{sizeof(rt_motion_desc), 0, 1, nullptr, nullptr, vel.data()};
    SceneHost ms;
    assemble_scene(inputs("rt_scene_create_moving", d, nullptr, nullptr, nullptr, &sphere), kMaxDepth, ms);
    EXPECT(ms.inst && ms.inst->has_motion && ms.inst->instances.empty());
  }
  {  // textures that no object names: the surface scene
    const rt_surface_desc su{sizeof(rt_surface_desc), g.smooth.data(), nullptr, g.uv.data()};
    const unsigned char texels[12] = {255, 0, 0, 0, 255, 0, 0, 0, 255, 9, 9, 9};
    const rt_texture t{texels, 2, 2, RT_TEX_BILINEAR, RT_TEX_BLEND_KD, RT_TEX_CLAMP, 255.0f};
    const int none[2] = {-1, -1};
    const rt_texture_desc unused{sizeof(rt_texture_desc), 1, &t, none, none, none};
    SceneHost surf, a, b;
    assemble_scene(inputs("rt_scene_create_surface", d, &su), kMaxDepth, surf);
    assemble_scene(inputs("rt_scene_create_textured", d, &su, &unused), kMaxDepth, a);
    assemble_scene(inputs("rt_scene_create_textured", d, &su, nullptr), kMaxDepth, b);
    EXPECT(surf.smooth && !surf.textured && !surf.host.vertex_uv.empty() && !same_scene(plain, surf));
    EXPECT(same_scene(surf, a) && same_scene(surf, b));
    const int first[2] = {0, -1};
    const rt_texture_desc used{sizeof(rt_texture_desc), 1, &t, first, none, none};
    SceneHost tex;
    assemble_scene(inputs("rt_scene_create_textured", d, &su, &used), kMaxDepth, tex);
    EXPECT(tex.textured && tex.smooth && tex.host.textures.size() == 1 && !same_scene(surf, tex));
  }
  {  // a tree deeper than the kernels' culling stack: the scene without a culling tree
    SceneHost a;
    assemble_scene(inputs("rt_scene_create", d), plain.host.depth, a);
    EXPECT(plain.host.accel_depth <= plain.host.depth || a.host.accel_root < 0);
  }
}

static void check_refusals(Geometry& g) {
  const rt_scene_desc* d = &g.desc;
  std::string what;
  const std::vector<int> mesh{0}, mat{0};
  std::vector<float> xf{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rt_instance_desc in{sizeof(rt_instance_desc), 1, mesh.data(), mat.data(), xf.data()};
  rt_surface_desc su{sizeof(rt_surface_desc), g.smooth.data(), nullptr, nullptr};

  EXPECT(thrown(inputs("rt_scene_create", nullptr), kMaxDepth) == 1);
  su.struct_size = 8;
  EXPECT(thrown(inputs("rt_scene_create_surface", d, &su), kMaxDepth, &what) == 1);
  EXPECT(what == "rt_scene_create_surface: rt_surface_desc::struct_size too small");
  EXPECT(thrown(inputs("rt_scene_create_textured", d, &su), kMaxDepth, &what) == 1);
  EXPECT(what == "rt_scene_create_textured: rt_surface_desc::struct_size too small");
  su.struct_size = sizeof su;

  in.struct_size = 8;
  EXPECT(thrown(inputs("rt_scene_create_instanced", d, nullptr, nullptr, &in), kMaxDepth, &what) == 1);
  EXPECT(what == "rt_scene_create_instanced: rt_instance_desc::struct_size too small");
  in.struct_size = sizeof in;
  in.num_instances = -1;
  EXPECT(thrown(inputs("rt_scene_create_moving", d, nullptr, nullptr, &in), kMaxDepth, &what) == 1);
  EXPECT(what == "rt_scene_create_moving: num_instances < 0");
  in.num_instances = 1;

  rt_motion_desc mo{8, 0, 0, nullptr, nullptr, nullptr};
  EXPECT(thrown(inputs("rt_scene_create_moving", d, nullptr, nullptr, &in, &mo), kMaxDepth) == 1);
  mo = rt_motion_desc{sizeof(rt_motion_desc), 2, 0, nullptr, nullptr, nullptr};
  const std::vector<float> vel(6, 0.0f);
  mo.instance_velocity = vel.data();  // a count that differs from the instance descriptor's
  EXPECT(thrown(inputs("rt_scene_create_moving", d, nullptr, nullptr, &in, &mo), kMaxDepth) == 1);

  xf[0] = 0;  // a singular matrix
  EXPECT(thrown(inputs("rt_scene_create_instanced", d, nullptr, nullptr, &in), kMaxDepth) == 1);
  xf[0] = 1;
  EXPECT(thrown(inputs("rt_scene_create_instanced", d, nullptr, nullptr, &in), kMaxDepth) == 0);

  // what no entry can express: instances or motion with surface data or textures
  EXPECT(thrown(inputs("rt_scene_create_instanced", d, &su, nullptr, &in), kMaxDepth) == 2);
  const rt_texture_desc empty{sizeof(rt_texture_desc), 0, nullptr, nullptr, nullptr, nullptr};
  EXPECT(thrown(inputs("rt_scene_create_instanced", d, nullptr, &empty, &in), kMaxDepth) == 2);

  {  // the caller's own tree: not with instances
    rt_scene_desc own = g.desc;
    own.bvh_num_leaves = 1;
    EXPECT(thrown(inputs("rt_scene_create_instanced", &own, nullptr, nullptr, &in), kMaxDepth) == 2);
  }
  {  // a texture id out of range, a textured mesh without uv
    const unsigned char texels[3] = {1, 2, 3};
    const rt_texture t{texels, 1, 1, RT_TEX_NEAREST, RT_TEX_REPLACE_KD, RT_TEX_REPEAT, 255.0f};
    const int bad[2] = {1, -1}, first[2] = {0, -1};
    rt_texture_desc tx{sizeof(rt_texture_desc), 1, &t, bad, nullptr, nullptr};
    EXPECT(thrown(inputs("rt_scene_create_textured", d, nullptr, &tx), kMaxDepth) == 1);
    tx.mesh_texture = first;
    EXPECT(thrown(inputs("rt_scene_create_textured", d, nullptr, &tx), kMaxDepth) == 1);
    tx.struct_size = 8;
    EXPECT(thrown(inputs("rt_scene_create_textured", d, &su, &tx), kMaxDepth) == 1);
  }
  {  // the description itself, through every kind of entry
    std::vector<int> faces = g.faces;
    faces[0] = g.desc.num_vertices;
    rt_scene_desc bad = g.desc;
    bad.mesh_faces = faces.data();
    EXPECT(thrown(inputs("rt_scene_create", &bad), kMaxDepth, &what) == 1);
    EXPECT(what == "vertex index out of range");
    EXPECT(thrown(inputs("rt_scene_create_surface", &bad, &su), kMaxDepth) == 1);
    EXPECT(thrown(inputs("rt_scene_create_instanced", &bad, nullptr, nullptr, &in), kMaxDepth) == 1);
    bad = g.desc;
    bad.max_recursion_depth = -1;
    EXPECT(thrown(inputs("rt_scene_create_instanced", &bad, nullptr, nullptr, &in), kMaxDepth) == 1);
  }
  // a reference tree deeper than the kernels take
  EXPECT(thrown(inputs("rt_scene_create", d), 1, &what) == 1);
  EXPECT(what == "BVH deeper than 1 levels is not supported");
}

// One scene file with the options of one scene-file entry, against the loaders and a hand-made
// set of descriptors.
static void check_file(const char* path, bool shading, bool instances, bool motion) {
  SceneHost a, b;
  try {
    SceneFileOptions opt;
    opt.shading_mode = shading;
    opt.instances = instances;
    opt.motion = motion;
    SceneFile f;
    load_scene_file("file", path, opt, f);
    assemble_scene(f.in, kMaxDepth, a);
  } catch (const std::exception& e) {
    std::printf("%s (%d%d%d): refused: %s\n", path, shading, instances, motion, e.what());
    return;
  }
  XmlSceneStorage st;
  XmlInstances xi;
  rt_scene_desc d;
  if (instances)
    load_instances_xml(path, st, d, xi, motion);
  else
    load_scene_xml(path, st, d);
  const rt_surface_desc su{sizeof(rt_surface_desc), st.mesh_smooth.data(), nullptr, nullptr};
  const rt_instance_desc in{sizeof(rt_instance_desc), (int)xi.mesh.size(), xi.mesh.data(),
                            xi.material.data(), xi.transform.data()};
  const rt_motion_desc mo{sizeof(rt_motion_desc), (int)xi.mesh.size(), d.num_spheres,
                          xi.velocity.data(), xi.sphere_transform.data(), xi.sphere_velocity.data()};
  SceneInputs s = inputs("desc", &d, shading ? &su : nullptr, nullptr, instances ? &in : nullptr,
                         motion ? &mo : nullptr);
  s.image_names = &st.image_names;
  assemble_scene(s, kMaxDepth, b);
  EXPECT(same_scene(a, b));
  std::printf("%s (%d%d%d): %zu leaves, %zu instances%s\n", path, shading, instances, motion,
              a.host.prims.size(), a.inst ? a.inst->instances.size() : (size_t)0,
              a.inst && a.inst->has_motion ? ", motion" : "");
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {
    check_file(argv[i], false, false, false);
    check_file(argv[i], true, false, false);
    check_file(argv[i], false, true, false);
    check_file(argv[i], false, true, true);
    // the rt_host_* entries' flat scene: the tree creation builds
    try {
      SceneFile f;
      load_scene_file("file", argv[i], SceneFileOptions{}, f);
      SceneHost s;
      assemble_scene(f.in, kMaxDepth, s);
      HostScene h;
      long long stats[4];
      flat_host_scene(argv[i], kDefaultTreeletLeaves, kMaxDepth, stats, h);
      h.image_names = s.host.image_names;
      EXPECT(same_host(s.host, h) && s.deep == tree_deep(h));
    } catch (const std::exception& e) {
      std::printf("%s: refused: %s\n", argv[i], e.what());
    }
  }
  Geometry g;
  make_geometry(g);
  check_equivalences(g);
  check_refusals(g);
  EXPECT(!write_text_file("/nonexistent-directory/x.txt", "x"));
  std::printf(failures ? "scene_assemble_check: %d FAILED\n" : "scene_assemble_check: ok\n", failures);
  return failures ? 1 : 0;
}
