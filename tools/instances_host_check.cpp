// Stand-alone host check of the instanced scene build, for sanitizer runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread \
//       tools/instances_host_check.cpp \
//       ceng795_amd/csrc/{instances,instances_xml,scene_build,accel_build,scene_xml,xml_dom}.cpp \
//       -o instances_host_check && ./instances_host_check [scene.xml ...]
// Every scene file named is loaded with its instances (load_instances_xml) and built as well.
// Builds scenes like the tests' (a height field instanced with identity, a composed and a
// mirrored matrix, a one-face mesh, loose primitives; a single instance; a singular matrix; a
// top-level tree that is too deep) and checks the sizes and links of what comes out.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../ceng795_amd/csrc/host_scene.h"

using namespace rt;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Geometry {
  std::vector<float> verts;
  std::vector<int> faces, counts, tri, sphere_center, zero;
  std::vector<float> radius;
  rt_material material;
  rt_scene_desc desc;
};

static void make_geometry(Geometry& g, int n, bool loose) {
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
  std::memset(&g.material, 0, sizeof g.material);
  std::memset(&g.desc, 0, sizeof g.desc);
  rt_scene_desc& d = g.desc;
  d.vertices = g.verts.data();
  d.num_vertices = (int)g.verts.size() / 3;
  d.materials = &g.material;
  d.num_materials = 1;
  d.num_meshes = 2;
  d.mesh_material = g.zero.data();
  d.mesh_face_count = g.counts.data();
  d.mesh_faces = g.faces.data();
  if (loose) {
    d.num_triangles = 1;
    d.triangle_indices = g.tri.data();
    d.triangle_material = g.zero.data();
    d.num_spheres = 1;
    d.sphere_center = g.sphere_center.data();
    d.sphere_radius = g.radius.data();
    d.sphere_material = g.zero.data();
  }
}

static std::vector<float> matrix(float sx, float sy, float sz, float tx, float ty, float tz, float deg) {
  const float c = std::cos(deg * 3.14159265f / 180), s = std::sin(deg * 3.14159265f / 180);
  return {c * sx, -s * sy, 0, tx, s * sx, c * sy, 0, ty, 0, 0, sz, tz, 0, 0, 0, 1};
}

static rt_instance_desc instances_of(const std::vector<int>& mesh, const std::vector<int>& mat,
                                     const std::vector<float>& xf) {
  rt_instance_desc in;
  in.struct_size = sizeof in;
  in.num_instances = (int)mesh.size();
  in.instance_mesh = mesh.data();
  in.instance_material = mat.data();
  in.instance_transform = xf.data();
  return in;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {  // scene files: the XML ingest, then the same build
    XmlSceneStorage st;
    XmlInstances xi;
    rt_scene_desc d;
    try {
      load_instances_xml(argv[i], st, d, xi);
      const rt_instance_desc in = instances_of(xi.mesh, xi.material, xi.transform);
      InstHost ih;
      build_instanced(d, in, kDefaultTreeletLeaves, ih);
      std::printf("%s: %zu instances of %zu meshes, %zu top-level objects\n", argv[i],
                  ih.instances.size(), ih.meshes.size(), ih.top_prims.size());
      EXPECT(ih.instances.size() == xi.mesh.size());
    } catch (const std::exception& e) {
      std::printf("%s: refused: %s\n", argv[i], e.what());
    }
  }
  {  // "three": every kind of object
    Geometry g;
    make_geometry(g, 6, true);
    std::vector<int> mesh{0, 0, 0, 1}, mat{0, 0, 0, 0};
    std::vector<float> xf;
    for (auto m : {matrix(1, 1, 1, 0, 0, 0, 0), matrix(0.7f, 1.3f, 0.9f, 2.5f, 1, -0.5f, 30),
                   matrix(-1, 1, 1.2f, -2.5f, 1.2f, 0.3f, 0), matrix(1, 1, 1, 0.3f, -2.2f, 0.8f, 0)})
      xf.insert(xf.end(), m.begin(), m.end());
    const rt_instance_desc in = instances_of(mesh, mat, xf);
    InstHost ih;
    build_instanced(g.desc, in, kDefaultTreeletLeaves, ih);
    EXPECT(ih.instances.size() == 4 && ih.meshes.size() == 2);
    EXPECT(ih.top_prims.size() == 6 && ih.top_nodes.size() == 5 && ih.top_root_kind == kTopNode);
    EXPECT(ih.meshes[0].prims.size() == 50 && ih.meshes[1].root_kind == kRootTriangle);
    EXPECT(ih.leaves == 53 && ih.has_spheres);
    std::vector<char> seen(6, 0);
    for (int p : ih.inst_top_dfs) {
      EXPECT(p >= 0 && p < 6 && ih.top_prims[(size_t)p].kind == kPrimInstance);
      seen[(size_t)p] = 1;
    }
    for (size_t p = 0; p < 6; p++)
      if (!seen[p]) EXPECT(ih.top_prims[p].kind != kPrimInstance && ih.top_info[2 * p] >= 51);
    for (const DevNode& nd : ih.top_nodes)
      for (int s = 0; s < 2; s++)
        EXPECT(nd.child[s] >= 0 ? nd.child[s] < 5 : ~nd.child[s] < 6);
  }
  {  // a single instance; larger mesh (culling tree with inner nodes)
    Geometry g;
    make_geometry(g, 40, false);
    std::vector<int> mesh{0}, mat{0};
    std::vector<float> xf = matrix(0.7f, 1.3f, 0.9f, 2.5f, 1, -0.5f, 30);
    const rt_instance_desc in = instances_of(mesh, mat, xf);
    InstHost ih;
    build_instanced(g.desc, in, kDefaultTreeletLeaves, ih);
    EXPECT(ih.top_root_kind == kTopSingle && ih.top_prims.size() == 1 && ih.top_nodes.empty());
    EXPECT(ih.meshes[0].accel_root >= 0 && ih.meshes[0].prims.size() == 2 * 39 * 39);
  }
  {  // refused: a singular matrix, a mesh id out of range, a tree too deep
    Geometry g;
    make_geometry(g, 4, true);
    std::vector<int> mesh{0}, mat{0};
    std::vector<float> xf = matrix(1, 0, 1, 0, 0, 0, 0);
    InstHost ih;
    bool threw = false;
    try {
      build_instanced(g.desc, instances_of(mesh, mat, xf), kDefaultTreeletLeaves, ih);
    } catch (const std::invalid_argument&) { threw = true; }
    EXPECT(threw);
    mesh[0] = 2;
    xf = matrix(1, 1, 1, 0, 0, 0, 0);
    threw = false;
    try {
      build_instanced(g.desc, instances_of(mesh, mat, xf), kDefaultTreeletLeaves, ih);
    } catch (const std::invalid_argument&) { threw = true; }
    EXPECT(threw);
    std::vector<int> many(71, 1), mats(71, 0);
    std::vector<float> xfs;
    for (int k = 0; k < 71; k++) {
      const float s = std::ldexp(1.0f, 35 - k);
      const auto m = matrix(s, s, s, s, s, s, 0);
      xfs.insert(xfs.end(), m.begin(), m.end());
    }
    threw = false;
    try {
      build_instanced(g.desc, instances_of(many, mats, xfs), kDefaultTreeletLeaves, ih);
    } catch (const std::domain_error&) { threw = true; }
    EXPECT(threw);
  }
  std::printf(failures ? "instances_host_check: %d FAILED\n" : "instances_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
