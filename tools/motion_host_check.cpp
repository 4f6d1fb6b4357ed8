// Stand-alone host check of the build of scenes with motion, for sanitizer runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread \
//       tools/motion_host_check.cpp \
//       ceng795_amd/csrc/{instances,instances_xml,scene_build,accel_build,scene_xml,xml_dom}.cpp \
//       -o motion_host_check && ./motion_host_check [scene.xml ...]
// Every scene file named is loaded with its motion (load_instances_xml(..., true)) and built.
// Exercises the descriptor checks, the expanded boxes, the sphere inverses, the top-level kinds
// and motion_inverse (the walk's per-ray inverse, compiled here for the host) against mat4.h.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "../ceng795_amd/csrc/host_scene.h"
#include "../ceng795_amd/csrc/mat4.h"

using namespace rt;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Geometry {
  std::vector<float> verts, radius;
  std::vector<int> faces, counts, tri, sphere_center, zero;
  rt_material material;
  rt_scene_desc desc;
};

static void make_geometry(Geometry& g, int n) {
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
  g.verts.insert(g.verts.end(), {-3, -2, -1, -2, -2, -1.2f, -2.5f, -1, -0.8f, 2.5f, -1.5f, -0.5f,
                                 -0.8f, 2.4f, 0.6f, 1.2f, -2.6f, 0.9f});
  g.tri = {base, base + 1, base + 2};
  g.sphere_center = {base + 3, base + 4, base + 5};
  g.radius = {0.6f, 0.5f, 0.45f};
  g.zero = {0, 0, 0};
  std::memset(&g.material, 0, sizeof g.material);
  std::memset(&g.desc, 0, sizeof g.desc);
  rt_scene_desc& d = g.desc;
  d.vertices = g.verts.data();
  d.num_vertices = (int)g.verts.size() / 3;
  d.materials = &g.material;
  d.num_materials = 1;
  d.num_meshes = 1;
  d.mesh_material = g.zero.data();
  d.mesh_face_count = g.counts.data();
  d.mesh_faces = g.faces.data();
  d.num_triangles = 1;
  d.triangle_indices = g.tri.data();
  d.triangle_material = g.zero.data();
  d.num_spheres = 3;
  d.sphere_center = g.sphere_center.data();
  d.sphere_radius = g.radius.data();
  d.sphere_material = g.zero.data();
}

static std::vector<float> matrix(float sx, float sy, float sz, float tx, float ty, float tz, float deg) {
  const float c = std::cos(deg * 3.14159265f / 180), s = std::sin(deg * 3.14159265f / 180);
  return {c * sx, -s * sy, 0, tx, s * sx, c * sy, 0, ty, 0, 0, sz, tz, 0, 0, 0, 1};
}

template <typename E, typename F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const E&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++) {  // scene files: the XML ingest with motion, then the same build
    XmlSceneStorage st;
    XmlInstances xi;
    rt_scene_desc d;
    try {
      load_instances_xml(argv[i], st, d, xi, true);
      const rt_instance_desc in{sizeof(rt_instance_desc), (int)xi.mesh.size(), xi.mesh.data(),
                                xi.material.data(), xi.transform.data()};
      const rt_motion_desc mo{sizeof(rt_motion_desc), (int)xi.mesh.size(), d.num_spheres,
                              xi.velocity.data(), xi.sphere_transform.data(), xi.sphere_velocity.data()};
      EXPECT(xi.velocity.size() == 3 * xi.mesh.size());
      EXPECT(xi.sphere_transform.size() == 16 * (size_t)d.num_spheres);
      EXPECT(xi.sphere_velocity.size() == 3 * (size_t)d.num_spheres);
      InstHost ih;
      build_moving(d, &in, &mo, kDefaultTreeletLeaves, ih);
      std::printf("%s: %zu instances, %zu top-level objects, %zu moving-sphere records, motion %d\n",
                  argv[i], ih.instances.size(), ih.top_prims.size(), ih.motion_spheres.size(),
                  (int)ih.has_motion);
    } catch (const std::exception& e) {
      std::printf("%s: refused: %s\n", argv[i], e.what());
    }
  }
  Geometry g;
  make_geometry(g, 6);
  std::vector<int> mesh{0, 0, 0}, mat{0, 0, 0};
  std::vector<float> xf;
  for (auto m : {matrix(1, 1, 1, 0, 0, 0, 0), matrix(0.7f, 1.3f, 0.9f, 2.5f, 1, -0.5f, 30),
                 matrix(-1, 1, 1.2f, -2.5f, 1.2f, 0.3f, 0)})
    xf.insert(xf.end(), m.begin(), m.end());
  const rt_instance_desc in{sizeof(rt_instance_desc), 3, mesh.data(), mat.data(), xf.data()};
  std::vector<float> vel{0, 0, 0, 0.8f, -0.5f, 0.3f, -0.0f, -0.0f, -0.0f};
  std::vector<float> sxf;
  for (auto m : {matrix(1, 1, 1, 0, 0, 0, 0), matrix(1, 1, 1, 0, 0, 0, 0), matrix(1.4f, 0.6f, 0.8f, 0.4f, -0.3f, 0.2f, 20)})
    sxf.insert(sxf.end(), m.begin(), m.end());
  std::vector<float> svel{0, 0, 0, 0.6f, 0.9f, -0.4f, 0, 0, 0};
  rt_motion_desc mo{sizeof(rt_motion_desc), 3, 3, vel.data(), sxf.data(), svel.data()};
  {  // every kind of object; boxes, records, kinds
    InstHost ih, still;
    build_moving(g.desc, &in, &mo, kDefaultTreeletLeaves, ih);
    build_instanced(g.desc, in, kDefaultTreeletLeaves, still);
    EXPECT(ih.has_motion && !still.has_motion && !motion_trivial(g.desc, &in, &mo));
    EXPECT(ih.motion_instances.size() == 3 && ih.motion_spheres.size() == 2);
    EXPECT(ih.instances[1].moving == 1 && ih.instances[0].moving == 0 && ih.instances[2].moving == 0);
    EXPECT(ih.top_prims.size() == 7 && ih.object_top_dfs.size() == 7 && ih.sphere_box.size() == 18);
    for (int a = 0; a < 3; a++) {  // expanded by +-v; the others as the instanced build has them
      EXPECT(ih.instances[1].box[a] == still.instances[1].box[a] - std::fabs(vel[3 + a]));
      EXPECT(ih.instances[1].box[a + 3] == still.instances[1].box[a + 3] + std::fabs(vel[3 + a]));
    }
    EXPECT(std::memcmp(ih.instances[0].box, still.instances[0].box, 24) == 0);
    EXPECT(std::memcmp(ih.instances[2].box, still.instances[2].box, 24) == 0);  // -0 is no velocity
    int kinds[4] = {0, 0, 0, 0};
    for (const DevPrim& p : ih.top_prims) kinds[p.kind]++;
    EXPECT(kinds[kPrimInstance] == 3 && kinds[kPrimTriangle] == 1 && kinds[kPrimSphere] == 1 &&
           kinds[kPrimMovingSphere] == 2);
    for (const DevPrim& p : ih.top_prims)
      if (p.kind == kPrimMovingSphere) EXPECT(p.material >= 0 && p.material < 2);
    EXPECT(ih.motion_spheres[0].moving == 1 && ih.motion_spheres[1].moving == 0);
    // the placed sphere's inverse is Mat4::inverse of its matrix
    Mat4 m, inv;
    std::memcpy(m.a, &sxf[32], sizeof m.a);
    EXPECT(m.inverse(inv) && std::memcmp(inv.a, &ih.sphere_inverse[32], 64) == 0);
    EXPECT(std::memcmp(inv.a, ih.motion_spheres[1].inv, 48) == 0);
    // motion_inverse = Mat4's product and inverse, rows 0..2, at several times
    for (float tau : {0.0f, 0.37f, -1.0f, 1.5f, -0.0f, 3e5f}) {
      Mat4 t = Mat4::identity(), f;
      std::memcpy(f.a, &xf[16], sizeof f.a);
      for (int a = 0; a < 3; a++) t.a[a][3] = tau * vel[3 + a];
      Mat4 want;
      float got[12];
      EXPECT((t * f).inverse(want) && motion_inverse(&xf[16], &vel[3], tau, got));
      EXPECT(std::memcmp(got, want.a, sizeof got) == 0);
    }
    // a per-ray determinant of exactly 0 under an invertible matrix (tests/motion_util.py)
    float p[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1}, v[3] = {33554432.0f, 0, 0}, got[12];
    EXPECT(motion_inverse(p, v, 0.25f, got) && !motion_inverse(p, v, 0.5f, got) && std::isnan(got[0]));
  }
  {  // trivial descriptors; no instances at all
    rt_motion_desc none{sizeof(rt_motion_desc), 0, 0, nullptr, nullptr, nullptr};
    EXPECT(motion_trivial(g.desc, &in, nullptr) && motion_trivial(g.desc, &in, &none));
    std::vector<float> zeros(9, 0.0f);
    rt_motion_desc zero{sizeof(rt_motion_desc), 3, 3, zeros.data(), nullptr, zeros.data()};
    EXPECT(motion_trivial(g.desc, &in, &zero));
    InstHost ih;
    rt_motion_desc loose{sizeof(rt_motion_desc), 0, 3, nullptr, sxf.data(), svel.data()};
    build_moving(g.desc, nullptr, &loose, kDefaultTreeletLeaves, ih);
    EXPECT(ih.instances.empty() && ih.top_prims.size() == 4 && ih.has_motion && ih.meshes.size() == 1);
  }
  {  // refused
    InstHost ih;
    auto build = [&](rt_motion_desc m) { build_moving(g.desc, &in, &m, kDefaultTreeletLeaves, ih); };
    rt_motion_desc bad = mo;
    bad.struct_size = 16;
    EXPECT(throws<std::invalid_argument>([&] { build(bad); }));
    bad = mo;
    bad.num_instances = 2;
    EXPECT(throws<std::invalid_argument>([&] { build(bad); }));
    bad = mo;
    bad.num_spheres = 0;
    EXPECT(throws<std::invalid_argument>([&] { build(bad); }));
    std::vector<float> nanv = vel;
    nanv[4] = std::numeric_limits<float>::quiet_NaN();
    bad = mo;
    bad.instance_velocity = nanv.data();
    EXPECT(throws<std::invalid_argument>([&] { build(bad); }));
    std::vector<float> sing = sxf;
    sing[16 + 5] = 0.0f;  // sphere 1: a zero scale
    bad = mo;
    bad.sphere_transform = sing.data();
    EXPECT(throws<std::invalid_argument>([&] { build(bad); }));
    rt_scene_desc own = g.desc;
    own.bvh_num_nodes = 1;
    EXPECT(throws<std::domain_error>([&] { build_moving(own, &in, &mo, kDefaultTreeletLeaves, ih); }));
  }
  std::printf(failures ? "motion_host_check: %d FAILED\n" : "motion_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
