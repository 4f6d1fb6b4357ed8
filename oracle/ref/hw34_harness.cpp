// ORACLE TEST INFRASTRUCTURE — never shipped, never measured as the product.
//
// Probe harness linked against the UNMODIFIED reference HW3 or HW4 sources (every src/*.cpp but
// main.cpp), compiled where they lie by oracle/Makefile: -DREF_HW=3 gives oracle/_ref/hw3_harness,
// -DREF_HW=4 gives oracle/_ref/hw4_harness.  Nothing of the reference is copied.
//
// Public reference API driven here:
//   * Scene::Scene(xml)                              src/Scene.cpp
//   * scene.bvh->intersect(Ray(o, d, r_primary, time), Hit_data&)     Shape.h, Ray.h, Hit_data.h
//   * Shape::get_material_id(), on HW4 Shape::get_texture_id(), Hit_data::u / v
//   * scene.textures[k].get_color_at(u, v)           HW4 Texture.h:12
//   * scene.vertex_data[i].has_vertex_normal() / get_vertex_normal()   Vertex.h
//   * Ray::in_medium                                 Ray.h (public member)
// One private member is opened: Scene::trace_ray (Scene.h).  This translation unit alone sees
// Scene.h with `private` redefined, after every standard header and every other reference header
// is in, so that only the Scene class itself is touched; the layout of the class does not depend
// on access, and the reference's objects are compiled unmodified.
//
// All files are raw little-endian records of 4-byte fields (f: float, i: int32).
//
//   hits <xml> <rays.bin> <out.bin>
//       rays.bin: 28 B  {f o[3], f d[3], f time}
//       out.bin:  40 B  {i hit, f t, f normal[3], i material, f u, f v, i texture, i 0}
//       of bvh->intersect(Ray(o, d, r_primary, time), h) with h.t = +inf, h.shape = NULL.
//       material / texture are the hit shape's 0-based ids (-1: none).  u, v are Hit_data's on
//       HW4 where the shape has a texture, else 0 (HW3 has neither field).  A miss is
//       {0, 0, 0 0 0, -1, 0, 0, -1, 0}.
//   trace <xml> <rays.bin> <out.bin> [depth]
//       rays.bin: 32 B  {f o[3], f d[3], f time, i in_medium}
//       out.bin:  12 B  {f r, f g, f b} = Scene::trace_ray(ray, depth), ray a Ray(o, d,
//       r_primary, time) with ray.in_medium set; depth defaults to the scene's MaxRecursionDepth.
//   texels <xml> <queries.bin> <out.bin>             (HW4 only)
//       queries.bin: 12 B {i k, f u, f v};  out.bin: 12 B raw channels of
//       scene.textures[k].get_color_at(u, v).
//   normals <xml> <out.bin>
//       16 B per vertex of scene.vertex_data: {i has_normal, f normal[3]} after the loader's
//       finalize pass.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <memory>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Area_light.h"
#include "Bounding_box.h"
#include "Bounding_volume_hierarchy.h"
#include "Camera.h"
#include "Hit_data.h"
#include "Material.h"
#include "Matrix4x4.h"
#include "Mesh.h"
#include "Mesh_triangle.h"
#include "Point_light.h"
#include "Ray.h"
#include "Shape.h"
#include "Sphere.h"
#include "Transformation.h"
#include "Triangle.h"
#include "Vector3.h"
#include "Vertex.h"
#if REF_HW >= 4
#include "Perlin_noise.h"
#include "Texture.h"
#endif
#define private public
#include "Scene.h"
#undef private

static_assert(sizeof(float) == 4 && sizeof(int) == 4, "4-byte fields");

struct HitRecord {
  int hit;
  float t;
  float normal[3];
  int material;
  float u, v;
  int texture;
  int zero;
};
static_assert(sizeof(HitRecord) == 40, "hits record");

static std::vector<char> read_all(const char* path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) {
    std::cerr << "cannot read " << path << std::endl;
    std::exit(1);
  }
  return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::cerr << "usage: hw" << REF_HW << "_harness hits|trace|texels|normals <xml> ..." << std::endl;
    return 2;
  }
  const std::string cmd = argv[1];
  Scene scene(argv[2]);
  if (cmd == "hits" && argc >= 5) {
    const std::vector<char> in = read_all(argv[3]);
    const size_t n = in.size() / 28;
    std::vector<HitRecord> out(n);
    for (size_t i = 0; i < n; i++) {
      float r[7];
      std::memcpy(r, in.data() + 28 * i, 28);
      Hit_data h;
      h.t = std::numeric_limits<float>::infinity();
      h.shape = NULL;
#if REF_HW >= 4
      h.u = h.v = 0.0f;
#endif
      const Ray ray(Vector3(r[0], r[1], r[2]), Vector3(r[3], r[4], r[5]), r_primary, r[6]);
      HitRecord rec = {0, 0.0f, {0.0f, 0.0f, 0.0f}, -1, 0.0f, 0.0f, -1, 0};
      if (scene.bvh->intersect(ray, h)) {
        rec.hit = 1;
        rec.t = h.t;
        rec.normal[0] = h.normal.x;
        rec.normal[1] = h.normal.y;
        rec.normal[2] = h.normal.z;
        rec.material = h.shape->get_material_id();
#if REF_HW >= 4
        rec.texture = h.shape->get_texture_id();
        if (rec.texture != -1) {
          rec.u = h.u;
          rec.v = h.v;
        }
#endif
      }
      out[i] = rec;
    }
    std::ofstream f(argv[4], std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), out.size() * sizeof(HitRecord));
  } else if (cmd == "trace" && argc >= 5) {
    const std::vector<char> in = read_all(argv[3]);
    const size_t n = in.size() / 32;
    const int depth = argc > 5 ? std::atoi(argv[5]) : scene.max_recursion_depth;
    std::vector<float> out(3 * n);
    for (size_t i = 0; i < n; i++) {
      float r[7];
      int medium;
      std::memcpy(r, in.data() + 32 * i, 28);
      std::memcpy(&medium, in.data() + 32 * i + 28, 4);
      Ray ray(Vector3(r[0], r[1], r[2]), Vector3(r[3], r[4], r[5]), r_primary, r[6]);
      ray.in_medium = medium != 0;
      const Vector3 c = scene.trace_ray(ray, depth);
      out[3 * i + 0] = c.x;
      out[3 * i + 1] = c.y;
      out[3 * i + 2] = c.z;
    }
    std::ofstream f(argv[4], std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), out.size() * sizeof(float));
#if REF_HW >= 4
  } else if (cmd == "texels" && argc >= 5) {
    const std::vector<char> in = read_all(argv[3]);
    const size_t n = in.size() / 12;
    std::vector<float> out(3 * n);
    for (size_t i = 0; i < n; i++) {
      int k;
      float uv[2];
      std::memcpy(&k, in.data() + 12 * i, 4);
      std::memcpy(uv, in.data() + 12 * i + 4, 8);
      if (k < 0 || (size_t)k >= scene.textures.size()) {
        std::cerr << "texels: no texture " << k << std::endl;
        return 1;
      }
      const Vector3 c = scene.textures[k].get_color_at(uv[0], uv[1]);
      out[3 * i + 0] = c.x;
      out[3 * i + 1] = c.y;
      out[3 * i + 2] = c.z;
    }
    std::ofstream f(argv[4], std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), out.size() * sizeof(float));
#endif
  } else if (cmd == "normals") {
    std::ofstream f(argv[3], std::ios::binary);
    for (const Vertex& v : scene.vertex_data) {
      const int has = v.has_vertex_normal() ? 1 : 0;
      const Vector3& nrm = v.get_vertex_normal();
      const float rec[3] = {nrm.x, nrm.y, nrm.z};
      f.write(reinterpret_cast<const char*>(&has), 4);
      f.write(reinterpret_cast<const char*>(rec), 12);
    }
  } else {
    std::cerr << "unknown command " << cmd << std::endl;
    return 2;
  }
  return 0;
}
