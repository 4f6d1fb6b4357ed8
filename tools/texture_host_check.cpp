// Stand-alone host check of the texture code, for sanitizer runs:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -pthread \
//       tools/texture_host_check.cpp \
//       ceng795_amd/csrc/{scene_build,accel_build,scene_xml,xml_dom}.cpp \
//       -o texture_host_check && ./texture_host_check [scene.xml ...]
// Runs the host lookup (pack_textures + tex_get_color, the function the kernels run) on the edge
// grid of the tests — every size and mode pair, coordinates at the texel borders and their fp32
// neighbours, negative, large, NaN and infinite ones — with every texture in a heap block of its
// exact size, so a read past a texture's end is a sanitizer error; checks the hand-derived values;
// builds a textured scene's leaf records; and parses every scene file named (load_textures_xml).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <vector>

#include "../ceng795_amd/csrc/host_scene.h"

using namespace rt;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::vector<float> edge_coordinates(int n) {
  std::vector<float> out;
  const float inf = std::numeric_limits<float>::infinity();
  for (int k = 0; k <= n; k++) {
    const float x = (float)k / (float)n;
    out.insert(out.end(), {std::nextafter(x, -inf), x, std::nextafter(x, inf)});
  }
  out.insert(out.end(), {-0.0f, -0.25f, -1.0f, 1.0f - 0x1p-24f, 1.0f, 1.5f, 2.0f, 1e9f,
                         std::numeric_limits<float>::quiet_NaN(), inf, -inf});
  return out;
}

// One texture of w x h texels in a heap block of exactly 3 w h bytes.
struct Image {
  std::unique_ptr<unsigned char[]> px;
  rt_texture t;
  Image(int w, int h, int interpolation, int appearance, unsigned seed) : px(new unsigned char[3 * w * h]) {
    for (int i = 0; i < 3 * w * h; i++) px[i] = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
    t = rt_texture{px.get(), w, h, interpolation, RT_TEX_BLEND_KD, appearance, 255.0f};
  }
};

static void lookup(const rt_texture& t, const std::vector<rt_tex_query>& q, std::vector<float>& rgb) {
  rt_texture_desc d{};
  d.struct_size = sizeof d;
  d.num_textures = 1;
  d.textures = &t;
  // the packed blob in a heap block of its exact size too
  std::vector<DevTexture> table;
  std::vector<uint32_t> texels;
  pack_textures(d, table, texels);
  texels.shrink_to_fit();
  rgb.assign(3 * q.size(), -1.0f);
  host_texture_lookup(table, texels, q.data(), (long long)q.size(), rgb.data());
}

static void grid() {
  const int sizes[][2] = {{1, 1}, {2, 2}, {3, 2}, {2, 3}, {4, 4}, {5, 7}};
  long long lookups = 0;
  for (const auto& s : sizes)
    for (int interpolation = 0; interpolation < 2; interpolation++)
      for (int appearance = 0; appearance < 2; appearance++) {
        const Image img(s[0], s[1], interpolation, appearance, 7u * s[0] + s[1]);
        std::vector<rt_tex_query> q;
        for (float u : edge_coordinates(s[0]))
          for (float v : edge_coordinates(s[1])) q.push_back(rt_tex_query{0, u, v, 0});
        q.push_back(rt_tex_query{-1, 0.5f, 0.5f, 0});
        q.push_back(rt_tex_query{1, 0.5f, 0.5f, 0});
        std::vector<float> rgb;
        lookup(img.t, q, rgb);
        for (size_t i = 0; i + 2 < q.size(); i++)
          for (int c = 0; c < 3; c++) EXPECT(rgb[3 * i + c] >= 0.0f && rgb[3 * i + c] <= 255.0f);
        for (size_t i = q.size() - 2; i < q.size(); i++)
          for (int c = 0; c < 3; c++) EXPECT(rgb[3 * i + c] == 0.0f);
        lookups += (long long)q.size();
      }
  std::printf("grid: %lld lookups\n", lookups);
}

static void hand_derived() {
  auto grey = [](std::vector<unsigned char> v) {
    std::vector<unsigned char> out;
    for (unsigned char x : v) out.insert(out.end(), {x, x, x});
    return out;
  };
  const std::vector<unsigned char> a = grey({0, 40, 80, 120}), b = grey({0, 40, 80, 120, 200, 16});
  const rt_texture t22{a.data(), 2, 2, RT_TEX_BILINEAR, RT_TEX_BLEND_KD, RT_TEX_CLAMP, 255.0f};
  const rt_texture t23{b.data(), 2, 3, RT_TEX_BILINEAR, RT_TEX_BLEND_KD, RT_TEX_CLAMP, 255.0f};
  std::vector<float> rgb;
  lookup(t22, {rt_tex_query{0, 0.25f, 0.25f, 0}, rt_tex_query{0, 0.75f, 0.25f, 0}}, rgb);
  EXPECT(rgb[0] == 60.0f && rgb[1] == 60.0f && rgb[2] == 60.0f);
  EXPECT(rgb[3] == 10.0f);  // pn == w: the index past the end is skipped
  lookup(t23, {rt_tex_query{0, 0.75f, 1.0f / 6.0f, 0}}, rgb);
  EXPECT(rgb[0] == 60.0f);  // ... and here it is the first texel of row 2: 10 + 200 / 4
}

static void bad_descriptors() {
  const Image img(2, 2, RT_TEX_BILINEAR, RT_TEX_CLAMP, 1);
  auto refused = [&](rt_texture t, size_t struct_size = sizeof(rt_texture_desc)) {
    rt_texture_desc d{};
    d.struct_size = struct_size;
    d.num_textures = 1;
    d.textures = &t;
    std::vector<DevTexture> table;
    std::vector<uint32_t> texels;
    try {
      pack_textures(d, table, texels);
    } catch (const std::invalid_argument&) {
      return true;
    }
    return false;
  };
  rt_texture t = img.t;
  EXPECT(!refused(t));
  EXPECT(refused(t, sizeof(rt_texture_desc) - 1));
  t.rgb8 = nullptr;
  EXPECT(refused(t));
  t = img.t, t.width = 0;
  EXPECT(refused(t));
  t = img.t, t.height = 16385;
  EXPECT(refused(t));
  t = img.t, t.interpolation = 2;
  EXPECT(refused(t));
  t = img.t, t.decal = -1;
  EXPECT(refused(t));
  t = img.t, t.appearance = 2;
  EXPECT(refused(t));
  t = img.t, t.normalizer = 0.0f;
  EXPECT(refused(t));
  t = img.t, t.normalizer = std::numeric_limits<float>::quiet_NaN();
  EXPECT(refused(t));
}

// A quad mesh, a loose triangle and a sphere, each with a texture: the leaf records.
static void textured_scene() {
  const std::vector<float> verts = {-1, 0, -1, 1, 0, -1, 1, 0, 1, -1, 0, 1, 0, 1, 0, 1, 2, 0, -1, 2, 0, 0, 3, 0};
  const std::vector<int> faces = {0, 2, 1, 0, 3, 2}, counts = {2}, zero = {0}, tri = {4, 5, 6}, center = {7};
  const std::vector<float> radius = {0.5f}, uv(2 * 8, 0.25f);
  rt_material m;
  std::memset(&m, 0, sizeof m);
  rt_scene_desc d;
  std::memset(&d, 0, sizeof d);
  d.vertices = verts.data(), d.num_vertices = 8;
  d.materials = &m, d.num_materials = 1;
  d.num_meshes = 1, d.mesh_material = zero.data(), d.mesh_face_count = counts.data(), d.mesh_faces = faces.data();
  d.num_triangles = 1, d.triangle_indices = tri.data(), d.triangle_material = zero.data();
  d.num_spheres = 1, d.sphere_center = center.data(), d.sphere_radius = radius.data(), d.sphere_material = zero.data();
  const Image i0(3, 2, RT_TEX_NEAREST, RT_TEX_REPEAT, 5), i1(5, 7, RT_TEX_BILINEAR, RT_TEX_CLAMP, 6);
  const rt_texture recs[2] = {i0.t, i1.t};
  const std::vector<int> one = {1}, none = {-1};
  rt_texture_desc t{};
  t.struct_size = sizeof t, t.num_textures = 2, t.textures = recs;
  t.mesh_texture = zero.data(), t.triangle_texture = one.data(), t.sphere_texture = one.data();
  const rt_surface_desc surf{sizeof(rt_surface_desc), nullptr, nullptr, uv.data()};
  HostScene s;
  build_host_scene(d, s);
  build_surface(d, &surf, s);
  build_textures(d, &surf, &t, s);
  EXPECT(s.textures.size() == 2 && s.texels.size() == 3 * 2 + 5 * 7);
  EXPECT(s.blank_material == 1 && s.materials.size() == 2);
  EXPECT(s.leaf_tri.size() == 4 * s.leaf_src.size() && s.leaf_src.size() == 4);
  for (size_t k = 0; k < s.leaf_src.size(); k++) {
    const LeafSource& l = s.leaf_src[k];
    const int want = l.object < 2 ? 0 : 1;
    EXPECT((s.leaf_tri[4 * k + 3] >> kSurfTexShift) - 1 == want);
  }
  // without uv: the sphere alone may be textured
  HostScene plain;
  build_host_scene(d, plain);
  build_surface(d, nullptr, plain);
  bool refused = false;
  try {
    build_textures(d, nullptr, &t, plain);
  } catch (const std::invalid_argument&) {
    refused = true;
  }
  EXPECT(refused);
  t.mesh_texture = none.data(), t.triangle_texture = nullptr;
  build_textures(d, nullptr, &t, plain);
  EXPECT(plain.textures.size() == 2 && plain.leaf_tri.size() == 16);
  t.sphere_texture = none.data();  // nothing textured: the scene is left as it was
  HostScene bare;
  build_host_scene(d, bare);
  build_textures(d, nullptr, &t, bare);
  EXPECT(bare.textures.empty() && bare.leaf_tri.empty() && bare.materials.size() == 1);
}

int main(int argc, char** argv) {
  grid();
  hand_derived();
  bad_descriptors();
  textured_scene();
  for (int i = 1; i < argc; i++) {
    try {
      XmlTextures xt;
      load_textures_xml(argv[i], xt);
      std::printf("%s: %zu textures, %zu uv pairs, %zu + %zu + %zu objects\n", argv[i],
                  xt.image_name.size(), xt.uv.size() / 2, xt.mesh_texture.size(),
                  xt.triangle_texture.size(), xt.sphere_texture.size());
    } catch (const std::exception& e) {
      std::printf("%s: refused: %s\n", argv[i], e.what());
    }
  }
  std::printf(failures ? "texture_host_check: %d FAILURES\n" : "texture_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
