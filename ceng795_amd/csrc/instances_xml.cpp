// XML ingest of instanced scenes: load_scene_xml's description plus what HW3
// adds for instances.
//
//   <Transformations> block   HW3/src/Scene.cpp:572-608, Transformation.cpp:6-72 (Scaling,
//                             Translation, Rotation in degrees, the host's std::cos / std::sin)
//   per-object lists          "s1 t2 r1", each element left-multiplying (Scene.cpp:641-664)
//   <Mesh> k                  instance k with its own base transformation (Scene.cpp:706-710)
//   <MeshInstance>            baseMeshId, resetTransform, its material (Scene.cpp:713-761)
//   vertexOffset              added to the mesh's vertex ids (Scene.cpp:681)
//
// All numbers go through one std::stringstream and operator>>, as there.  Compiled with
// -ffp-contract=off: the matrix products round as the reference's.
#include <cmath>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>

#include "host_scene.h"
#include "mat4.h"
#include "xml_dom.h"

namespace rt {
namespace {

[[noreturn]] void unsupported(const std::string& what) {
  throw std::domain_error("scene xml: " + what + " is not supported in instanced scenes");
}

Mat4 scaling(float x, float y, float z) {
  Mat4 m = Mat4::zero();
  m.a[0][0] = x;
  m.a[1][1] = y;
  m.a[2][2] = z;
  m.a[3][3] = 1.0f;
  return m;
}
Mat4 translation(float x, float y, float z) {
  Mat4 m = Mat4::identity();
  m.a[0][3] = x;
  m.a[1][3] = y;
  m.a[2][3] = z;
  return m;
}
// Rotation::Rotation: the basis (u, v, w) with u the axis, M^T (R_x(angle) M).
Mat4 rotation(float angle, float x, float y, float z) {
  auto unit = [](float* v) {
    const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int i = 0; i < 3; i++) v[i] = v[i] / len;
  };
  float u[3] = {x, y, z};
  unit(u);
  float v[3] = {0.0f, 1.0f, 0.0f};
  if (x != 0.0f || y != 0.0f) {
    v[0] = -u[1];
    v[1] = u[0];
    v[2] = 0.0f;
  }
  unit(v);
  const float w[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                      u[0] * v[1] - u[1] * v[0]};
  Mat4 m = Mat4::zero();
  for (int j = 0; j < 3; j++) {
    m.a[0][j] = u[j];
    m.a[1][j] = v[j];
    m.a[2][j] = w[j];
  }
  m.a[3][3] = 1.0f;
  Mat4 rot = Mat4::zero();
  rot.a[0][0] = 1.0f;
  rot.a[1][1] = std::cos(angle);
  rot.a[1][2] = -std::sin(angle);
  rot.a[2][1] = -rot.a[1][2];
  rot.a[2][2] = rot.a[1][1];
  rot.a[3][3] = 1.0f;
  return m.transposed() * (rot * m);
}

struct Lists {
  std::vector<Mat4> s, t, r;
};

// "<Transformations>s1 t2 r1</Transformations>" onto m, each element left-multiplying.
Mat4 apply_list(std::stringstream& ss, const Node* n, const Lists& T, Mat4 m) {
  if (!n) return m;
  ss.clear();
  ss << node_text(n, "Transformations") << std::endl;
  char type;
  int index;
  while (!(ss >> type).eof()) {
    ss >> index;
    if (ss.fail()) throw std::runtime_error("scene xml: bad <Transformations> list");
    index--;
    const std::vector<Mat4>* list = type == 's' ? &T.s : type == 't' ? &T.t : type == 'r' ? &T.r : nullptr;
    if (!list) continue;  // (the reference's switch has no default)
    if (index < 0 || index >= (int)list->size())
      throw std::runtime_error("scene xml: transformation index out of range");
    m = (*list)[(size_t)index] * m;
  }
  ss.clear();
  return m;
}

// <MotionBlur>x y z</MotionBlur> (Scene.cpp:666-672, 752-758, 856-862): appended to `velocity`
// when the loader reads motion, else refused unless zero.
void read_motion_blur(std::stringstream& ss, const Node* object, std::vector<float>* velocity) {
  const Node* mb = object->first("MotionBlur");
  float v[3] = {0, 0, 0};
  if (mb) {
    ss << node_text(mb, "MotionBlur") << std::endl;
    ss >> v[0] >> v[1] >> v[2];
    ss.clear();
  }
  if (velocity)
    velocity->insert(velocity->end(), v, v + 3);
  else if (v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f)
    unsupported("a non-zero <MotionBlur>");
}

}  // namespace

void load_instances_xml(const std::string& path, XmlSceneStorage& st, rt_scene_desc& d,
                        XmlInstances& out, bool motion) {
  load_scene_xml(path, st, d);
  const std::unique_ptr<Node> root = parse_xml_file(path);
  std::stringstream ss;
  Lists T;
  if (const Node* tr = root->first("Transformations")) {
    for (const Node* c : tr->each("Scaling")) {
      float x, y, z;
      ss << node_text(c, "Scaling") << std::endl;
      ss >> x >> y >> z;
      T.s.push_back(scaling(x, y, z));
    }
    for (const Node* c : tr->each("Translation")) {
      float x, y, z;
      ss << node_text(c, "Translation") << std::endl;
      ss >> x >> y >> z;
      T.t.push_back(translation(x, y, z));
    }
    const float degree_to_pi = M_PI / 180.0f;  // Scene.cpp:315
    for (const Node* c : tr->each("Rotation")) {
      float angle, x, y, z;
      ss << node_text(c, "Rotation") << std::endl;
      ss >> angle >> x >> y >> z;
      T.r.push_back(rotation(angle * degree_to_pi, x, y, z));
    }
    if (ss.fail()) throw std::runtime_error("scene xml: bad <Transformations> block");
  }
  ss.clear();
  const Node* objs = root->first("Objects");  // (load_scene_xml has checked it)
  out = XmlInstances{};
  std::vector<Mat4> base;
  auto add = [&](int mesh, int material, const Mat4& m) {
    out.mesh.push_back(mesh);
    out.material.push_back(material);
    out.transform.insert(out.transform.end(), &m.a[0][0], &m.a[0][0] + 16);
  };
  size_t face = 0;
  int k = 0;
  for (const Node* m : objs->each("Mesh")) {
    const Node* faces = m->first("Faces");
    if (faces && faces->attr("plyFile")) unsupported("plyFile");
    read_motion_blur(ss, m, motion ? &out.velocity : nullptr);
    // vertexOffset (text faces; load_scene_xml has applied a binary list's already)
    const size_t count = 3 * (size_t)st.mesh_face_count[(size_t)k];
    if (faces && !faces->attr("binaryFile")) {
      const int offset = faces->int_attr("vertexOffset", 0);
      for (size_t i = 0; i < count; i++) st.mesh_faces[face + i] += offset;
    }
    face += count;
    base.push_back(apply_list(ss, m->first("Transformations"), T, Mat4::identity()));
    add(k, st.mesh_material[(size_t)k], base.back());
    k++;
  }
  for (const Node* e : objs->each("MeshInstance")) {
    const int id = e->int_attr("baseMeshId", 0) - 1;
    if (id < 0 || id >= (int)base.size()) throw std::runtime_error("scene xml: baseMeshId out of range");
    int material;
    ss << node_text(e->first("Material"), "Material") << std::endl;
    ss >> material;
    ss.clear();
    read_motion_blur(ss, e, motion ? &out.velocity : nullptr);  // (its own, not its base's)
    Mat4 m = base[(size_t)id];
    const char* reset = e->attr("resetTransform");
    if (reset && std::string(reset) == "true") m = Mat4::identity();
    add(id, material - 1, apply_list(ss, e->first("Transformations"), T, m));
  }
  for (const char* kind : {"Triangle", "Sphere"})
    for (const Node* e : objs->each(kind)) {
      const bool sphere = std::string(kind) == "Sphere";
      if (motion && sphere) {  // Scene.cpp:838-863: its own list onto the identity, its velocity
        const Mat4 m = apply_list(ss, e->first("Transformations"), T, Mat4::identity());
        out.sphere_transform.insert(out.sphere_transform.end(), &m.a[0][0], &m.a[0][0] + 16);
        read_motion_blur(ss, e, &out.sphere_velocity);
        continue;
      }
      if (e->first("Transformations")) unsupported(std::string("<Transformations> on a <") + kind + ">");
      read_motion_blur(ss, e, nullptr);
    }
}

}  // namespace rt
