// Instanced scenes on the host: HW3's Mesh_instance over HW2's scene.
//
//   object list order   HW3/src/Scene.cpp:706-869 (instances, loose triangles, spheres)
//   base mesh tree      Mesh::Mesh, HW3/include/Mesh.h:31-34 (create_bvh over its faces alone)
//   matrices            HW3/src/Matrix4x4.cpp (mat4.h): inverse by cofactors, multiply(point)
//   instance box        Bounding_box::apply_transform, HW3/src/bounding_box.cpp:40-114
//   top-level tree      the median-split BVH of HW2/Bounding_volume_hierarchy.cpp:3-29
//
// Compiled with -ffp-contract=off like scene_build.cpp: every fp32 expression rounds as there.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

#include "host_scene.h"
#include "mat4.h"

namespace rt {
namespace {

constexpr float kInf = std::numeric_limits<float>::infinity();

void fail(const std::string& m) { throw std::invalid_argument(m); }

struct Box {
  float lo[3] = {kInf, kInf, kInf};
  float hi[3] = {-kInf, -kInf, -kInf};
  float mid[3] = {0, 0, 0};  // Bounding_box::center = (max + min) / 2
  void set_mid() {
    for (int a = 0; a < 3; a++) mid[a] = (hi[a] + lo[a]) / 2.0f;
  }
};

// Bounding_box::apply_transform: the eight corners through multiply(point), fmin / fmax folded in
// the corner order 000 001 010 011 100 101 110 111 (x the slowest).
Box transformed_box(const float root_box[6], const Mat4& m) {
  Box b;
  for (int k = 0; k < 8; k++) {
    const float c[3] = {root_box[(k & 4) ? 3 : 0], root_box[(k & 2) ? 4 : 1],
                        root_box[(k & 1) ? 5 : 2]};
    float p[3];
    m.point(c, p);
    for (int a = 0; a < 3; a++) {
      b.lo[a] = k == 0 ? p[a] : std::fmin(b.lo[a], p[a]);
      b.hi[a] = k == 0 ? p[a] : std::fmax(b.hi[a], p[a]);
    }
  }
  b.set_mid();
  return b;
}

// BVH::BVH over ids[begin, end) (HW2/Bounding_volume_hierarchy.cpp:3-29) as scene_build.cpp builds
// it, flattened as it goes: nodes in DFS preorder, each holding both child boxes; a leaf child is
// ~(its DFS position) and its slot holds the +-1e30 box of rt_internal.h.
struct TopBuilder {
  const std::vector<Box>& boxes;
  std::vector<DevNode>& nodes;
  std::vector<int>& order;  // DFS position -> object
  int depth = 0;

  Box united(const std::vector<int>& ids, int b, int e) const {
    Box u;
    for (int i = b; i < e; i++)
      for (int a = 0; a < 3; a++) {
        u.lo[a] = std::fmin(u.lo[a], boxes[ids[i]].lo[a]);
        u.hi[a] = std::fmax(u.hi[a], boxes[ids[i]].hi[a]);
      }
    u.set_mid();
    return u;
  }
  static void put_child(DevNode& n, int side, const float* lo, const float* hi) {
    for (int a = 0; a < 3; a++) {
      n.lo[a][side] = lo[a];
      n.hi[a][side] = hi[a];
    }
  }
  // the node over ids[b, e) (e - b >= 2), whose own box is `box`; returns its index
  int build(std::vector<int>& ids, int b, int e, int axis, const Box& box, int level) {
    const float split = box.mid[axis];
    int m = b;
    for (int i = b; i < e; i++)
      if (boxes[ids[i]].mid[axis] < split) std::swap(ids[i], ids[m++]);
    if (m == b || m == e) m = b + (e - b) / 2;
    const int id = (int)nodes.size();
    nodes.push_back(DevNode{});
    nodes[id].axis = axis;
    depth = std::max(depth, level + 1);
    const int next = (axis + 1) % 3;
    const int bounds[2][2] = {{b, m}, {m, e}};
    for (int side = 0; side < 2; side++) {
      const int cb = bounds[side][0], ce = bounds[side][1];
      if (cb + 1 == ce) {
        const float lo[3] = {-1e30f, -1e30f, -1e30f}, hi[3] = {1e30f, 1e30f, 1e30f};
        put_child(nodes[id], side, lo, hi);
        nodes[id].child[side] = ~(int)order.size();
        order.push_back(ids[cb]);
      } else {
        const Box cbx = united(ids, cb, ce);
        put_child(nodes[id], side, cbx.lo, cbx.hi);
        const int c = build(ids, cb, ce, next, cbx, level + 1);
        nodes[id].child[side] = c;
      }
    }
    return id;
  }
};

// Mesh_instance::Mesh_instance / Sphere::Sphere with velocity != 0 (Mesh.h:104-110,
// Sphere.h:30-36): (min, max) expanded by (min + v, max + v), then by (min - v, max - v).
void expand_by_velocity(Box& b, const float v[3]) {
  for (int a = 0; a < 3; a++) {
    const float lo = b.lo[a], hi = b.hi[a];
    b.lo[a] = std::fmin(b.lo[a], lo + v[a]);
    b.hi[a] = std::fmax(b.hi[a], hi + v[a]);
    b.lo[a] = std::fmin(b.lo[a], lo - v[a]);
    b.hi[a] = std::fmax(b.hi[a], hi - v[a]);
  }
  b.set_mid();
}

bool nonzero3(const float* v) { return v && !(v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f); }

// The motion descriptor against the other two: what build_moving and motion_trivial refuse.
void check_motion_desc(const rt_scene_desc& d, const rt_instance_desc* in,
                       const rt_motion_desc* mo) {
  if (!mo) return;
  if (mo->struct_size < sizeof(rt_motion_desc)) fail("rt_motion_desc::struct_size too small");
  const int ni = in ? in->num_instances : 0;
  if (mo->num_instances != ni && !(mo->num_instances == 0 && !mo->instance_velocity))
    fail("rt_motion_desc::num_instances differs from the instance descriptor's");
  if (mo->num_spheres != d.num_spheres &&
      !(mo->num_spheres == 0 && !mo->sphere_transform && !mo->sphere_velocity))
    fail("rt_motion_desc::num_spheres differs from the scene description's");
  auto finite = [](const float* p, size_t count, const char* what) {
    for (size_t k = 0; p && k < count; k++)
      if (!std::isfinite(p[k])) fail(std::string(what) + ": a non-finite entry");
  };
  finite(mo->instance_velocity, 3 * (size_t)std::max(mo->num_instances, 0), "instance_velocity");
  finite(mo->sphere_transform, 16 * (size_t)std::max(mo->num_spheres, 0), "sphere_transform");
  finite(mo->sphere_velocity, 3 * (size_t)std::max(mo->num_spheres, 0), "sphere_velocity");
  for (int k = 0; mo->sphere_transform && k < mo->num_spheres; k++) {
    Mat4 m, inv;
    std::memcpy(m.a, mo->sphere_transform + 16 * (size_t)k, sizeof m.a);
    if (!m.inverse(inv))
      fail("sphere " + std::to_string(k) + ": the transformation is not invertible");
  }
}

void build_impl(const rt_scene_desc& d, const rt_instance_desc* inp, const rt_motion_desc* mo,
                int treelets, InstHost& out);

}  // namespace

void build_instanced(const rt_scene_desc& d, const rt_instance_desc& in, int treelets,
                     InstHost& out) {
  if (d.bvh_num_leaves > 0 || d.bvh_num_nodes > 0)
    throw std::domain_error("instanced scenes do not take the caller's own BVH (bvh_*)");
  if (in.num_instances <= 0) fail("num_instances <= 0");
  build_impl(d, &in, nullptr, treelets, out);
}

bool motion_trivial(const rt_scene_desc& d, const rt_instance_desc* in, const rt_motion_desc* mo) {
  check_motion_desc(d, in, mo);
  if (!mo) return true;
  for (int i = 0; mo->instance_velocity && i < mo->num_instances; i++)
    if (nonzero3(mo->instance_velocity + 3 * (size_t)i)) return false;
  for (int k = 0; k < mo->num_spheres; k++) {
    if (mo->sphere_velocity && nonzero3(mo->sphere_velocity + 3 * (size_t)k)) return false;
    if (mo->sphere_transform) {
      Mat4 m;
      std::memcpy(m.a, mo->sphere_transform + 16 * (size_t)k, sizeof m.a);
      if (!m.identity_p()) return false;
    }
  }
  return true;
}

void build_moving(const rt_scene_desc& d, const rt_instance_desc* in, const rt_motion_desc* mo,
                  int treelets, InstHost& out) {
  if (d.bvh_num_leaves > 0 || d.bvh_num_nodes > 0)
    throw std::domain_error("instanced scenes do not take the caller's own BVH (bvh_*)");
  check_motion_desc(d, in, mo);
  build_impl(d, in, mo, treelets, out);
}

namespace {

void build_impl(const rt_scene_desc& d, const rt_instance_desc* inp, const rt_motion_desc* mo,
                int treelets, InstHost& out) {
  const rt_instance_desc none{sizeof(rt_instance_desc), 0, nullptr, nullptr, nullptr};
  const rt_instance_desc& in = inp ? *inp : none;
  const int n = in.num_instances;
  if (n < 0) fail("num_instances < 0");
  if (n > 0 && (!in.instance_mesh || !in.instance_material || !in.instance_transform))
    fail("instance_mesh / instance_material / instance_transform == NULL");
  const float* inst_vel = mo && mo->num_instances == n ? mo->instance_velocity : nullptr;
  const bool sphere_motion = mo && mo->num_spheres == d.num_spheres;
  const float* sph_vel = sphere_motion ? mo->sphere_velocity : nullptr;
  const float* sph_xf = sphere_motion ? mo->sphere_transform : nullptr;
  if (d.num_meshes < 0 || d.num_triangles < 0 || d.num_spheres < 0 || d.num_vertices < 0 ||
      d.num_materials < 0)
    fail("negative count in scene description");
  if (d.num_meshes > 0 && (!d.mesh_face_count || !d.mesh_faces)) fail("mesh arrays == NULL");
  out = InstHost{};

  // ---- the base meshes: each a scene of its own
  out.meshes.resize((size_t)d.num_meshes);
  long long face_base = 0;
  int leaf_base = 0;
  const int zero_material = 0;
  for (int m = 0; m < d.num_meshes; m++) {
    rt_scene_desc sub;
    std::memset(&sub, 0, sizeof sub);
    sub.vertices = d.vertices;
    sub.num_vertices = d.num_vertices;
    sub.materials = d.materials;  // (mesh_material is ignored: the faces carry material 0)
    sub.num_materials = d.num_materials;
    sub.num_meshes = 1;
    sub.mesh_material = &zero_material;
    sub.mesh_face_count = d.mesh_face_count + m;
    sub.mesh_faces = d.mesh_faces + 3 * face_base;
    if (d.num_materials < 1) fail("material id out of range");
    HostScene& hs = out.meshes[(size_t)m];
    build_host_scene(sub, hs);
    build_accel(hs, treelets);
    long long stats[4] = {0, 0, 0, 0};
    if (hs.accel_root >= 0) {
      const std::string bad = check_accel(hs, treelets, stats);
      if (!bad.empty()) fail("base mesh " + std::to_string(m) + ": " + bad);
    }
    out.accel_stats.insert(out.accel_stats.end(), stats, stats + 4);
    if (hs.prims.size() >= (size_t(1) << 26))  // leaf indices share a 32-bit queue word with a lane
      fail("base mesh " + std::to_string(m) + ": meshes of 2^26 faces or more are not supported");
    if (std::max(hs.depth, hs.accel_depth) > kLaneStack - 2)
      throw std::domain_error("base mesh " + std::to_string(m) + ": a tree deeper than " +
                              std::to_string(kLaneStack - 2) +
                              " levels is not supported in instanced scenes");
    out.mesh_leaf_base.push_back(leaf_base);
    out.mesh_object_base.push_back((int)face_base);
    leaf_base += (int)hs.prims.size();
    face_base += d.mesh_face_count[m];
  }

  // ---- the loose primitives: a flat scene of them alone gives their records
  const int loose = d.num_triangles + d.num_spheres;
  HostScene ls;
  std::vector<int> loose_leaf((size_t)loose, -1);  // loose object -> its leaf in `ls`
  if (loose > 0) {
    rt_scene_desc sub;
    std::memset(&sub, 0, sizeof sub);
    sub.vertices = d.vertices;
    sub.num_vertices = d.num_vertices;
    sub.materials = d.materials;
    sub.num_materials = d.num_materials;
    sub.num_triangles = d.num_triangles;
    sub.triangle_indices = d.triangle_indices;
    sub.triangle_material = d.triangle_material;
    sub.num_spheres = d.num_spheres;
    sub.sphere_center = d.sphere_center;
    sub.sphere_radius = d.sphere_radius;
    sub.sphere_material = d.sphere_material;
    build_host_scene(sub, ls);
    for (size_t k = 0; k < ls.leaf_object.size(); k++) loose_leaf[(size_t)ls.leaf_object[k]] = (int)k;
    out.top_quot_ok = ls.quot_ok;
  }

  // ---- the instances
  std::vector<Box> boxes;
  out.instances.resize((size_t)n);
  out.inverse.resize((size_t)16 * n);
  for (int i = 0; i < n; i++) {
    const int mesh = in.instance_mesh[i], mat = in.instance_material[i];
    if (mesh < 0 || mesh >= d.num_meshes)
      fail("instance " + std::to_string(i) + ": mesh id out of range");
    if (mat < 0 || mat >= d.num_materials)
      fail("instance " + std::to_string(i) + ": material id out of range");
    Mat4 m, inv;
    std::memcpy(m.a, in.instance_transform + 16 * (size_t)i, sizeof m.a);
    if (!m.inverse(inv))
      fail("instance " + std::to_string(i) + ": the transformation is not invertible");
    std::memcpy(&out.inverse[16 * (size_t)i], inv.a, sizeof inv.a);
    const HostScene& hs = out.meshes[(size_t)mesh];
    // Mesh::get_bounding_box: its tree's root box; a one-face mesh: that triangle's box
    float root_box[6];
    if (hs.root_kind == kRootNode) {
      std::memcpy(root_box, hs.root_box, sizeof root_box);
    } else {
      const LeafSource& src = hs.leaf_src[(size_t)hs.root_ref];  // (ids checked by the build)
      for (int a = 0; a < 3; a++) {  // Triangle.cpp:4-34
        const float v0 = d.vertices[3 * src.i0 + a], v1 = d.vertices[3 * src.i1 + a],
                    v2 = d.vertices[3 * src.i2 + a];
        root_box[a] = std::fmin(std::fmin(v0, v1), v2);
        root_box[a + 3] = std::fmax(std::fmax(v0, v1), v2);
      }
    }
    Box b = transformed_box(root_box, m);
    const bool moves = inst_vel && nonzero3(inst_vel + 3 * (size_t)i);
    if (moves) expand_by_velocity(b, inst_vel + 3 * (size_t)i);
    if (mo) {
      DevMotionInstance mi;
      std::memset(&mi, 0, sizeof mi);
      std::memcpy(mi.fwd, m.a, sizeof mi.fwd);
      if (moves) std::memcpy(mi.vel, inst_vel + 3 * (size_t)i, sizeof mi.vel);
      out.motion_instances.push_back(mi);
      out.has_motion = out.has_motion || moves;
    }
    DevInstance& di = out.instances[(size_t)i];
    std::memset(&di, 0, sizeof di);
    di.moving = moves ? 1 : 0;
    std::memcpy(di.inv, inv.a, sizeof di.inv);  // rows 0..2
    std::memcpy(di.box, b.lo, 12);
    std::memcpy(di.box + 3, b.hi, 12);
    di.mesh = mesh;
    di.material = mat;
    boxes.push_back(b);
  }
  // loose triangles (Triangle.cpp:4-34), then spheres (Sphere.h:17-20)
  auto vertex = [&](int v, int a) {
    if (v < 0 || v >= d.num_vertices) fail("vertex index out of range");
    return d.vertices[3 * v + a];
  };
  for (int t = 0; t < d.num_triangles; t++) {
    Box b;
    for (int a = 0; a < 3; a++) {
      const float v0 = vertex(d.triangle_indices[3 * t], a), v1 = vertex(d.triangle_indices[3 * t + 1], a),
                  v2 = vertex(d.triangle_indices[3 * t + 2], a);
      b.lo[a] = std::fmin(std::fmin(v0, v1), v2);
      b.hi[a] = std::fmax(std::fmax(v0, v1), v2);
    }
    b.set_mid();
    boxes.push_back(b);
  }
  std::vector<int> sphere_record((size_t)d.num_spheres, -1);  // its DevMotionSphere, if any
  out.sphere_inverse.assign(16 * (size_t)d.num_spheres, 0.0f);
  for (int k = 0; k < d.num_spheres; k++) {
    Box b;
    for (int a = 0; a < 3; a++) {
      const float c = vertex(d.sphere_center[k], a), r = d.sphere_radius[k];
      b.lo[a] = c - r;
      b.hi[a] = c + r;
    }
    b.set_mid();
    // Sphere::Sphere (Sphere.h:18-37): through apply_transform unless the matrix is the identity,
    // then expanded by the velocity
    Mat4 m = Mat4::identity(), inv = Mat4::identity();
    if (sph_xf) std::memcpy(m.a, sph_xf + 16 * (size_t)k, sizeof m.a);
    const bool placed = !m.identity_p();
    const bool moves = sph_vel && nonzero3(sph_vel + 3 * (size_t)k);
    if (placed) {
      const float flat[6] = {b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]};
      b = transformed_box(flat, m);
      if (!m.inverse(inv))
        fail("sphere " + std::to_string(k) + ": the transformation is not invertible");
    }
    if (moves) expand_by_velocity(b, sph_vel + 3 * (size_t)k);
    std::memcpy(&out.sphere_inverse[16 * (size_t)k], inv.a, sizeof inv.a);
    if (placed || moves) {
      DevMotionSphere ms;
      std::memset(&ms, 0, sizeof ms);
      std::memcpy(ms.fwd, m.a, sizeof ms.fwd);
      std::memcpy(ms.inv, inv.a, sizeof ms.inv);  // rows 0..2
      if (moves) std::memcpy(ms.vel, sph_vel + 3 * (size_t)k, sizeof ms.vel);
      ms.moving = moves ? 1 : 0;
      for (int a = 0; a < 3; a++) ms.center[a] = vertex(d.sphere_center[k], a);
      ms.radius = d.sphere_radius[k];
      ms.material = d.sphere_material[k];
      sphere_record[(size_t)k] = (int)out.motion_spheres.size();
      out.motion_spheres.push_back(ms);
      out.has_motion = true;
    }
    out.sphere_box.insert(out.sphere_box.end(), b.lo, b.lo + 3);
    out.sphere_box.insert(out.sphere_box.end(), b.hi, b.hi + 3);
    boxes.push_back(b);
    out.has_spheres = true;
  }

  // ---- the top-level tree
  const int objects = n + loose;
  if (objects == 0) fail("no instance, loose triangle or sphere");
  std::vector<int> ids((size_t)objects), order;
  for (int i = 0; i < objects; i++) ids[(size_t)i] = i;
  if (objects == 1) {  // create_bvh, size 1: the object itself
    out.top_root_kind = kTopSingle;
    order.push_back(0);
  } else {
    TopBuilder tb{boxes, out.top_nodes, order};
    const Box root = tb.united(ids, 0, objects);
    tb.build(ids, 0, objects, 0, root, 0);
    out.top_root_kind = kTopNode;
    out.top_depth = tb.depth;
    std::memcpy(out.top_box, root.lo, 12);
    std::memcpy(out.top_box + 3, root.hi, 12);
    if (out.top_depth > kLaneStack - 2)
      throw std::domain_error("a top-level tree deeper than " + std::to_string(kLaneStack - 2) +
                              " levels is not supported");
  }
  out.inst_top_dfs.assign((size_t)n, -1);
  out.object_top_dfs.assign((size_t)objects, -1);
  out.top_prims.assign(order.size(), DevPrim{});
  out.top_normals.assign(4 * order.size(), 0.0f);
  out.top_info.assign(2 * order.size(), -1);
  const int total_faces = (int)face_base;
  for (size_t pos = 0; pos < order.size(); pos++) {
    const int obj = order[pos];
    DevPrim& p = out.top_prims[pos];
    out.object_top_dfs[(size_t)obj] = (int)pos;
    if (obj < n) {
      p.kind = kPrimInstance;
      p.material = obj;
      out.inst_top_dfs[(size_t)obj] = (int)pos;
    } else {
      const int k = obj - n, leaf = loose_leaf[(size_t)k];
      p = ls.prims[(size_t)leaf];
      std::memcpy(&out.top_normals[4 * pos], &ls.normals[4 * (size_t)leaf], 16);
      out.top_info[2 * pos] = total_faces + k;
      out.top_info[2 * pos + 1] = leaf_base + k;
      const int sphere = k - d.num_triangles;
      if (sphere >= 0 && sphere_record[(size_t)sphere] >= 0) {  // a kind of its own (§4.17)
        p.kind = kPrimMovingSphere;
        p.material = sphere_record[(size_t)sphere];
      }
    }
  }
  out.leaves = leaf_base + loose;
}

}  // namespace

}  // namespace rt
