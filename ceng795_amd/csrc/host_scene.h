// Host-side scene: validation, the reference-identical BVH build and its flattening into the
// device layout of rt_internal.h.  Untimed, like the reference's Scene constructor.
#ifndef CENG795_HOST_SCENE_H_
#define CENG795_HOST_SCENE_H_

#include <memory>
#include <string>
#include <vector>

#include "../../include/ceng795_rt.h"
#include "rt_internal.h"

namespace rt {

struct LeafSource {  // what the leaf was in the reference object list (for BVH dumps)
  int kind;          // kPrimTriangle / kPrimSphere
  int i0, i1, i2;    // triangle vertex ids (0-based)
  float center[3], radius;
  int material;
  int object;        // index in the object lists: triangles (mesh faces in mesh order, then loose
                     // triangles), then spheres — rt_scene_desc::bvh_leaf_object's numbering
};

struct HostScene {
  // scalars / lists copied from the description
  float background[3] = {0, 0, 0};
  float ambient[3] = {0, 0, 0};
  float eps = 0.001f;
  int max_depth = 0;
  std::vector<DevMaterial> materials;
  std::vector<DevLight> lights;
  std::vector<rt_camera> cameras;
  std::vector<std::string> image_names;
  // flattened acceleration structure
  std::vector<DevNode> nodes;
  std::vector<DevPrim> prims;
  std::vector<float> normals;  // 4 per leaf
  std::vector<LeafSource> leaf_src;
  std::vector<int> leaf_object;  // per DFS leaf: leaf_src[leaf].object (uploaded for ray queries)
  int root_kind = kRootNode;
  int root_ref = 0;
  float root_box[6] = {0, 0, 0, 0, 0, 0};
  int depth = 0;  // internal-node levels
  // culling tree over reference treelets (accel_build.cpp), FAST traversal only
  int accel_root = -1;   // tagged index into nodes (8-wide nodes follow the reference's), -1 = none
  int accel_depth = 0;   // stack entries a traversal from accel_root can need
  int accel_items = 0;   // treelets
  int accel_stride = 0;  // node slots from one octant copy of the culling nodes to the next (0: no culling tree)
  float accel_box[6] = {0, 0, 0, 0, 0, 0};
  // per-axis outward margin of every culling box: 2^-18 * the largest coordinate magnitude of
  // the scene, its cameras and every ray origin; it lets the kernels cull on
  // a plain slab test
  double cull_margin[3] = {0, 0, 0};
  std::vector<DevLeaf> leaves;        // culling-tree order (DevLeaf)
  std::vector<DevAncestry> ancestry;  // max(nodes, leaves) entries, see DevAncestry
  int quot_ok = 0;  // every triangle v0 coordinate passes quot_coord_ok (rt_internal.h)
  // surface data (build_surface): empty unless a mesh is smooth or the caller
  // gave texture coordinates
  bool smooth = false;                // some mesh is smooth
  std::vector<int> leaf_tri;          // 4 per DFS leaf: i0 i1 i2 flags (kSurfSmooth); a sphere: 0
  std::vector<float> vertex_normals;  // 4 per vertex (smooth scenes)
  std::vector<float> vertex_uv;       // 2 per vertex (scenes with uv)
  // image textures (build_textures): empty unless some object names a texture.
  // A textured scene has leaf_tri, with each leaf's texture id + 1 above the smooth bit, and one
  // material more than the description's: blank_material, all zero, for REPLACE_ALL hits.
  std::vector<DevTexture> textures;
  std::vector<uint32_t> texels;       // every texture's texels, 4 bytes each
  int blank_material = -1;
};

// The vertex normals of HW3/src/Scene.cpp:690-695 and 870-876 (the rule in ceng795_rt.h) into
// out[3 * num_vertices]; throws std::invalid_argument on a bad description.
void host_vertex_normals(const rt_scene_desc& desc, float* out);
// The surface data of a built scene (s made from desc by build_host_scene); surf may be null.
void build_surface(const rt_scene_desc& desc, const rt_surface_desc* surf, HostScene& s);
// The textures of a built scene (after build_surface with the same `surf`); tex may be null.
// Checks the descriptor (std::invalid_argument).  No object with a texture: s is left as it was.
void build_textures(const rt_scene_desc& desc, const rt_surface_desc* surf,
                    const rt_texture_desc* tex, HostScene& s);
// The descriptor's textures, checked, as the device table and the 4-byte texel blob.
void pack_textures(const rt_texture_desc& tex, std::vector<DevTexture>& table,
                   std::vector<uint32_t>& texels);
// tex_get_color for n queries; a texture id out of range gives 0 0 0.
void host_texture_lookup(const std::vector<DevTexture>& table, const std::vector<uint32_t>& texels,
                         const rt_tex_query* q, long long n, float* rgb);

// Cuts the reference tree into treelets of <= K leaves (K = 1: lone leaves; 2: also leaf
// pairs; K <= 0: no culling tree) and appends an 8-wide SAH tree over them.  Leaves the
// reference nodes, leaves and tie-break order untouched.
// The culling nodes are stored kOctantCopies times, once per octant (rt_internal.h).  Throws
// std::domain_error when the node array would pass kMaxNodeSlots.
void build_accel(HostScene& s, int K);
// "" when a scene of ref_slots reference node slots and wide_slots culling node slots (one copy)
// fits the kernels' 32-bit node offsets, else the error build_accel reports.
std::string accel_slots_error(size_t ref_slots, size_t wide_slots);
// Invariants of the culling tree (coverage, guard boxes, conservative containment with the
// margin, child layout, ancestry); "" if they hold.  stats: treelets, culling nodes, culling
// depth, lone-leaf treelets.
std::string check_accel(const HostScene& s, int K, long long stats[4]);
// hist[v] = culling nodes with v valid slots (a tree that passed check_accel).
void accel_slot_histogram(const HostScene& s, long long hist[kWideSlots + 1]);
// hist[9 * i + l] = culling nodes with i inner and l leafy slots (a tree that passed check_accel).
void accel_kind_histogram(const HostScene& s, long long hist[(kWideSlots + 1) * (kWideSlots + 1)]);
// The slot order of one wide node (rt_internal.h DevNode8), part of check_accel: "" or the
// broken rule.
std::string wide_slot_order_error(const DevNode8& W);

// Entry cuts (entry_cuts.cpp): per frame tile of camera c, kEntryCut tagged
// references to culling nodes of octant copy 0 (-1 pads the unused places) that together hold every
// leaf a pixel ray of the tile can reach; the frame kernel's primary walk starts at them instead of
// the root.  Decided on the host from the tile's frustum alone, with no test in the kernel.
// stats (may be null): see the kEc* indices.
enum : int {
  kEcTiles = 0,        // tiles
  kEcBySize = 0,       // [kEcBySize + n], n = 1 .. kEntryCut: tiles whose cut has n nodes
  kEcSavedVisits = 6,  // culling nodes above the cuts, summed over the tiles (visits no walk makes)
  kEcSavedSlots = 7,   // ... and their valid slots
  kEcByDepth = 8,      // [kEcByDepth + d]: tiles whose shallowest cut node lies d levels below the root
  kEntryCutDepths = 15,  // (deeper ones count in the last)
  kEcToRoot = 23,      // tiles the sign / skip rule sent to the root
  kEntryCutStats = 24
};
static_assert(kEntryCut >= 1 && kEntryCut < kEcSavedVisits, "cut sizes 1 .. kEntryCut fit the stats");
// Whether a scene gets tables at all: it has a culling tree under a node root, and the tree's
// stack bound plus kEntryCut - 1 fits the `stack_entries` of the kernel instantiation that runs.
bool entry_cuts_apply(const HostScene& s, int stack_entries);
std::vector<int> build_entry_cuts(const HostScene& s, const rt_camera& c,
                                  long long stats[kEntryCutStats]);
// Every pixel ray of every tile of camera c, walked from the root with visit_wide's per-lane slot
// test restated on the host: each leafy slot a ray enters must lie under a node of its tile's
// record.  Returns the number of (ray, slot) violations (-1: the table does not fit the camera)
// and in first[4] the first one: px, py, node slot, slot.
long long check_entry_cuts(const HostScene& s, const rt_camera& c, const std::vector<int>& table,
                           long long first[4]);

// Builds `out` from `desc`; throws std::invalid_argument on a bad description.
void build_host_scene(const rt_scene_desc& desc, HostScene& out);

// The part of build_host_scene that copies the description's scalars, materials, lights and
// cameras (what an instanced scene keeps in its HostScene; it has no flat tree).
void build_host_globals(const rt_scene_desc& desc, HostScene& out);

// An instanced scene on the host (instances.cpp): one HostScene per base mesh
// (tree, culling tree, leaves; no globals), the instance records, and the top-level reference
// tree over instances, loose triangles and spheres in that order (HW3/src/Scene.cpp:706-869).
struct InstHost {
  std::vector<HostScene> meshes;
  std::vector<int> mesh_leaf_base;    // scene-wide leaf id of each mesh's leaf 0
  std::vector<int> mesh_object_base;  // object-list index of each mesh's face 0
  std::vector<long long> accel_stats; // 4 per mesh: check_accel's stats (zeros: no culling tree)
  std::vector<DevInstance> instances;
  std::vector<float> inverse;         // 16 per instance: the whole inverse matrix
  std::vector<int> inst_top_dfs;      // per instance: its top-level DFS position
  std::vector<DevNode> top_nodes;     // leaf children: ~top-level DFS position
  std::vector<DevPrim> top_prims;     // per position (rt_internal.h InstParams)
  std::vector<float> top_normals;     // 4 per position
  std::vector<int> top_info;          // 2 per position: object index, scene-wide leaf id
  int top_root_kind = kTopNode;
  int top_depth = 0;                  // internal-node levels of the top-level tree
  int top_quot_ok = 1;
  float top_box[6] = {0, 0, 0, 0, 0, 0};
  bool has_spheres = false;
  int leaves = 0;                     // scene-wide leaf ids
  // a scene with motion (build_moving): some instance or sphere has a velocity,
  // or some sphere a matrix other than the identity
  bool has_motion = false;
  std::vector<DevMotionInstance> motion_instances;  // per instance (scenes with motion)
  std::vector<DevMotionSphere> motion_spheres;      // the kPrimMovingSphere records
  std::vector<float> sphere_inverse;  // 16 per sphere: the whole inverse of its matrix
  std::vector<float> sphere_box;      // 6 per sphere: its box in the top-level tree
  std::vector<int> object_top_dfs;    // per top-level object: its top-level DFS position
};
// Builds `out` from the description's meshes (bases only) and the instance descriptor; treelets:
// build_accel's K for every base mesh, each checked with check_accel.  Throws
// std::invalid_argument on a bad description (a singular matrix among them) and std::domain_error
// on what instanced scenes do not take (the caller's own BVH, trees deeper than the wave stack).
void build_instanced(const rt_scene_desc& desc, const rt_instance_desc& inst, int treelets,
                     InstHost& out);
// build_instanced with the motion descriptor's velocities and sphere matrices (either descriptor
// may be null; no instance: the top level is the loose primitives).  Checks the motion descriptor
// (struct_size, counts, finite entries, invertible sphere matrices: std::invalid_argument).  The
// boxes of moving objects are expanded by +-velocity (Mesh.h:104-110, Sphere.h:30-36).
void build_moving(const rt_scene_desc& desc, const rt_instance_desc* inst,
                  const rt_motion_desc* motion, int treelets, InstHost& out);
// Every velocity zero and every sphere matrix the identity (or the arrays null).  Checks the
// descriptor as build_moving does.
bool motion_trivial(const rt_scene_desc& desc, const rt_instance_desc* inst,
                    const rt_motion_desc* motion);

// load_scene_xml plus the file's instances (instances_xml.cpp): the root <Transformations> block,
// every <Mesh> as an instance with its own transformation list, then the <MeshInstance>s;
// vertexOffset is added to the meshes' vertex ids in `st`.  Throws std::domain_error on what
// instanced scenes do not take (<Transformations> on a <Triangle> or <Sphere>, a non-zero
// <MotionBlur>, plyFile).
struct XmlSceneStorage;
struct XmlInstances {
  std::vector<int> mesh, material;
  std::vector<float> transform;  // 16 per instance, row-major
  // load_instances_xml(..., motion = true) only (rt_scene_load_xml_moving): <MotionBlur> per
  // instance and per <Sphere>, and the <Sphere>s' composed <Transformations>
  std::vector<float> velocity;          // 3 per instance
  std::vector<float> sphere_transform;  // 16 per sphere
  std::vector<float> sphere_velocity;   // 3 per sphere
};
void load_instances_xml(const std::string& path, XmlSceneStorage& st, rt_scene_desc& desc,
                        XmlInstances& out, bool motion = false);

// Preorder dump in oracle/ref/ref_harness.cpp's format (without the Mesh "M" markers, which
// the flattened layout splices away).
std::string dump_bvh(const HostScene& s);

// XML ingest (HW2/Scene.cpp:198-451) into a description whose arrays live in `storage`.
struct XmlSceneStorage {
  std::vector<float> vertices;
  std::vector<rt_material> materials;
  std::vector<rt_point_light> lights;
  std::vector<rt_camera> cameras;
  std::vector<std::string> image_names;
  std::vector<int> mesh_material, mesh_face_count, mesh_faces;
  std::vector<int> triangle_indices, triangle_material;
  std::vector<int> sphere_center, sphere_material;
  std::vector<float> sphere_radius;
  // per <Mesh>: shadingMode="smooth" (HW3/src/Scene.cpp:634-639); no rt_scene_desc field points
  // here, and rt_scene_load_xml ignores it as HW2 does
  std::vector<unsigned char> mesh_smooth;
};
void load_scene_xml(const std::string& path, XmlSceneStorage& st, rt_scene_desc& desc);

// The texture part of a scene file (rt_scene_load_xml_textured; HW4/src/Scene.cpp:690-701,
// 761-768, 905-911, 1008-1014, 1030-1077): <TexCoordData> as pairs, the root <Textures> block with
// the reference's defaults, the 1-based <Texture> child of <Mesh>, <Triangle> and <Sphere>.
// Throws std::domain_error on what textured scenes do not take (perlin, bumpmap="true",
// <BackgroundTexture>, a textured mesh whose textureOffset differs from its vertexOffset, plyFile).
struct XmlTextures {
  std::vector<std::string> image_name;
  std::vector<int> interpolation, decal, appearance;  // RT_TEX_*
  std::vector<float> normalizer;
  std::vector<int> mesh_texture, triangle_texture, sphere_texture;  // 0-based, -1: none
  std::vector<float> uv;  // 2 per <TexCoordData> pair
};
void load_textures_xml(const std::string& path, XmlTextures& out);
// The descriptor of a loaded file: its textures matched to the caller's image records by name
// (std::ios_base::failure for a name without one), the per-vertex uv (pairs by vertex id, zeros
// past the file's; std::domain_error when a textured face needs a pair the file lacks).  `tex`
// points into xt, records and uv.
void textures_from_xml(const XmlTextures& xt, const rt_scene_desc& d, const rt_texture_image* images,
                       int num_images, std::vector<rt_texture>& records, std::vector<float>& uv,
                       rt_texture_desc& tex);

// ---- scene assembly (scene_assemble.cpp): the one place that decides which kind
// of scene a set of descriptors denotes and builds everything creation derives on the host.  No
// HIP: the C ABI's creation entries run it before their first HIP call.

// What a creation entry was given.  Everything but `desc` may be null.
struct SceneInputs {
  const char* entry = "";  // the entry's name, for messages
  const rt_scene_desc* desc = nullptr;
  const rt_surface_desc* surface = nullptr;
  const rt_texture_desc* textures = nullptr;
  const rt_instance_desc* instances = nullptr;
  const rt_motion_desc* motion = nullptr;
  const std::vector<std::string>* image_names = nullptr;  // per camera (scene files)
};

// What creation derives from them.
struct SceneHost {
  HostScene host;
  // made of instances (rt_scene_create_instanced): `host` holds the scene's scalars, materials,
  // lights and cameras and no tree; the ray queries, the radiance queries and the frames (on the
  // ray-tree path, like a smooth scene's) run their INST kernels; nothing that reads the flat
  // tree takes such a scene (hit attributes, pixel records, the BVH dump)
  std::unique_ptr<InstHost> inst;
  bool deep = false;  // the flat tree needs more stack than a lane's (tree_deep)
  bool needs_recursion = false;  // some material is a mirror or a dielectric, and max_depth > 0
  bool has_spheres = false;
  // some mesh is smooth (rt_scene_create_surface): frames take the ray-tree path, as a scene that
  // recurses does, and the ray-tree and closest-hit kernels run their SMOOTH instantiations
  bool smooth = false;
  // some object has a texture (rt_scene_create_textured): frames take the ray-tree path too, and
  // the ray-tree kernels run their TEX instantiations
  bool textured = false;
  size_t most = 1;  // pixel records of the largest camera frame (whole tiles)
};

// Fills `out` (a fresh one) from `in`.  Checks the descriptors' struct_size and counts, then
// decides by the rules of ceng795_rt.h: no instance and trivial motion give the flat scene (with
// its surface data and textures, if any), instances and trivial motion the two-level scene,
// anything else the scene with motion.  A flat scene gets its culling tree (none when that tree
// would be deeper than max_tree_depth, the kernels' largest stack).  Throws what the build_*
// functions throw; std::invalid_argument for a scene of 2^26 primitives or more or a reference
// tree deeper than max_tree_depth; std::domain_error for instances or motion together with
// surface data or textures, which no entry can express.
void assemble_scene(const SceneInputs& in, int max_tree_depth, SceneHost& out);

// struct_size and num_instances of an instance descriptor (null: nothing to check);
// std::invalid_argument with `fn` in front.
void check_instance_desc(const char* fn, const rt_instance_desc* in);

// What the six scene-file entries differ in.
struct SceneFileOptions {
  bool shading_mode = false;  // honour the meshes' shadingMode (rt_scene_load_xml_surface)
  bool textures = false;      // ... and the file's textures, with the caller's images
  bool instances = false;     // every <Mesh> an instance, and the <MeshInstance>s
  bool motion = false;        // ... and <MotionBlur>, the spheres' <Transformations>
  const rt_texture_image* images = nullptr;
  int num_images = 0;
};
// A loaded scene file: `in` points into the rest, so the object stays where it is.
struct SceneFile {
  XmlSceneStorage st;
  XmlInstances xi;
  XmlTextures xt;
  std::vector<rt_texture> records;
  std::vector<float> uv;
  rt_scene_desc desc;
  rt_surface_desc surface;
  rt_texture_desc textures;
  rt_instance_desc instances;
  rt_motion_desc motion;
  SceneInputs in;
};
void load_scene_file(const char* entry, const std::string& path, const SceneFileOptions& opt,
                     SceneFile& out);

// Whether the flat tree (with its culling tree) needs the kernels' deep instantiations, and
// whether its frames get entry cuts: entry_cuts_apply with the stack of the instantiation that runs.
bool tree_deep(const HostScene& h);
bool scene_entry_cuts_apply(const HostScene& h, int max_tree_depth);

// The flat scene of a scene file, for the rt_host_* entries: load_flat_scene without a culling
// tree, flat_host_scene with build_accel(treelet_leaves)'s.  stats4 given: checked with check_accel
// (std::invalid_argument "culling tree: ..." when it fails).  max_tree_depth > 0: without the
// culling tree when it is deeper, as assemble_scene does.
void load_flat_scene(const std::string& xml_path, HostScene& out);
void flat_host_scene(const std::string& xml_path, int treelet_leaves, int max_tree_depth,
                     long long stats4[4], HostScene& out);

// `text` as the file `path`; false when the file cannot be opened.
bool write_text_file(const char* path, const std::string& text);

void camera_from_view(const float pos[3], const float gaze[3], const float up[3],
                      const float np[4], float dist, int w, int h, int ns, rt_camera& c);

}  // namespace rt

#endif
