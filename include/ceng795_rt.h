/* ceng795_rt — MI355X (gfx950) ray-trace hot path behind a C ABI.
 *
 * This is the drop-in boundary for the reference's render seam:
 *
 *   void Scene::render_image(int camera_index, Pixel* result, int starting_row,
 *                            int height_increase = 1) const;      HW2/Scene.h:34-35
 *                                                                 HW2/Scene.cpp:16-70
 *
 * The reference calls it from T host threads on a shared const Scene, each thread with a
 * disjoint row set (HW2/main.cpp:33-36).  Here the whole row set runs as one HIP launch
 * (or several callers on disjoint rows — rt_render is reentrant).  Everything up to the
 * seam stays on the host, as in the reference: XML ingest (HW2/Scene.cpp:198-451), the
 * Camera basis (HW2/Camera.h:10-29) and the BVH build (HW2/Bounding_volume_hierarchy.cpp:3-29)
 * happen in rt_scene_create / rt_scene_load_xml, untimed like the reference's Scene ctor.
 * rt_scene_create_multi spreads one scene's frames over several GPUs of the process.
 *
 * Plain C types only: no torch, no HIP types in signatures (streams are void*).
 * Every function returns 0 on success or a negative RT_E* code; the message of the last
 * failure on the calling thread is in rt_last_error().  No C++ exception crosses the ABI.
 */
#ifndef CENG795_RT_H_
#define CENG795_RT_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CENG795_RT_ABI_VERSION 7  /* 2: MSAA cameras + rt_set_msaa_seed; 3: tile ranges,
                                      kernel timing; 4: multi-device scenes, stream scratch
                                      release, no CULL mode; 5: pixel records
                                      (RT_TILE_RECORDS, rt_resolve_device); 6: rt_tile_costs,
                                      row-major records + rt_resolve_rows; 7: the caller's own
                                      BVH in rt_scene_desc (bvh_*), rt_host_dump_bvh_desc,
                                      rt_host_alloc / rt_host_free */

enum {
  RT_OK = 0,
  RT_E_INVALID = -1,  /* bad argument or scene description            */
  RT_E_HIP = -2,      /* HIP runtime error (message has the HIP text)   */
  RT_E_IO = -3,       /* file could not be read / written                */
  RT_E_PARSE = -4,    /* scene XML malformed (reference would throw/crash) */
  RT_E_UNSUPPORTED = -5
};

/* HW2/Material.h:5-13 (field order kept). */
typedef struct rt_material {
  float ambient[3];
  float diffuse[3];
  float specular[3];
  float mirror[3];
  float transparency[3];
  float refraction_index;
  float phong_exponent;
} rt_material;

/* HW2/Point_light.h:5-8 */
typedef struct rt_point_light {
  float position[3];
  float intensity[3];
} rt_point_light;

/* A camera after HW2/Camera.h:10-29's precompute: primary ray for pixel (x, y) is
 *   o = e,  d = normalize((top_left + (x+0.5)*s_u) - (y+0.5)*s_v - e).          Camera.h:30-35
 * num_samples is the per-axis sample count n = (int)sqrt(<NumSamples>) (Scene.cpp:275-276). */
typedef struct rt_camera {
  float e[3];
  float top_left[3];
  float s_u[3];
  float s_v[3];
  int width, height;
  int num_samples;
} rt_camera;

/* Scene description, flattened, 0-based, host-owned (copied by rt_scene_create).
 * Objects enter the top-level BVH in the reference's parse order: meshes, then loose
 * triangles, then spheres (HW2/Scene.cpp:380-449). */
typedef struct rt_scene_desc {
  float background[3];          /* <BackgroundColor>, default 0 0 0      */
  float shadow_ray_epsilon;     /* <ShadowRayEpsilon>, default 0.001     */
  int max_recursion_depth;      /* <MaxRecursionDepth>, default 0        */
  float ambient_light[3];       /* <Lights><AmbientLight>                */

  const float* vertices;        /* fp32[3*num_vertices]  <VertexData>    */
  int num_vertices;
  const rt_material* materials;
  int num_materials;
  const rt_point_light* lights;
  int num_lights;
  const rt_camera* cameras;
  int num_cameras;

  int num_meshes;               /* <Mesh>: material + faces              */
  const int* mesh_material;     /* int32[num_meshes]                     */
  const int* mesh_face_count;   /* int32[num_meshes]                     */
  const int* mesh_faces;        /* int32[3*sum(face_count)], vertex ids  */

  int num_triangles;            /* <Triangle>                            */
  const int* triangle_indices;  /* int32[3*num_triangles]                */
  const int* triangle_material; /* int32[num_triangles]                  */

  int num_spheres;              /* <Sphere>                              */
  const int* sphere_center;     /* int32[num_spheres], vertex id         */
  const float* sphere_radius;   /* fp32[num_spheres]                     */
  const int* sphere_material;   /* int32[num_spheres]                    */

  /* Optional (ABI 7): the caller's own BVH — e.g. the reference's Scene::bvh walked through
   * its public members (BVH::left / right / bounding_box, Mesh::bvh, Triangle::index_* /
   * normal, Sphere::center / radius; HW2/Bounding_volume_hierarchy.h:39-41, Mesh.h:12,
   * Triangle.h:12-14).  bvh_num_leaves == 0 (zero-initialised desc): the library builds the
   * reference's tree itself from the object lists (HW2/Bounding_volume_hierarchy.cpp:3-29).
   * Otherwise the library adopts this tree as given, Mesh wrappers spliced out (Mesh::intersect
   * delegates to its BVH with no box test of its own, Mesh.h:13-15):
   *   internal nodes in DFS preorder, node 0 the root (none when the root is one primitive);
   *   bvh_children[2 i + s] = child s (0 left, 1 right) of node i: >= 0 an internal node
   *     (> i), < 0 ~k for leaf k;  leaves numbered in DFS (left-first) order, which is the
   *     closest-hit tie-break order (appendix A.5 of SURVEY.md);
   *   bvh_boxes[6 i ..] = node i's Bounding_box (min xyz, max xyz) exactly as the caller holds
   *     it — these are the boxes the slab tests see;
   *   bvh_leaf_object[k] = leaf k's primitive: an index into the triangles of the object lists
   *     (mesh faces in mesh order, then loose triangles) or, past them, into the spheres;
   *   bvh_leaf_normals: NULL, or fp32[3 bvh_num_leaves] = each triangle leaf's flat normal as
   *     the caller computed it (Triangle.cpp:14; sphere leaves: ignored).
   * Every leaf index and every primitive must occur exactly once. */
  int bvh_num_nodes;
  const int* bvh_children;      /* int32[2*bvh_num_nodes]                */
  const float* bvh_boxes;       /* fp32[6*bvh_num_nodes]                 */
  int bvh_num_leaves;
  const int* bvh_leaf_object;   /* int32[bvh_num_leaves]                 */
  const float* bvh_leaf_normals;/* fp32[3*bvh_num_leaves] or NULL        */
} rt_scene_desc;

/* Work counters for one render call. */
typedef struct rt_stats {
  long long primary_rays;
  long long shadow_rays;
  long long secondary_rays;
  long long primary_hits;
  double kernel_ms;             /* HIP-event time of the render kernel(s)  */
} rt_stats;

/* Traversal modes.  Both give the reference's result on every input. */
enum {
  RT_TRAVERSAL_FAST = 0,        /* culling tree over reference treelets, near-first order,
                                   batched leaf tests (default)                               */
  RT_TRAVERSAL_REFERENCE = 1    /* visits every box the reference visits, in its order        */
};
typedef struct rt_scene rt_scene;

/* Replaces Scene::Scene's object + BVH construction (HW2/Scene.cpp:378-449 and
 * Bounding_volume_hierarchy.cpp:3-29).  `device` < 0 = the calling thread's current HIP
 * device.  Uploads the flattened scene to that device. */
int rt_scene_create(const rt_scene_desc* desc, int device, rt_scene** out);
void rt_scene_destroy(rt_scene* scene);

/* Host convenience: HW2/Scene.cpp:198-451's XML ingest, then rt_scene_create. */
int rt_scene_load_xml(const char* xml_path, int device, rt_scene** out);

/* One scene over several GPUs of this process (the reference's T render
 * threads, HW2/main.cpp:33-36, become the devices of one node).  The scene is built once on
 * the host and replicated on devices[0 .. device_count-1] (NULL: devices 0 .. device_count-1);
 * devices[0] holds the output.  rt_render / rt_render_device on such a scene deal the frame's
 * 8x8 tiles round-robin over the devices (tile t -> device t mod device_count), render every
 * share on its own device, gather the shares onto devices[0] with RCCL (one communicator per
 * device, ncclCommInitAll; send / receive pairs in one group, over xGMI) and untile them there.
 * Pixels are the single-device ones bit for bit.  MSAA cameras (whose 3x3 splat crosses tile
 * borders, HW2/Scene.cpp:51-63) split by bands of rows instead: device d owns rows
 * [H*d/n, H*(d+1)/n), renders every sample pass over its band plus a one-row halo each side,
 * resolves its band, and the bands are gathered the same way.
 * Frames of one multi-device scene are serialised (its RCCL communicators are shared). */
int rt_scene_create_multi(const rt_scene_desc* desc, int device_count, const int* devices,
                          rt_scene** out);
int rt_scene_load_xml_multi(const char* xml_path, int device_count, const int* devices,
                            rt_scene** out);
int rt_scene_device_count(const rt_scene* scene);

int rt_scene_num_cameras(const rt_scene* scene);
int rt_scene_camera(const rt_scene* scene, int camera_index, rt_camera* out);
/* Output file name of a camera's <ImageName> (loaded scenes only; "" otherwise). */
const char* rt_scene_image_name(const rt_scene* scene, int camera_index);
int rt_scene_num_lights(const rt_scene* scene);
/* Preorder BVH dump (oracle/ref/ref_harness.cpp `bvh` format) for topology parity. */
int rt_scene_dump_bvh(const rt_scene* scene, const char* path);
/* Host-only variant for tests without a GPU: XML ingest + BVH build + flatten, then the
 * same dump.  Touches no HIP API. */
int rt_host_dump_bvh_xml(const char* xml_path, const char* out_path);
/* Host-only, for tests without a GPU: the same dump for a scene description (with or without
 * the caller's own BVH, bvh_*).  Touches no HIP API. */
int rt_host_dump_bvh_desc(const rt_scene_desc* desc, const char* out_path);
/* Host-only, for tests: XML ingest + BVH build + the culling tree over reference treelets of
 * <= treelet_leaves leaves, then a check of the invariants the kernels'
 * exactness rests on (every leaf in exactly one treelet, guard boxes = the reference boxes
 * they stand for, culling boxes contain every guard box below them, ancestry links).
 * stats4: treelets, culling nodes, culling-tree depth, lone-leaf treelets (zeros when the
 * tree is a single treelet).  RT_E_INVALID with the violation in rt_last_error(). */
int rt_host_check_accel_xml(const char* xml_path, int treelet_leaves, long long* stats4);
/* Host-only: builds and checks the culling tree as above, then hist9[v] = its 8-wide nodes with
 * v valid slots (v = 0..8; all zero when the tree is a single treelet). */
int rt_host_accel_slot_hist_xml(const char* xml_path, int treelet_leaves, long long* hist9);
/* Host-only: builds and checks the culling tree as above, then hist81[9 * i + l] = its 8-wide
 * nodes with i inner and l leafy slots (i, l = 0..8). */
int rt_host_accel_kind_hist_xml(const char* xml_path, int treelet_leaves, long long* hist81);
/* Host-only, for tests: the slot-order rule of one 8-wide node record (128 bytes)
 * as the culling-tree check applies it to every node: inner slots contiguous from slot 0, leafy
 * slots contiguous down from slot 7, nothing valid between them, the two counts in the top byte
 * of `kinds` equal to the bits, NaN planes in the invalid slots.  RT_E_INVALID with the broken
 * rule in rt_last_error(). */
int rt_host_check_wide_node(const void* node, unsigned long long bytes);
/* Host-only: the size rule a scene's node array must pass (the kernels address culling nodes by
 * 32-bit byte offset, and the culling nodes are stored once per direction-sign octant, DESIGN.md
 * §3): RT_OK when ref_slots reference node slots and wide_slots culling node slots (one copy) fit,
 * else RT_E_UNSUPPORTED with the message scene creation fails with in rt_last_error(). */
int rt_host_accel_slots_check(long long ref_slots, long long wide_slots);
/* Host-only, for tests: the frame kernel's index arithmetic, which divides by multiplying with
 * host-computed constants — the functions the kernel itself runs.
 * rt_host_packet_div: quot[i] = (first + i) / divisor by that arithmetic, i < count
 * (divisor >= 1, first + count <= 2^31).
 * rt_host_packet_coords: for a launch of num_sel_tiles selected units (tiles tile_begin + k
 * tile_step of a frame tiles_x tiles wide; with block_deal 2x2 blocks in deal order, four tiles
 * each) and every logical packet p < count: out4[4p] = the selected tile wave p takes in block
 * order (-1: none), out4[4p+1], out4[4p+2] = its tile column and row, out4[4p+3] = the order-list
 * word workgroup p reads in an ordered launch of order_regions regions, order_stride words each.
 * Returns the launch's logical packets, or an error. */
int rt_host_packet_div(int divisor, int first, int count, int* quot);
int rt_host_packet_coords(int tiles_x, int num_sel_tiles, int tile_begin, int tile_step,
                          int block_deal, int order_regions, int order_stride, int count,
                          int* out4);
/* Host-only, for tests: the frame kernel's scaled visit time — the functions the
 * launch and the kernel themselves run.
 * rt_host_visit_time_exp: the exponent E a frame launch takes for a culling-tree root box
 * box6 = {lo xyz, hi xyz} and a camera position cam3; INT_MIN on a NULL argument.
 * rt_test_visit_time_exp: on != 0 makes every later frame launch of the process take for 2^E the
 * largest power of two not above 2^rel times the root box's diagonal (frames must not change:
 * too small an E only costs culling); on == 0 restores the rule. */
int rt_host_visit_time_exp(const float* box6, const float* cam3);
int rt_test_visit_time_exp(int on, int rel);
/* Host-only, for tests and tools: the entry cuts of camera `cam` of a scene file —
 * per 8x8 frame tile, row-major, RT_ENTRY_CUT_NODES references to culling-tree nodes (tagged node
 * slots of octant copy 0, -1 in the unused places) at which the frame kernel starts the tile's
 * primary walk, built by the function scene creation runs.
 * rt_host_entry_cuts_xml returns the table's length in ints, tiles x RT_ENTRY_CUT_NODES, and
 * copies it to `out` when capacity holds it (out may be NULL); 0: the scene gets no table (no
 * culling tree, a root that is a primitive, or a tree too deep for the walk's stack); < 0: an
 * error.  stats24 (may be NULL): [0] tiles, [n] tiles whose cut has n nodes (n = 1 ..
 * RT_ENTRY_CUT_NODES), [6] culling nodes above the cuts summed over the tiles (the visits the
 * walks no longer make) and [7] their valid slots, [8 + d] tiles whose shallowest cut node lies d
 * levels below the root (d >= 14 in [22]), [23] tiles kept at the root because their frustum
 * holds a direction with a zero or nearly zero component.
 * rt_host_check_entry_cuts_xml builds the same table and walks every pixel ray of every tile from
 * the root with the kernel's per-lane slot test restated on the host; every leafy slot a ray
 * enters must lie under a node of its tile's record.  *violations = the (ray, slot) pairs that do
 * not, first4 (may be NULL) = the first one's pixel x, y, node slot and slot.  Returns as above.
 * rt_test_entry_cuts: mode 1 makes every later launch of the process walk from the root (frames
 * must not change), 0 restores the default. */
#define RT_ENTRY_CUT_NODES 4
int rt_host_entry_cuts_xml(const char* xml_path, int treelet_leaves, int cam, int* out,
                           long long capacity, long long* stats24);
int rt_host_check_entry_cuts_xml(const char* xml_path, int treelet_leaves, int cam,
                                 long long* violations, long long* first4);
int rt_test_entry_cuts(int mode);
/* Height of the flattened BVH (levels of internal nodes). */
int rt_scene_bvh_depth(const rt_scene* scene);

int rt_set_traversal(rt_scene* scene, int mode);

/* Scene::render_image(camera_index, result, starting_row, row_stride) with NumSamples == 1
 * (HW2/Scene.cpp:24-31).  Writes fp32 RGB radiance — exactly Pixel::color after the
 * reference's add_color(color, 1) — for rows j = starting_row + k*row_stride into
 * out_rgb[3*(j*width + i)] (w*h*3 floats, row-major, top row first).  Other rows are left
 * untouched.  Synchronous; safe to call concurrently on one scene from several threads.
 *
 * NumSamples > 1 (jittered MSAA + 3x3 Gaussian splat, HW2/Scene.cpp:32-69): whole frames
 * only (starting_row 0, row_stride 1, else RT_E_UNSUPPORTED).  out_rgb is then
 * Pixel::color / Pixel::weight, the value Pixel::get_color truncates (HW2/Pixel.h:17-27),
 * with the splat summed in the single-threaded reference order.  The reference seeds each
 * pixel's std::default_random_engine from the wall clock; here it is seeded with
 * splitmix64(msaa_seed, j*width + i) (rt_set_msaa_seed, default 0), so frames are
 * reproducible.  rt_stats counts every sample's rays. */
int rt_render(rt_scene* scene, int camera_index, int starting_row, int row_stride,
              float* out_rgb, rt_stats* stats);

/* Page-locked host memory for rt_render's out_rgb (ABI 7): the frame kernel writes such a buffer
 * directly through its device-visible address, with no device-to-host copy afterwards (any
 * pinned buffer, e.g. torch's pin_memory, gets the same path).  NULL on failure
 * (rt_last_error). */
void* rt_host_alloc(size_t bytes);
void rt_host_free(void* ptr);

/* tile_major flags of rt_render_device / rt_render_device_range */
enum { RT_TILE_MAJOR = 1, RT_TILE_BLOCKS = 2,
       RT_TILE_RECORDS = 4  /* each pixel as one 32-bit pixel record (the primary hit's
                               primitive and the shadow bits) instead of 3 floats — a third of the
                               bytes for the framebuffer exchange; the gathering rank shades the
                               records: tile-major shares with rt_resolve_device, row-major ones
                               (no RT_TILE_MAJOR: a 4-B word per pixel at py * width + px) with
                               rt_resolve_rows.  Only where rt_scene_records_ok. */ };

/* Device-resident variant (the building block of the one-process-per-GPU image tiling, and
 * of frames kept in HBM).  The image (rows starting_row +
 * k*row_stride) is cut into 8x8 tiles; this call renders the deal units
 * tile_begin, tile_begin + tile_step, ... into d_out (device memory).  A deal unit is
 *   one tile, tiles numbered row-major (tile_major without RT_TILE_BLOCKS), or
 *   with RT_TILE_BLOCKS one 2x2 block of tiles, blocks numbered row-major with block row by
 *   rotated left by by (unit d = by*nbx + (bx - by) mod nbx, nbx = ceil(tiles_x / 2)); a
 *   block's tiles are taken in the order (0,0) (1,0) (0,1) (1,1).  This is the deal the
 *   multi-GPU paths use: a share keeps whole blocks (the traversal workgroup's unit, so the
 *   rays of a workgroup stay neighbours) and a deal d = r (mod N) takes diagonal stripes.
 * Output (tile_major & RT_TILE_MAJOR):
 *   0: d_out is a full w*h*3 frame, written in place;
 *   1: d_out holds the selected units' tiles back to back, 8*8*3 floats each (pixels or
 *      block tiles outside the image are written as 0).
 * MSAA cameras: only the whole frame, row-major (tile_begin 0, tile_step 1, tile_major 0).
 * Asynchronous on `hip_stream` (a hipStream_t, NULL = default stream).  Ray counts
 * accumulate on the device until rt_collect_stats.  Calls on one stream run in order and share
 * that stream's scratch buffers (hit records, occlusion bits, tile schedule); each further
 * stream a scene renders on gets scratch of its own, so frames on different streams may be
 * in flight at the same time (their outputs must not overlap); host threads may enqueue
 * concurrently.  A stream's scratch lives until rt_release_stream_scratch or the scene's
 * destruction.  Multi-device scenes: whole frames only (tile_begin 0, tile_step 1,
 * tile_major 0; row subsets allowed), d_out and hip_stream on devices[0]; every caller stream
 * gets a context (device stream + buffers) of its own on each device, kept until
 * rt_release_stream_scratch, so frames on different caller streams overlap on every device. */
int rt_render_device(rt_scene* scene, int camera_index, int starting_row, int row_stride,
                     int tile_begin, int tile_step, int tile_major, float* d_out,
                     void* hip_stream);
/* rt_render_device restricted to the first `tile_count` selected deal units (tile_count < 0:
 * all): units tile_begin + k*tile_step for k < tile_count.  With RT_TILE_MAJOR the k-th tile
 * rendered lands at d_out + k*192 floats (4 tiles per unit with RT_TILE_BLOCKS).  Lets a rank render its share of a frame in chunks and hand each
 * chunk to the framebuffer gather while the next one renders (multi-GPU).
 * MSAA cameras: whole frames only. */
int rt_render_device_range(rt_scene* scene, int camera_index, int starting_row, int row_stride,
                           int tile_begin, int tile_step, int tile_count, int tile_major,
                           float* d_out, void* hip_stream);
/* The other half of the process-per-GPU tile deal: rank 0 holds every rank's share as
 * d_gathered[devices][slot][8*8*3] (rank r rendered the frame's deal units u with
 * (u + tile_offset) mod devices == r, tile-major, in order, into its slot of `slot` tiles — what
 * one equal-size gather of rt_render_device(tile_begin, tile_step = devices, RT_TILE_MAJOR
 * [| RT_TILE_BLOCKS with RT_UNTILE_BLOCKS]) outputs leaves; with blocks, slot is a multiple of
 * 4);
 * this writes them into the row-major frame d_out (rows starting_row + k*row_stride of
 * camera_index), one wave per tile, on hip_stream (device devices[0] of the scene).  Replaces
 * nothing in the reference (its threads share one Pixel array, HW2/main.cpp:33-36): it is the
 * gather's inverse. */
int rt_untile_device(rt_scene* scene, int camera_index, int starting_row, int row_stride,
                     int devices, int slot, int tile_offset, int flags, const float* d_gathered,
                     float* d_out, void* hip_stream);
/* rt_untile_device flags */
enum { RT_UNTILE_BLOCKS = 1,    /* the units are 2x2 blocks (shares rendered with RT_TILE_BLOCKS) */
       RT_UNTILE_SKIP_ROOT = 2  /* rank 0's units are not touched: the gathering rank rendered its
                                   own share in place into d_out (tile_major without
                                   RT_TILE_MAJOR), so its slot need not be gathered */ };
/* 1 when camera_index of the scene can exchange pixel records (RT_TILE_RECORDS): a pixel-centre
 * camera, no mirror/dielectric recursion, at most 4 point lights; else 0. */
int rt_scene_records_ok(const rt_scene* scene, int camera_index);
/* rt_untile_device for shares rendered with RT_TILE_RECORDS: d_gathered holds
 * [devices][slot][8*8] 32-bit pixel records; each is shaded into its pixel of the row-major
 * frame d_out — the colour the rank that traced it would have written, bit for bit (the hit's
 * distance is re-derived by the same intersection arithmetic).  Same layout and flags as
 * rt_untile_device.  This is the shading step of Scene::trace_ray (HW2/Scene.cpp:101-138)
 * moved to the gathering GPU. */
int rt_resolve_device(rt_scene* scene, int camera_index, int starting_row, int row_stride,
                      int devices, int slot, int tile_offset, int flags,
                      const unsigned* d_gathered, float* d_out, void* hip_stream);
/* The measured cost of every tile of the last frame rt_render_device enqueued on `hip_stream`
 * (single-device scenes, pixel-centre cameras without recursion): each 8x8 packet's time from
 * its first traversal step to its shading, in ticks of the 100 MHz device clock, in the order
 * of that call's tile selection (row-major tiles for a whole frame).  Waits for the stream;
 * writes at most `capacity` values to host memory and returns how many it wrote.  The row bands
 * of the multi-GPU frame split are cut from these (dist_tiles.BandPlan).  Nothing in the
 * reference measures work; its threads take interleaved rows (HW2/main.cpp:33-36). */
int rt_tile_costs(rt_scene* scene, void* hip_stream, unsigned* host_out, int capacity);
/* Row-major pixel records (rt_render_device with RT_TILE_RECORDS and no RT_TILE_MAJOR: one
 * 32-bit word per pixel at py * width + px of d_records) shaded into rows [row_begin, row_end)
 * of the row-major frame d_out — bit for bit the colours the tracing rank would have written.
 * The band split's rank 0 runs it over the rows the other ranks sent (dist_tiles.BandPlan). */
int rt_resolve_rows(rt_scene* scene, int camera_index, int row_begin, int row_end,
                    const unsigned* d_records, float* d_out, void* hip_stream);
/* Waits for `hip_stream` and frees the scratch rt_render_device keeps for it (no-op for a
 * stream the scene never rendered on).  Streams that come and go should release theirs. */
int rt_release_stream_scratch(rt_scene* scene, void* hip_stream);
/* Per-kernel timing of render launches: while enabled, every launch records HIP events around
 * its kernels on the launch's stream.  rt_read_kernel_times returns (and resets) the summed
 * milliseconds ms4 = {frame kernel (primary rays, shadow rays and shading of every packet; or
 * the recursive kernel), order kernel (the next frame's dispatch order), other (0), all} and
 * the number of launches timed. */
int rt_set_kernel_timing(rt_scene* scene, int enable);
int rt_read_kernel_times(rt_scene* scene, double* ms4, long long* launches);
/* Seed of the per-pixel MSAA generators (see rt_render).  Replaces the reference's
 * system_clock seed (HW2/Scene.cpp:36-37) to make MSAA frames deterministic. */
int rt_set_msaa_seed(rt_scene* scene, unsigned long long seed);
int rt_num_tiles(const rt_scene* scene, int camera_index, int starting_row, int row_stride);
/* Reads (and resets) the device ray counters accumulated by rt_render_device calls. */
int rt_collect_stats(rt_scene* scene, rt_stats* stats);

/* Sums (and resets) all 16 device counter columns: [0] primary rays [1] shadow rays
 * [2] secondary rays [3] primary hits; RT_DIAG builds (libceng795_rt_diag.so) add packet-level
 * work: [4..7] primary node visits / active lanes summed over visits / leaf visits / leaf
 * lane tests, [8..11] the same for shadow rays, [12] lanes that fell back to the exact slab
 * test (node boxes and leaf guards), [13] leaf-batch guard tests (primary + shadow),
 * [14] / [15] the primary / shadow node visits that were 8-wide culling nodes (included in
 * [4] / [8]).
 * Returns 1 for a diagnostic build, 0 otherwise (columns 4..15 then read 0). */
int rt_debug_counters(rt_scene* scene, long long* out16);

/* RT_TIMELINE experiment builds (tools/timeline.py): copies and clears the per-wave start/end
 * ticks (100 MHz clock) and tile of the last traversal launches, out[2 kernels][2^18 waves][3].
 * Returns the number of values written (0 in other builds) or a negative RT_E_* code. */
long long rt_debug_timeline(unsigned long long* out, long long max_values);

/* RT_DIAG builds (tools/phases.py): copies and clears the per-phase attribution of the frame
 * kernel — per traversal kind (primary, shadow) the visit loop's events (visits, slots tested,
 * slot hits, leafy / pair / inner hits, stack pushes and pops, leaf-batch flushes and their
 * 64-test iterations), then shader-clock cycle sums per phase (rt_internal.h kPh*).  Returns the
 * number of values written (0 in other builds) or a negative RT_E_* code. */
long long rt_debug_phases(unsigned long long* out, long long max_values);

/* The HIP runtime's occupancy query for the frame kernel as a culling-tree scene without spheres
 * runs it (the benchmark's C3), on `device`: out4 = workgroups per CU, waves per CU, static LDS
 * bytes per workgroup, VGPRs per lane. */
int rt_debug_frame_occupancy(int device, int* out4);

/* Device self-check of the triangle test's shared-reciprocal quotients (rt_kernels.hip,
 * tri_quotients) against IEEE division on `count` seeded random operand pairs of the fast
 * range; out2[0] = mismatching quotients (must be 0), out2[1] = cases run. */
int rt_debug_quotient_check(int device, unsigned long long seed, long long count,
                            long long* out2);

/* The same check with a mode.  Mode 0 is rt_debug_quotient_check (out4[2], out4[3] stay 0).
 * Mode 1 checks the shading's forms of the shared reciprocal (normalize_shared, light_quotients)
 * on `count` seeded random cases, each a vector to normalise and six numerators over one divisor,
 * with zero components, components below 2^-49, lengths and divisors outside [2^-40, 2^40] and
 * all-ones mantissas among them: out4[0] = cases with a quotient that differs from IEEE division
 * in any bit (must be 0), out4[1] = cases run, out4[2] = helper calls that took the shared
 * reciprocal, out4[3] = calls that took `/`. */
int rt_debug_quotient_check_mode(int device, int mode, unsigned long long seed, long long count,
                                 long long* out4);

/* ---- Ray queries: closest hit and occlusion for the caller's own rays -------------------------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_RAY_QUERY / rt_ray_query_version).
 * The frame calls answer "what colour is pixel (x, y) of camera c"; these trace any ray the
 * caller generates — area-light, lens, glossy or path-tracing rays of the later homeworks, or
 * a caller's own shading — through the same intersection rule (HW2/Bounding_volume_hierarchy.cpp,
 * Triangle.cpp, Sphere.h):
 *
 *   closest hit  ray i's result is what Scene::trace_ray's bvh->intersect(ray, hit) yields: the
 *                minimum of (t, DFS leaf) over the leaves the ray may reach with 0 < t < inf, or,
 *                when the scene's root is one primitive, that primitive's own rule (a lone sphere
 *                reports its negative root).  tmax is ignored.
 *   occlusion    1 iff some leaf the ray may reach has 0 < t < tmax (the shadow-ray test of
 *                HW2/Scene.cpp:123-127 with tmax = dist - eps); tmax <= 0 or NaN gives 0.
 *
 * Both honour rt_set_traversal (both modes give the same bits) and are independent per ray: a
 * ray's result does not depend on n, its position in the batch, its neighbours or `flags`.
 * d need not be normalised (t is in units of d).  A ray is INVALID when a component of o or d is
 * not finite, or when all three |d_i| < 1e-6; it reports a miss / 0 and does not disturb other
 * rays.  The all-zero direction is the one deliberate departure from the reference, whose slab
 * test would skip every axis and test every leaf for such a ray (it never builds one); with one
 * or two |d_i| < 1e-6 the ray is valid and those axes are skipped as in HW2/bounding_box.cpp:21.
 *
 * RT_QUERY_REORDER: the library first groups similar rays (by origin cell and quantised
 * direction, one counting sort on the device) so the 64 rays of a wave walk similar paths; the
 * results are bit-identical with and without it, and land in the caller's order either way.
 *
 * rays, hits: 16-byte aligned.  n == 0 succeeds and launches nothing; n < 0, an unknown flag
 * bit, a NULL pointer with n > 0 or a misaligned pointer is RT_E_INVALID.  Multi-device scenes:
 * RT_E_UNSUPPORTED.  The ray counters of rt_stats are not touched. */
#define CENG795_RT_HAS_RAY_QUERY 1
int rt_ray_query_version(void); /* 1 */

typedef struct rt_ray {      /* 32 B */
  float o[3];  float tmax;   /* tmax: occlusion queries only */
  float d[3];  float pad;    /* d need not be normalised     */
} rt_ray;
typedef struct rt_ray_hit {  /* 32 B */
  float t;        /* the reference's Hit_data::t; +inf on a miss                     */
  int   object;   /* index in the object lists, bvh_leaf_object's numbering; -1 miss */
  int   material; /* -1 miss                                                         */
  int   leaf;     /* DFS leaf index = the closest-hit tie-break key; -1 miss         */
  float normal[3];/* Hit_data::normal: flat triangle normal (a smooth mesh's face: the
                     interpolated vertex normal, "Surface data" below), or
                     (o + d*t - center).normalize() for a sphere; 0 0 0 on a miss    */
  int   pad;
} rt_ray_hit;
enum { RT_QUERY_REORDER = 1 };

/* Device-resident variants: d_rays / d_hits / d_occ are device memory of the scene's device.
 * Asynchronous on `hip_stream`; they use that stream's scratch like rt_render_device (the
 * reorder stage's buffers live there), so calls on one stream run in order and may interleave
 * with frames, different streams may be in flight together, and rt_release_stream_scratch
 * frees the scratch.  d_occ: one byte per ray, 0 or 1. */
int rt_trace_rays_device(rt_scene* scene, const rt_ray* d_rays, long long n, rt_ray_hit* d_hits,
                         int flags, void* hip_stream);
int rt_occluded_device(rt_scene* scene, const rt_ray* d_rays, long long n, unsigned char* d_occ,
                       int flags, void* hip_stream);
/* Host variants, synchronous: upload, run, download. */
int rt_trace_rays(rt_scene* scene, const rt_ray* rays, long long n, rt_ray_hit* hits, int flags);
int rt_occluded(rt_scene* scene, const rt_ray* rays, long long n, unsigned char* occ, int flags);
/* Host-only, touches no HIP API: for each DFS leaf of the description's tree (built by the
 * library, or the caller's own bvh_*: then it is bvh_leaf_object) its index in the object lists
 * — what rt_ray_hit::object reports for rt_ray_hit::leaf.  Writes min(leaves, capacity) values
 * (out may be NULL with capacity 0) and returns the leaf count, or a negative RT_E_* code. */
int rt_host_leaf_objects_desc(const rt_scene_desc* desc, int* out, int capacity);

/* ---- Radiance queries: Scene::trace_ray for the caller's own rays -----------------------------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_RADIANCE_QUERY /
 * rt_radiance_query_version).  The ray queries above return (t, normal, material) and leave the
 * shading to the caller; these run the library's own — ambient and the point lights with their
 * shadow rays, the mirror and dielectric recursion, the fp64 pow / exp / log, the background rule
 * — for any ray: a thin-lens or fisheye camera, an anti-aliasing pattern, or the continuation
 * ray of a caller-side bounce.
 *
 *   value     ray i's rgb is 0.0f + Scene::trace_ray(Ray(o, d, in_medium), depth)
 *             (HW2/Scene.cpp:88-196): Pixel::color after add_color(c, 1) onto a zeroed pixel, so a
 *             camera's pixel rays give that camera's frame bit for bit.  t is the first hit's
 *             Hit_data::t, +inf on a miss — the bits of rt_ray_hit::t, a lone root sphere's
 *             negative root included.  rt_ray::tmax and rt_ray::pad are ignored; d is used as
 *             given (the reference normalises only where trace_ray does).
 *   depth     -1: the scene's MaxRecursionDepth; 0 .. MaxRecursionDepth: the reference's
 *             current_recursion_depth; anything else is RT_E_INVALID.  A first-ray miss returns
 *             the background only when depth equals the scene's maximum (Scene.cpp:96-99), else
 *             black.  A continuation ray goes back in at depth - 1.
 *   flags     RT_QUERY_IN_MEDIUM: every ray of the batch starts with in_medium = true, so local
 *             shading is skipped at its first hit (Scene.cpp:107) — per call, not per ray: split
 *             the batch.  rt_trace_rays* / rt_occluded* refuse this bit like any unknown one.
 *             RT_QUERY_REORDER: as above; results are bit-identical with and without it and land
 *             in the caller's order.
 *
 * A ray's result does not depend on n, its position, its neighbours, the flags other than
 * RT_QUERY_IN_MEDIUM, the traversal mode or the scratch limit.  Invalid rays (defined above) stay
 * inactive, report (0, 0, 0, +inf) and disturb no other ray.  rays, out: 16-byte aligned; n == 0
 * launches nothing; n < 0, an unknown flag bit, a NULL pointer with n > 0 or a misaligned pointer
 * is RT_E_INVALID before any HIP call.  Multi-device scenes: RT_E_UNSUPPORTED.
 *
 * Counters: the device variant adds to the scene's device counters (rt_collect_stats): primary
 * rays = the valid rays traced; primary hits, shadow rays and secondary rays as for
 * rt_render_device.  The host variant fills *stats (nullable) with the call's own counts and the
 * HIP-event time of its kernels.
 *
 * Streams and scratch: the rules of rt_trace_rays_device.  A query that can recurse (depth > 0 and
 * a material with a non-zero mirror or transparency) keeps (depth + 1) x 28 floats of ray-tree
 * frames per ray in the stream's scratch and runs in chunks of whole waves whose frames stay under
 * the scratch limit: 256 MiB unless rt_set_radiance_scratch_limit sets another (0: the default
 * again; a limit below one wave's frames at the scene's MaxRecursionDepth is RT_E_INVALID).  A
 * query that cannot recurse allocates and touches no ray-tree scratch. */
#define CENG795_RT_HAS_RADIANCE_QUERY 1
int rt_radiance_query_version(void); /* 1 */

typedef struct rt_radiance { float rgb[3]; float t; } rt_radiance; /* 16 B */
enum { RT_QUERY_IN_MEDIUM = 2 };

int rt_shade_rays_device(rt_scene* scene, const rt_ray* d_rays, long long n, int depth,
                         rt_radiance* d_out, int flags, void* hip_stream);
int rt_shade_rays(rt_scene* scene, const rt_ray* rays, long long n, int depth, rt_radiance* out,
                  int flags, rt_stats* stats);
int rt_set_radiance_scratch_limit(rt_scene* scene, size_t bytes);
/* Bytes of ray-tree frames the scene keeps for `hip_stream`'s radiance queries and frames (0: none,
 * or a stream the scene holds no scratch for).  For tests of the no-scratch rule above. */
long long rt_stream_frame_scratch_bytes(rt_scene* scene, void* hip_stream);

/* ---- Films: filtered accumulation of the caller's own samples ---------------------------------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_FILM / rt_film_version).  The
 * radiance queries give a colour per ray; a film turns many such samples per pixel into an image
 * the way Scene::render_image's MSAA branch does (HW2/Scene.cpp:51-63, Pixel::add_color /
 * get_color), for samples the caller chose: depth of field, area lights, anti-aliasing patterns.
 * It stays in device memory, takes batch after batch and resolves to a frame.
 *
 * A film is width x height Pixels (color[3], weight) on the scene's device.  A sample is a film
 * position (x, y) in pixel units — pixel (i, j) covers [i, i+1) x [j, j+1); the reference's MSAA
 * sample of pixel i is x = (float)i + sample_x — plus an rgb.  Its SOURCE PIXEL is
 * (floor x, floor y).  It is VALID iff 0 <= x < width and 0 <= y < height as fp32 comparisons:
 * -0.0f is valid and belongs to pixel 0; NaN, +-inf, x == width and -1e-30f are not.  Invalid
 * samples are dropped and counted and disturb nothing.  (The position decides, not the pixel the
 * caller had in mind: (float)i + sample_x is i + 1 when sample_x lies within half an ulp of i below
 * 1 — about 3 samples in 10^5 at i ~ 1000 — and such a sample belongs to pixel i + 1.)
 *
 * After one splat call the film holds what a single thread would leave that started from the
 * film's state before the call, took the call's valid samples sorted by (source row, source
 * column, index in the batch) and ran Scene.cpp:51-62 for each: for the up to nine pixels
 * (ai, aj) of the source pixel's 3x3 neighbourhood inside the film,
 *     w = gaussian_filter(x - ((float)ai + 0.5f), y - ((float)aj + 0.5f), sigma)
 * (fp32 argument, double exp, double division by 2 pi sigma, narrowed), then Pixel::add_color in
 * fp32 without contraction: color = color + rgb * w, weight = weight + w.  So the result does not
 * depend on how a batch is ordered across source pixels, does depend on the order within one, and
 * two calls cut between source rows equal one call.  Calls add in sequence.
 *   RT_FILM_GAUSSIAN  sigma 0 means 1.0f / 3.0f, the reference's; the footprint is always 3x3.
 *   RT_FILM_BOX       w = 1 into the source pixel only (add_color(c, 1) of the NumSamples == 1
 *                     branch); sigma is ignored.
 * Resolve is color / weight per channel (IEEE division); a pixel with weight == 0 gives 0 0 0
 * (Pixel::get_color, HW2/Pixel.h:20).
 *
 * width, height in [1, 32768]; sigma finite and >= 0; one call takes at most 2^28 samples (cutting
 * a call by index changes the order, so the caller cuts); d_xy 8-byte aligned, d_rad / d_rays
 * 16-byte aligned; n == 0 launches nothing.  Argument errors are RT_E_INVALID before any HIP call;
 * multi-device scenes are RT_E_UNSUPPORTED.  Destroy films before their scene.
 *
 * The `_device` entries are asynchronous on `hip_stream` and use that stream's scratch (the
 * per-call sort buffers and the fused entry's radiance buffer; rt_release_stream_scratch frees
 * it).  Calls on ONE film must be ordered by the caller (one stream, or events); different films
 * on different streams overlap.  The host variants are synchronous: upload, run, download. */
#define CENG795_RT_HAS_FILM 1
int rt_film_version(void); /* 1 */

typedef struct rt_film rt_film;
enum { RT_FILM_GAUSSIAN = 0, RT_FILM_BOX = 1 };
int  rt_film_create(rt_scene* scene, int width, int height, int filter, float sigma /* 0: 1/3 */,
                    rt_film** out);
void rt_film_destroy(rt_film* film); /* NULL ok */
int  rt_film_clear_device(rt_film* film, void* hip_stream);
/* d_xy: n x 2 floats; d_rad: n rt_radiance records (t ignored). */
int  rt_film_splat_device(rt_film* film, const float* d_xy, const rt_radiance* d_rad, long long n,
                          void* hip_stream);
/* = rt_shade_rays_device(d_rays, depth, flags) into the stream's scratch, then the splat of those
 * colours at d_xy; the sample of an invalid ray is dropped (and counted as dropped).  Flags, depth
 * and ray counters as rt_shade_rays_device. */
int  rt_film_shade_rays_device(rt_film* film, const rt_ray* d_rays, const float* d_xy, long long n,
                               int depth, int flags, void* hip_stream);
int  rt_film_resolve_device(rt_film* film, float* d_rgb /* width*height*3 */, void* hip_stream);
int  rt_film_clear(rt_film* film);
int  rt_film_splat(rt_film* film, const float* xy, const rt_radiance* rad, long long n);
int  rt_film_shade_rays(rt_film* film, const rt_ray* rays, const float* xy, long long n, int depth,
                        int flags, rt_stats* stats /* nullable: this call's rays, kernel time */);
int  rt_film_resolve(rt_film* film, float* rgb /* width*height*3 */);
/* The raw Pixels, width*height*4 floats (for tests and checkpoints); waits for the device. */
int  rt_film_read(rt_film* film, float* color_weight4);
/* Samples added and samples dropped since create / clear; waits for the device. */
int  rt_film_counts(rt_film* film, long long out2[2]);
/* Per-stage HIP-event times of the film's splats (tools/film_bench.py): while enabled every splat
 * records events around its stages; rt_film_stage_times waits for the last one and writes its
 * times in ms (bin, scan, scatter, order, gather).  RT_E_INVALID when no splat was timed. */
int  rt_film_set_stage_timing(rt_film* film, int enable);
int  rt_film_stage_times(rt_film* film, double ms5[5]);

/* ---- Light samples: radiance queries and films shaded with the caller's own lights -----------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_LIGHT_SAMPLES /
 * rt_light_samples_version).  The scene's point lights are fixed when the scene is made; an area
 * light is a new point on the emitter for every ray (HW3/src/Scene.cpp:177-220 draws one per
 * shading call, shades it as a point light and applies the emitter's cosine).  The caller draws
 * the points; these entries are rt_shade_rays* / rt_film_shade_rays* with each ray's own light
 * records added to the light loop.
 *
 *   value     ray i's result is rt_shade_rays' result on a scene whose light list is L_i: the
 *             scene's point lights in their order (none with RT_QUERY_NO_SCENE_LIGHTS), followed
 *             by the ACTIVE records of lights[i k .. i k + k) in their order — with
 *             RT_QUERY_LIGHTS_SHARED by those of lights[0 .. k), for every ray.  The whole ray
 *             tree uses L_i, at every bounce.  (A deliberate departure: the reference draws a new
 *             point on the light at every shading call; here it is one per ray tree.  A caller who
 *             wants a fresh draw per bounce does the bounce itself and comes back in at depth - 1.)
 *             Everything else is rt_shade_rays' contract as it stands: t, depth, the miss rule,
 *             RT_QUERY_IN_MEDIUM, RT_QUERY_REORDER, invalid rays, independence of n / position /
 *             neighbours, streams, scratch, chunks under the scratch limit.
 *   active    a record is INACTIVE iff a component of `position` is not finite; it is skipped as if
 *             absent: no shadow ray, no count.  Rays with fewer than k lights pad with a NaN
 *             position.
 *   point     `normal` +-0 in all three components: exactly the scene's point-light term
 *             (HW2/Scene.cpp:113-138) in the same operation order.
 *   emitter   any other `normal`, used as given (not normalised): ic = dot(-w_i, normal), and each
 *             of the two contributions carries it as HW3/src/Scene.cpp:207-218 associates it,
 *             (((kd * I) * ic) * cos) / d^2  and  (((ks * I) * ic) * pw) / d^2, in fp32 without
 *             contraction, pw the same fp64 pow.  No clamp: a sample seen from behind its emitter
 *             subtracts light, as in the reference.  HW3's has_diffuse / has_specular skips are
 *             not taken over: HW2's loop has none, and its shadow-ray count is the one counted.
 *   counters  one shadow ray per shading lane and active light of L_i; the rest as rt_shade_rays*.
 *   k         0 .. 256 per ray, 0 .. 65535 shared.  k == 0 ignores `lights` and, without the two
 *             flags below, is rt_shade_rays bit for bit.  lights: 16-byte aligned, n k records (k
 *             shared); NULL with k > 0, a misaligned pointer or k out of range is RT_E_INVALID
 *             before any HIP call.  Multi-device scenes: RT_E_UNSUPPORTED.
 *
 * rt_shade_rays*, rt_film_shade_rays*, rt_trace_rays* and rt_occluded* refuse the two new flag bits
 * like any unknown one. */
#define CENG795_RT_HAS_LIGHT_SAMPLES 1
int rt_light_samples_version(void); /* 1 */

typedef struct rt_light_sample {          /* 48 B */
  float position[3];  float pad0;
  float intensity[3]; float pad1;
  float normal[3];    float pad2;          /* 0 0 0: a point light */
} rt_light_sample;
enum { RT_QUERY_LIGHTS_SHARED = 4, RT_QUERY_NO_SCENE_LIGHTS = 8 };

int rt_shade_rays_lit_device(rt_scene* scene, const rt_ray* d_rays, long long n, int depth,
                             const rt_light_sample* d_lights, int k,
                             rt_radiance* d_out, int flags, void* hip_stream);
int rt_shade_rays_lit(rt_scene* scene, const rt_ray* rays, long long n, int depth,
                      const rt_light_sample* lights, int k,
                      rt_radiance* out, int flags, rt_stats* stats);
int rt_film_shade_rays_lit_device(rt_film* film, const rt_ray* d_rays, const float* d_xy, long long n,
                                  int depth, const rt_light_sample* d_lights, int k,
                                  int flags, void* hip_stream);
int rt_film_shade_rays_lit(rt_film* film, const rt_ray* rays, const float* xy, long long n, int depth,
                           const rt_light_sample* lights, int k, int flags, rt_stats* stats);

/* ---- Surface data: smooth shading and hit attributes (barycentrics, normals, uv) --------------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_SURFACE / rt_surface_version);
 * rt_scene_desc and rt_ray_hit keep their layout.  Every entry above shades with one normal per
 * triangle (HW2's Triangle::normal).  These add the smooth-shaded meshes of the later homeworks
 * (<Mesh shadingMode="smooth">, HW3/src/Scene.cpp:634-639) and tell a caller with its own shading
 * where inside a triangle a ray hit.
 *
 *   scenes    rt_scene_create_surface is rt_scene_create with an rt_surface_desc beside the
 *             description: which meshes are smooth, the per-vertex normals (used as given, not
 *             normalised; NULL: computed by the rule below) and per-vertex texture coordinates.
 *             A NULL surface, or one without a smooth mesh and without uv, gives a scene whose
 *             every result equals rt_scene_create's, byte for byte.  The caller's own BVH
 *             (bvh_*) works as before: vertex data is found by vertex id.
 *             rt_scene_load_xml_surface is rt_scene_load_xml with shadingMode="smooth" honoured
 *             (no uv); rt_scene_load_xml itself keeps ignoring the attribute, as HW2 does.
 *             There is no _multi variant of either.
 *   normals   vn[v] = 0; then for the meshes in order and each mesh's faces in order (flat meshes
 *             too, loose <Triangle>s not): c = (v1 - v0).cross(v2 - v0), n = c / length(c) (the
 *             bits of the flat normal), area = length(c) / 2, vn[i] = vn[i] + n * area for i0, i1,
 *             i2 in that order; at the end every vertex that got a contribution becomes
 *             vn / length(vn) (HW3/src/Scene.cpp:690-695, 870-876, Mesh_triangle.cpp:16, 69-74,
 *             Vertex.h:13-22).  All fp32, one rounding per operation; a 0/0 stays NaN.
 *             rt_host_vertex_normals_desc computes exactly this on the host.
 *   hit       on a triangle of a smooth mesh Hit_data::normal is Mesh_triangle.cpp:101-106 with the
 *             beta, gamma of HW2/Triangle.cpp:51, 53 (re-derived after the walk from the winning
 *             leaf and the ray by the arithmetic the walk ran: the same bits):
 *               w = (1.0f - beta) - gamma;  N = ((n0 * w) + (n1 * beta)) + (n2 * gamma);
 *               normal = N / length(N)
 *             every product and sum rounded, no contraction, a true division.  Everything else of
 *             Scene::trace_ray is HW2's; the smooth normal feeds the diffuse and specular cosines,
 *             the mirror direction, the entering / leaving test and the refraction.  (The HW3
 *             program itself renormalises this normal once more in Mesh_instance, Mesh.h:69, so
 *             its frames differ from this contract in the last bits.)
 *   entries   rt_trace_rays* report the smooth normal in rt_ray_hit::normal; rt_shade_rays*,
 *             rt_shade_rays_lit*, rt_film_shade_rays*, rt_render* and MSAA frames shade with it.
 *             A scene with a smooth mesh renders its frames on the ray-tree path, and to pixel
 *             records, tile costs and the dispatch order it behaves like a scene that recurses:
 *             rt_scene_records_ok is 0, RT_TILE_RECORDS is refused, rt_tile_costs has nothing.
 *   attributes rt_hit_attributes* turn rays and the rt_ray_hit records a closest-hit query gave for
 *             them into rt_hit_attr records, on any single-device scene (flat ones too): record i
 *             is computed from ray i and hits[i].leaf alone.  A triangle gives beta, gamma as above,
 *             uv = ((uv0 * w) + (uv1 * beta)) + (uv2 * gamma) (0 0 without vertex_uv), the shading
 *             normal (smooth as above, else the flat normal) and the flat normal.  A sphere gives
 *             (o + d * hits[i].t - center).normalize() for both normals (Sphere.h:57) and beta =
 *             gamma = 0.  A leaf outside [0, leaves) or an invalid ray gives the all-zero record;
 *             nothing is read out of bounds whatever the caller passes.
 *
 * rays, hits, attr: 16-byte aligned.  n == 0 succeeds and launches nothing; n < 0, a NULL pointer
 * with n > 0 or a misaligned pointer is RT_E_INVALID before any HIP call.  Multi-device scenes:
 * RT_E_UNSUPPORTED. */
#define CENG795_RT_HAS_SURFACE 1
int rt_surface_version(void); /* 1 */

typedef struct rt_surface_desc {
  size_t struct_size;                 /* sizeof(rt_surface_desc): room to grow          */
  const unsigned char* mesh_smooth;   /* [num_meshes], non-zero: tsm_smooth; NULL: none */
  const float* vertex_normals;        /* fp32[3*num_vertices] used as given (not
                                         normalised), or NULL: computed by the rule above */
  const float* vertex_uv;             /* fp32[2*num_vertices] or NULL                   */
} rt_surface_desc;
int rt_scene_create_surface(const rt_scene_desc* desc, const rt_surface_desc* surface, int device,
                            rt_scene** out);
int rt_scene_load_xml_surface(const char* xml_path, int device, rt_scene** out);
int rt_scene_has_smooth(const rt_scene* scene);   /* 1 iff some mesh is smooth */
/* Host-only, touch no HIP API.  rt_host_vertex_normals_desc: the rule above into
 * out3n[3*num_vertices].  rt_host_mesh_smooth_xml: the scene file's meshes' shadingMode (1: smooth)
 * into out[min(meshes, capacity)]; returns the number of meshes. */
int rt_host_vertex_normals_desc(const rt_scene_desc* desc, float* out3n);
int rt_host_mesh_smooth_xml(const char* xml_path, unsigned char* out, int capacity);

enum { RT_ATTR_HIT = 1, RT_ATTR_TRIANGLE = 2, RT_ATTR_SMOOTH = 4 };
typedef struct rt_hit_attr {       /* 48 B, 16-byte aligned */
  float beta, gamma;               /* 0 0: sphere, miss                                */
  float uv[2];                     /* ((uv0*w) + (uv1*beta)) + (uv2*gamma); 0 0 without vertex_uv */
  float shading_normal[3]; int flags;  /* RT_ATTR_* */
  float geometric_normal[3]; int pad;  /* flat normal / the sphere normal              */
} rt_hit_attr;
int rt_hit_attributes_device(rt_scene* scene, const rt_ray* d_rays, const rt_ray_hit* d_hits,
                             long long n, rt_hit_attr* d_attr, void* hip_stream);
int rt_hit_attributes(rt_scene* scene, const rt_ray* rays, const rt_ray_hit* hits, long long n,
                      rt_hit_attr* attr);

/* ---- Mesh instances: transformed meshes through a two-level walk ------------------------------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_INSTANCES / rt_instances_version).
 * A scene can be made of INSTANCES: a base mesh, a material and a 4x4 transformation each, beside
 * loose triangles and spheres — HW3's Mesh_instance (HW3/include/Mesh.h:55-74, static branch)
 * under HW2's Scene::trace_ray.  The reference transforms the ray, not the vertices, and so does
 * this: 1000 copies of a mesh cost 1000 instance records, and the bits are the reference's.
 *
 *   objects   In an instanced scene the description's meshes are bases only: a mesh is reached only
 *             through instances and mesh_material is ignored.  The top-level object list is the
 *             instances in order, then the loose triangles, then the spheres
 *             (HW3/src/Scene.cpp:706-869), under the reference's median-split BVH; each base mesh
 *             has its own tree over its faces (Mesh::Mesh; a one-face mesh is that triangle).
 *             A NULL instance descriptor, or num_instances == 0, gives rt_scene_create's scene.
 *   matrices  instance_transform is object -> world, row-major.  Its inverse is
 *             Matrix4x4::invert_matrix (HW3/src/Matrix4x4.cpp:99-235: cofactors in that order,
 *             fp32); a zero determinant is RT_E_INVALID (the reference exits).  The normal matrix
 *             is the inverse's transpose.  The instance's box is Bounding_box::apply_transform
 *             (HW3/src/bounding_box.cpp:40-114) of the base mesh's root box.
 *   hit       ray (o, d) meets an instance as Mesh.h:55-74 has it: (1) the world ray against the
 *             instance box by the node rule (bbox_t < 0 || bbox_t == inf: a miss); (2) the local
 *             ray o' = inverse.multiply(o), d' = inverse.multiply(d, true) (Matrix4x4.cpp:29-49:
 *             per row from e[i][3] for a point, from 0.0f for a vector, then + e[i][0] x,
 *             + e[i][1] y, + e[i][2] z, every product and sum rounded); d' is not normalised, so
 *             the local t is the world t; (3) the mesh's closest hit for (o', d') from t = inf;
 *             (4) normal = normalT.multiply(n, true) / its length, n the flat normal; the material
 *             is the instance's.  An identity transformation takes this path too.
 *             Over the top level the result is the minimum of (t, top-level DFS leaf, mesh DFS
 *             leaf) over what the ray may reach; a one-object list is that object's own rule.
 *             Occlusion: some reachable primitive, through an instance or not, has 0 < t < tmax.
 *   departure a local ray that is no valid query ray (a non-finite component of o' or d', or all
 *             three |d'_i| < 1e-6) misses that instance and disturbs nothing.
 *   rt_ray_hit  t, normal as above; material the instance's; object the face's index in the object
 *             lists (mesh faces in mesh order, then loose triangles, then spheres); leaf a
 *             scene-wide leaf id: each base mesh's leaves in its DFS order, meshes in order, then
 *             the loose primitives in object-list order; pad the instance index, -1 for a loose
 *             primitive.  Flat scenes write what they always wrote.
 *   entries   rt_trace_rays*, rt_occluded*, rt_shade_rays*, rt_shade_rays_lit*,
 *             rt_film_*shade_rays* and rt_render* (MSAA frames included) take an instanced scene,
 *             in both traversal modes (the same bits) and with RT_QUERY_REORDER.  Like a smooth
 *             scene it renders its frames on the ray-tree path and behaves like a recursing scene
 *             elsewhere: rt_scene_records_ok is 0, RT_TILE_RECORDS is refused, rt_tile_costs has
 *             nothing.  RT_E_UNSUPPORTED with a message: rt_hit_attributes* and rt_scene_dump_bvh
 *             on an instanced scene, the caller's own BVH (bvh_*) with instances, multi-device
 *             scenes, a top-level or base-mesh tree deeper than 62 levels. */
#define CENG795_RT_HAS_INSTANCES 1
int rt_instances_version(void); /* 1 */

typedef struct rt_instance_desc {
  size_t struct_size;              /* sizeof(rt_instance_desc): room to grow            */
  int num_instances;
  const int*   instance_mesh;      /* [n] 0-based mesh of the description               */
  const int*   instance_material;  /* [n]                                               */
  const float* instance_transform; /* fp32[16 n], row-major 4x4, object -> world        */
} rt_instance_desc;
int rt_scene_create_instanced(const rt_scene_desc* desc, const rt_instance_desc* instances,
                              int device, rt_scene** out);
/* rt_scene_load_xml with the file's instances honoured (rt_scene_load_xml itself keeps ignoring
 * all of it): the root <Transformations> block (Scaling, Translation, Rotation in degrees:
 * HW3/src/Transformation.cpp:6-72 with the host's std::cos / std::sin), per-object lists such as
 * "s1 t2 r1", each element left-multiplying (Scene.cpp:641-664); <Mesh> k becomes instance k with
 * its own transformation and material, then each <MeshInstance baseMeshId resetTransform> with its
 * material (Scene.cpp:713-761); vertexOffset is honoured, shadingMode ignored.
 * RT_E_UNSUPPORTED: <Transformations> on a <Triangle> or <Sphere>, a non-zero <MotionBlur>,
 * plyFile.  rt_host_instances_xml (host-only, touches no HIP API) writes the first
 * min(n, capacity) instances' mesh, material and matrix (any output may be NULL) and returns n. */
int rt_scene_load_xml_instanced(const char* xml_path, int device, rt_scene** out);
int rt_host_instances_xml(const char* xml_path, int* mesh, int* material, float* transform16,
                          int capacity);
/* Host-only: builds every base mesh's culling tree (treelets of <= treelet_leaves leaves) and
 * checks the invariants of rt_host_check_accel_xml on each; stats4[4 m ..] = mesh m's treelets,
 * culling nodes, culling-tree depth, lone-leaf treelets (NULL: not reported).  Returns the number
 * of base meshes, or RT_E_INVALID with the violation in rt_last_error(). */
int rt_host_check_accel_instanced_desc(const rt_scene_desc* desc,
                                       const rt_instance_desc* instances, int treelet_leaves,
                                       long long* stats4);
int rt_scene_num_instances(const rt_scene* scene);   /* 0: a flat scene */
/* Host-only, touches no HIP API: per instance its inverse matrix (row-major 4x4), its world box
 * (min xyz, max xyz) and its DFS position among the top-level leaves.  Any output may be NULL.
 * Also builds and checks every base mesh's culling tree (RT_E_INVALID with the violation). */
int rt_host_instance_info_desc(const rt_scene_desc* desc, const rt_instance_desc* instances,
                               float* inverse16 /*[16 n]*/, float* box6 /*[6 n]*/,
                               int* top_dfs /*[n]*/);

/* ---- Motion blur: ray times, moving instances, transformed and moving spheres ------------------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_MOTION / rt_motion_version).
 * HW3's motion blur: a ray carries a TIME, and an instance or sphere with a velocity is met
 * through the inverse of Translation(time * velocity) * M, built per ray (HW3/include/Ray.h:18,
 * Mesh.h:75-92, Sphere.h:113-154).  A sphere may also carry a transformation (Sphere.h:76-112, the
 * static half of the same code).  A motion-blurred image is a film fed with rays that each carry
 * a time in [0, 1) from the caller's generator; every sample is the reference's bit for bit.
 *
 *   time      tau, any finite float (the reference documents [-1, 1] and draws [0, 1)); 0 unless
 *             the call has RT_QUERY_RAY_TIME, with which rt_ray::pad is the ray's time.  Every ray
 *             of a ray tree has the time of the tree's first ray: the shadow rays of the scene's
 *             lights and of the caller's light records, mirror, reflection and transmission rays
 *             (HW3/src/Scene.cpp:153, 196, 226, 258, 294-304).
 *   moving instance (velocity != 0; -0 == 0)  (1) the world ray against the instance box by the
 *             node rule, as for a static instance; (2) delta = tau * velocity per component;
 *             (3) A = T(delta) * M by Matrix4x4::operator*: every result[i][j] from 0 through
 *             a[i][k] * r[k][j], k = 0..3, the products with 0 and 1 included; (4) the inverse of A
 *             by Matrix4x4::invert_matrix; (5) the local ray A^-1.multiply(o),
 *             A^-1.multiply(d, true), not normalised; (6) the mesh's closest hit for it;
 *             (7) normal = (A^-1)^T.multiply(n, true).normalize(); (8) the instance's material.
 *             A static instance (velocity == 0) is met as before.
 *   boxes     an instance's box is apply_transform(mesh root box, M); a sphere's is center +-
 *             radius, taken through apply_transform unless its matrix is exactly the identity.
 *             With velocity != 0 the box (min, max) is then expanded by (min + v, max + v) and by
 *             (min - v, max - v) (Mesh.h:104-110, Sphere.h:30-36; fmin / fmax folds).  The box does
 *             not depend on tau: a ray whose time carries the object outside its box misses it at
 *             the box, as in the reference.  The top-level tree is built over these boxes.
 *   sphere    identity matrix and zero velocity: the HW2 rule, as ever.  Otherwise the sphere's
 *             test runs on the local ray, taken through the host-computed inverse of M (zero
 *             velocity) or through the per-ray inverse of T(tau v) * M; the normal is
 *             (inverse)^T.multiply((o' + t d' - center).normalize(), true).normalize().  In the
 *             top-level tree the leaf rule 0 < t < inf applies; a lone sphere reports its own
 *             answer.  rt_ray_hit: object, leaf and material as a sphere's, pad -1.
 *   departures  on a scene with motion a ray whose time is not finite is an INVALID ray (a miss,
 *             not occluded, radiance (0, 0, 0, +inf); a fused film entry still bins its sample,
 *             black).  A per-ray A with det == 0.0f misses that object (the reference exits).  A
 *             local ray with a non-finite component, or with all three |d'_i| < 1e-6, misses the
 *             object, as for instances.
 *   frames    rt_render*, MSAA frames included, render a scene with motion at tau = 0 for every
 *             ray (the reference seeds its time generator from the clock; nothing to reproduce).
 *             A blurred frame is a film.
 *   entries   as for instanced scenes.  RT_QUERY_RAY_TIME is accepted by rt_trace_rays*,
 *             rt_occluded*, rt_shade_rays*, rt_shade_rays_lit*, rt_film_shade_rays* and
 *             rt_film_shade_rays_lit*; on a scene without motion it has no effect and pad is not
 *             read.  Results do not depend on n, on a ray's position or neighbours, on
 *             RT_QUERY_REORDER or on the traversal mode.  Loose triangles take neither a
 *             transformation nor a velocity.
 *
 * rt_scene_create_moving: a NULL or trivial motion descriptor (every velocity zero, every sphere
 * matrix the identity or NULL) gives exactly rt_scene_create_instanced's scene.  The instance
 * descriptor may be NULL or empty: the top level is then the loose triangles and spheres, and the
 * description's meshes are unreachable bases.  RT_E_INVALID before any HIP call: a short
 * struct_size, counts that disagree with the other two descriptors (a count may be 0 when its
 * arrays are NULL), a non-finite velocity or matrix entry, a singular sphere matrix.  What
 * rt_scene_create_instanced answers with RT_E_UNSUPPORTED stays RT_E_UNSUPPORTED. */
#define CENG795_RT_HAS_MOTION 1
int rt_motion_version(void); /* 1 */

typedef struct rt_motion_desc {
  size_t struct_size;              /* sizeof(rt_motion_desc)                           */
  int num_instances;               /* = the instance descriptor's count, or 0          */
  int num_spheres;                 /* = desc->num_spheres, or 0                        */
  const float* instance_velocity;  /* fp32[3 ni], or NULL: all zero                    */
  const float* sphere_transform;   /* fp32[16 ns] row-major object->world, or NULL: identity */
  const float* sphere_velocity;    /* fp32[3 ns], or NULL: all zero                    */
} rt_motion_desc;                  /* 40 B */
int rt_scene_create_moving(const rt_scene_desc* desc, const rt_instance_desc* instances,
                           const rt_motion_desc* motion, int device, rt_scene** out);
/* rt_scene_load_xml_instanced plus <MotionBlur>x y z</MotionBlur> on <Mesh>, <MeshInstance> and
 * <Sphere> and <Transformations> on <Sphere> (composed as the per-object lists are).  A <Mesh>'s
 * velocity belongs to its instance k; a <MeshInstance> takes its own <MotionBlur>, not its
 * base's (HW3/src/Scene.cpp:666-760).  <Transformations> on a <Triangle> and plyFile stay
 * RT_E_UNSUPPORTED.  The other loaders read such files exactly as before. */
int rt_scene_load_xml_moving(const char* xml_path, int device, rt_scene** out);
int rt_scene_has_motion(const rt_scene* scene); /* 1: the motion kernels run on it */
enum { RT_QUERY_RAY_TIME = 32 };   /* rt_ray.pad is the ray's time */
/* Host-only, touch no HIP API.  rt_host_motion_info_desc: every instance's box (expanded), every
 * sphere's inverse matrix (row-major 4x4) and box, and the top-level DFS position of every
 * top-level object (instances, loose triangles, spheres); any output may be NULL.
 * rt_host_motion_xml: what rt_scene_load_xml_moving read — per instance its velocity, per sphere
 * its composed matrix and velocity, the first min(n, capacity) of each; any output may be NULL;
 * counts2 (nullable) = the numbers of instances and spheres.  Returns RT_OK. */
int rt_host_motion_info_desc(const rt_scene_desc* desc, const rt_instance_desc* instances,
                             const rt_motion_desc* motion, float* inst_box6 /*[6 ni]*/,
                             float* sphere_inverse16 /*[16 ns]*/, float* sphere_box6 /*[6 ns]*/,
                             int* top_dfs /*[ni + triangles + ns]*/);
int rt_host_motion_xml(const char* xml_path, float* instance_velocity3, float* sphere_transform16,
                       float* sphere_velocity3, int capacity, int* counts2);
/* Debug: the device's own per-ray T(tau v) * M and inversion for top-level object `top_object`
 * (an instance, or a sphere counted after the instances and loose triangles) of a scene with
 * motion, at n host times: out12[12 i ..] = rows 0..2 of the inverse the walk uses at times[i], or
 * 12 NaNs where det == 0.  RT_E_INVALID for an object that does not move. */
int rt_debug_motion_inverse(rt_scene* scene, int top_object, const float* times, long long n,
                            float* out12);

/* ---- Textures: image textures on the diffuse colour inside every ray tree ----------------------
 *
 * New symbols within ABI 7 (test for them with CENG795_RT_HAS_TEXTURES / rt_textures_version);
 * rt_scene_desc, rt_surface_desc, rt_ray_hit and rt_hit_attr keep their layouts.  rt_hit_attributes
 * tells a caller with its own shading where a ray hit; these put HW4's image textures into the
 * library's shading, so a textured floor is lit by the scene's lights and shadow rays, shows in a
 * mirror and through glass, and feeds films and light samples.
 *
 *   value     HW2's Scene::trace_ray, as every entry has it, with HW4's texture step at each hit
 *             (HW4/src/Scene.cpp:149-171, Texture.cpp:44-134): HW4's rule placed over HW2's loop,
 *             as smooth shading is HW3's.  It is not bit parity with the HW4 program.
 *   scenes    rt_scene_create_textured is rt_scene_create_surface with an rt_texture_desc beside
 *             the two descriptions: the textures, and per mesh, loose triangle and sphere a texture
 *             id (-1: none; a NULL list: none).  A NULL texture descriptor, or one in which no
 *             object names a texture, gives exactly rt_scene_create_surface's scene, byte for byte
 *             in every result.  Pixels are copied at creation.  Smooth meshes and the caller's own
 *             BVH (bvh_*) combine with textures as they do with surface data.  RT_E_INVALID before
 *             any HIP call: a short struct_size, a texture id outside [-1, num_textures), a size,
 *             mode or normalizer out of range, a NULL rgb8, a textured mesh or loose triangle
 *             without surface->vertex_uv (spheres need no uv).  There is no _multi, instanced or
 *             moving variant.
 *   (u, v)    triangle (Mesh_triangle.cpp:107-111): uva, uvb, uvc the vertex_uv of the leaf's three
 *             vertex ids, beta and gamma those of the smooth normal above (re-derived once per hit):
 *               u = (uva.x + beta * (uvb.x - uva.x)) + gamma * (uvc.x - uva.x),  v alike in .y
 *             every operation a rounded fp32 operation, no contraction.  This is HW4's expression,
 *             not the ((uv0*w) + (uv1*beta)) + (uv2*gamma) of rt_hit_attr::uv, which stays as it
 *             is: the two can differ in the last bit.
 *             sphere (Sphere.cpp:100-105), lc = (o + d * t) - center in fp32:
 *               theta = (float)acos((double)(lc.y / radius)); phi = (float)atan2((double)lc.z, (double)lc.x)
 *               u = (float)((M_PI - (double)phi) / (2 * M_PI));  v = (float)((double)theta / M_PI)
 *             acos and atan2 are fp64 islands like pow: libm's on the host, ocml's on the device.
 *   lookup    Texture::get_color_at(u, v), Texture.cpp:57-134, all fp32, raw channel values 0..255:
 *             clamp: u = fmax(0, fmin(1, u)); repeat: u = fmax(0, fmin(1, u - floor(u))) (a NaN
 *             becomes 1); u = u * width, minus 1.0f if u >= width; v alike with height.  Nearest:
 *             texel (row (unsigned)v, column (unsigned)u).  Bilinear, repeat: p = (unsigned)u % w,
 *             pn = (p+1) % w, q, qn alike, dx = u - p, dy = v - q; per channel
 *             T[q][p]*(1-dx)*(1-dy) += T[q][pn]*dx*(1-dy) += T[qn][pn]*dx*dy += T[qn][p]*(1-dx)*dy,
 *             products left to right, each += rounded.  Bilinear, clamp: p = (unsigned)u,
 *             pn = p + 1, q = (unsigned)v, qn = (unsigned)(v + 1.0f), texels by LINEAR index
 *             w*row + column with the reference's own guards: pn < w adds index w*q+pn;  qn < h
 *             adds index w*qn+pn (with pn == w that is the first texel of row qn + 1: kept);
 *             pn < w && qn < h adds index w*qn+p.  One departure: a term whose linear index is
 *             >= w*h, where the reference reads past its buffer, is skipped.
 *   shading   tex = lookup(u, v) at a hit on a textured object.  RT_TEX_REPLACE_ALL: the ray's
 *             colour is tex (raw, 0..255) and nothing else — no ambient, no light, no shadow ray
 *             counted, no mirror or refraction ray, in_medium or not (Scene.cpp:156-159); the hit
 *             still counts as a primary hit and reports t.  Otherwise kd' = tex / normalizer per
 *             channel (RT_TEX_REPLACE_KD) or ((tex / normalizer) + kd) / 2.0f (RT_TEX_BLEND_KD),
 *             true divisions, and kd' takes the place of material.diffuse in the scene's light
 *             loop and the light-sample loop of that hit; ambient, specular, mirror, transparency
 *             and Beer's law keep the material's values.  HW4's has_diffuse / has_specular skips
 *             are not taken over: HW2's loop has none, and its shadow-ray count is the one counted.
 *             Untextured objects of a textured scene shade exactly as before.
 *   entries   rt_shade_rays*, rt_shade_rays_lit*, rt_film_shade_rays*, rt_film_shade_rays_lit*,
 *             rt_render* and MSAA frames shade with textures; rt_trace_rays*, rt_occluded* and
 *             rt_hit_attributes* report what they report today.  A textured scene renders its
 *             frames on the ray-tree path and behaves like a recursing scene elsewhere:
 *             rt_scene_records_ok is 0, RT_TILE_RECORDS is refused, rt_tile_costs has nothing.
 *             Both traversal modes and RT_QUERY_REORDER give the same bits; results do not depend
 *             on n, position or neighbours.
 *   rt_texture_lookup*  the lookup alone, one record per query: rgb[3 i ..] = lookup of texture
 *             q[i].texture at (q[i].u, q[i].v); a texture id out of range gives 0 0 0 and reads
 *             nothing.  d_q: 16-byte aligned; n == 0 launches nothing; n < 0 or a NULL pointer with
 *             n > 0 is RT_E_INVALID before any HIP call.  rt_host_texture_lookup_desc runs the
 *             same function on the host for a descriptor (checked as scene creation checks it)
 *             and touches no HIP API. */
#define CENG795_RT_HAS_TEXTURES 1
int rt_textures_version(void); /* 1 */

enum { RT_TEX_NEAREST = 0, RT_TEX_BILINEAR = 1 };
enum { RT_TEX_REPLACE_KD = 0, RT_TEX_BLEND_KD = 1, RT_TEX_REPLACE_ALL = 2 };
enum { RT_TEX_REPEAT = 0, RT_TEX_CLAMP = 1 };
typedef struct rt_texture {
  const unsigned char* rgb8;  /* height rows of width texels, 3 bytes each, tightly packed, top row
                                 first (stbi_load(..., 3)) */
  int width, height;          /* 1 .. 16384 each */
  int interpolation, decal, appearance;
  float normalizer;           /* finite, != 0; the reference's default is 255 */
} rt_texture;
typedef struct rt_texture_desc {
  size_t struct_size;           /* sizeof(rt_texture_desc) */
  int num_textures;
  const rt_texture* textures;
  const int* mesh_texture;      /* [num_meshes]    -1: none; NULL: none */
  const int* triangle_texture;  /* [num_triangles] */
  const int* sphere_texture;    /* [num_spheres]   */
} rt_texture_desc;
int rt_scene_create_textured(const rt_scene_desc* desc, const rt_surface_desc* surface /* may be NULL */,
                             const rt_texture_desc* textures, int device, rt_scene** out);
int rt_scene_num_textures(const rt_scene* scene);  /* 0: an untextured scene */

typedef struct rt_tex_query { int texture; float u, v; int pad; } rt_tex_query; /* 16 B */
int rt_texture_lookup_device(rt_scene* scene, const rt_tex_query* d_q, long long n,
                             float* d_rgb /* 3 n */, void* hip_stream);
int rt_texture_lookup(rt_scene* scene, const rt_tex_query* q, long long n, float* rgb);
int rt_host_texture_lookup_desc(const rt_texture_desc* textures, const rt_tex_query* q, long long n,
                                float* rgb);

/* Scene files.  rt_scene_load_xml_textured is rt_scene_load_xml_surface plus (HW4/src/Scene.cpp:
 * 690-701, 761-768, 905-911, 1008-1014, 1030-1077): <TexCoordData>, read as pairs; the root
 * <Textures> block: <ImageName>, <Interpolation> (default bilinear; anything but "nearest" is
 * bilinear), <DecalMode> (default blend_kd; anything but "replace_kd" or "blend_kd" is
 * replace_all), <Appearance> (default clamp; anything but "repeat" is clamp), <Normalizer>
 * (default 255.0); and a 1-based <Texture> child of <Mesh>, <Triangle> and <Sphere>.  The library
 * decodes no image files: the caller passes the decoded images, matched to <ImageName> by string;
 * a name without a record is RT_E_IO.  RT_E_UNSUPPORTED with a message: ImageName "perlin",
 * bumpmap="true", <BackgroundTexture>, a textured mesh whose textureOffset differs from its
 * vertexOffset (uv is kept per vertex id), fewer uv pairs than a textured face's vertex ids need,
 * plyFile.  Every other loader reads such files exactly as before.
 * rt_host_textures_xml (host-only, touches no HIP API) reports what was parsed: per texture
 * (the first min(textures, texture_capacity)) its name (names: texture_capacity x 256 chars,
 * NUL-terminated), interpolation / decal / appearance (modes3: 3 ints each) and normalizer; each
 * object list's 0-based texture ids (-1: none; the first min(count, object_capacity) of each); the
 * first min(pairs, uv_capacity) <TexCoordData> pairs; counts5 = textures, meshes, triangles,
 * spheres, uv pairs.  Any output may be NULL. */
typedef struct rt_texture_image {
  const char* name;
  const unsigned char* rgb8;  /* as rt_texture::rgb8 */
  int width, height;
} rt_texture_image;
int rt_scene_load_xml_textured(const char* xml_path, const rt_texture_image* images, int num_images,
                               int device, rt_scene** out);
int rt_host_textures_xml(const char* xml_path, char* names, int* modes3, float* normalizer,
                         int texture_capacity, int* mesh_texture, int* triangle_texture,
                         int* sphere_texture, int object_capacity, float* uv2, int uv_capacity,
                         int* counts5);

/* PNG output as HW2/main.cpp:43-57: per channel clamp(int(c), 0, 255), alpha 255. */
int rt_write_png(const char* path, const float* rgb, int width, int height);

/* Camera precompute of HW2/Camera.h:10-29 in the reference's fp32 operation order. */
int rt_camera_from_view(const float position[3], const float gaze[3], const float up[3],
                        const float near_plane[4] /* l r b t */, float near_distance,
                        int width, int height, int num_samples, rt_camera* out);

const char* rt_last_error(void);
int rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
