// C-ABI implementation (include/ceng795_rt.h): scene upload, render launches, counters,
// multi-device frames.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <array>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ceng795_rt.h"
#include "hip_host.h"
#include "host_scene.h"
#include "rt_internal.h"

namespace rt {
hipError_t launch_render(const RenderParams& P, bool fast, bool deep, bool spheres,
                         const hipEvent_t* marks, const SurfParams* surf, const InstParams* inst,
                         const MotionParams* motion, const TexParams* tex, hipStream_t stream);
hipError_t launch_motion_inverse(const float* fwd, const float* vel, const float* times,
                                 long long n, float* out12, hipStream_t stream);
int max_supported_depth();
hipError_t launch_msaa_resolve(const MsaaResolveParams& M, hipStream_t stream);
hipError_t launch_untile(const UntileParams& U, hipStream_t stream);
hipError_t launch_resolve_rows(const RenderParams& P, const unsigned* rec, int row_begin,
                               int row_end, bool spheres, hipStream_t stream);
hipError_t launch_resolve(const RenderParams& P, const UntileParams& U, bool spheres,
                          hipStream_t stream);
unsigned long long read_reset_exact_fallbacks();
hipError_t launch_quot_check(int mode, unsigned long long seed, long long count,
                             unsigned long long* counts, hipStream_t stream);
bool diag_build();
long long read_reset_timeline(unsigned long long* out, long long max_values);
long long read_reset_phases(unsigned long long* out, long long max_values);
hipError_t frame_kernel_occupancy(int* out4);
int launch_cold_order(RenderParams P, hipStream_t stream);
void set_test_visit_time_exp(int on, int rel);
hipError_t launch_query(const RenderParams& P, QueryParams Q, const DevNode* nodes, bool occlusion,
                        bool reorder, bool fast, bool deep, bool spheres, const SurfParams* surf,
                        hipStream_t stream);
hipError_t launch_query_sort(QueryParams Q, hipStream_t stream);
hipError_t launch_inst_query(const RenderParams& P, QueryParams Q, const InstParams& T,
                             bool occlusion, bool reorder, bool fast, bool spheres,
                             const MotionParams* motion, hipStream_t stream);
hipError_t launch_radiance(const RenderParams& P, const QueryParams& Q, const RadianceParams& R,
                           const LitParams* lit, const DevNode* nodes, bool fast, bool deep,
                           bool spheres, const SurfParams* surf, const InstParams* inst,
                           const MotionParams* motion, const TexParams* tex, hipStream_t stream);
hipError_t launch_texture_lookup(const TexParams& X, const TexLookupParams& A, hipStream_t stream);
hipError_t launch_hit_attributes(const RenderParams& P, const SurfParams& S, const AttrParams& A,
                                 hipStream_t stream);
hipError_t launch_film_splat(const FilmParams& F, const hipEvent_t* marks, hipStream_t stream);
hipError_t launch_film_resolve(const float* pixels, float* out, int width, int height,
                               hipStream_t stream);
void write_png(const std::string& path, const float* rgb, int w, int h);
}  // namespace rt

using namespace rt;

// Device buffers of one synchronous call (rt_render, and every device's share of a
// multi-device frame), kept by the scene and reused: the reference calls render_image once per
// thread per camera (HW2/main.cpp:33-36), so a drop-in pays hipMalloc / hipFree only the first
// time a call of that size runs.  Calls on several host threads each take their own context
// (rt_render stays reentrant).
// rt_render into a caller buffer in pinned host memory: the frame kernel writes it directly
// (its device-visible address; C3 one frame at a time 0.94-0.97 -> 0.67-0.69 ms).  Into a
// pageable buffer: the frame as RT_RENDER_CHUNKS bands of tile rows, one launch each, each band
// copied out on a second stream as soon as it is done.  (The copies are blit kernels here,
// which wait for CU slots the render holds: pageable 1.00-1.05 ms unbanded, 0.89 with 2 bands,
// 0.98 with 4, 1.36 with 8; a high-priority copy stream changed nothing —
// profiles/r06/host_rate_bands.jsonl.)
#ifndef RT_RENDER_CHUNKS  // (A/B builds)
#define RT_RENDER_CHUNKS 2
#endif
constexpr int kRenderChunks = RT_RENDER_CHUNKS;

// Frame scratch of one chunk of a recursing radiance query: 256 MiB hold the
// frames of 342k rays at depth 6 (784 B each) — more waves than the device keeps resident, so a
// chunk still fills it — and of 1.2 M rays at depth 1.
constexpr size_t kRadianceDefaultLimit = size_t(256) << 20;

// What the launches on one stream (a pooled context's or a caller's) need besides their inputs
// and outputs; they run one after the other, so they share it.  The buffers only grow.
struct WorkSet {
  DevBuf<unsigned> occ;     // per pixel: the lights' occlusion bits
  DevBuf<unsigned> sched;   // tile costs, unit order lists, cost snapshot (rt_internal.h)
  DevBuf<float> frames;     // ray-tree frames: recursive scenes' frames and radiance queries
  DevBuf<float> samples;    // MSAA cameras: the sample passes
  DevBuf<unsigned> query;   // queries with RT_QUERY_REORDER: permutation, histogram, totals
  DevBuf<unsigned> film;    // film splats: per-pixel offsets, scan totals, sample lists (FilmParams)
  DevBuf<rt_radiance> film_rad;  // rt_film_shade_rays*: the colours between the query and the splat
  void reserve_tiles(const HostScene& h, size_t tiles);  // occ and sched
  // Sizes the set for launch P of camera c, whose num_sel_tiles is final, and points P at it.
  void bind(const rt_scene* s, const rt_camera& c, RenderParams& P);
};

struct RenderCtx {
  Stream stream;
  Event e0, e1;
  DevBuf<float> d_out;
  DevBuf<unsigned long long> d_cnt;
  WorkSet work;
  DevBuf<float> d_recv;   // multi-device frames, first device: the gathered tiles
  DevBuf<float> d_image;  // multi-device rt_render, first device: the row-major frame
  Event ev_in, ev_out;    // multi-device frames: caller-stream ordering
  // copy-gather frames (a device listed twice): recorded on the first device's stream after it
  // has copied the shares out of the other contexts' buffers; a context renders its next share
  // only after it (the copy reads d_out / d_image on another stream: write-after-read)
  Event ev_gathered;
  // rt_render's chunked copy-out (render_banded): a second stream for the device-to-host copies
  // and one event per row chunk (created on first use)
  Stream copy_stream;
  Event ev_chunk[kRenderChunks];
  // the host query entries: the uploaded rays and the results (rt_ray_hit or rt_radiance
  // records, or n bytes of occlusion flags)
  DevBuf<rt_ray> d_rays;
  DevBuf<rt_ray_hit> d_ray_out;
  DevBuf<float> d_xy;  // the host film entries: the uploaded positions; the resolved frame
  DevBuf<rt_light_sample> d_lit;  // the host `_lit` entries: the uploaded light records
};

// What the `_device` entries keep for one caller stream.  Owned through a unique_ptr, so its
// address is stable while the table grows; `mu` serialises host threads that enqueue on the
// same stream.
struct StreamScratch {
  void* stream = nullptr;
  std::mutex mu;
  WorkSet work;
  // warm order: the selection whose heavy-first unit order the last frame on this stream left
  // in `work.sched` (valid: that frame ran the order kernel)
  std::array<long long, 7> order_key{};
  bool order_valid = false;
  Event done;  // after the last frame enqueued on the stream (eviction waits on it)
  unsigned long long used = 0;  // Replica::tick of the last lookup (least recently used first)
};

// Streams a replica keeps scratch / a multi-device context for: beyond this many, the least
// recently used one is released (after its work has finished), so callers that make a new
// stream per frame do not grow device memory without bound.
constexpr size_t kMaxStreamTables = 64;

// Per-kernel HIP-event timing of render launches (rt_set_kernel_timing): one quad of events per
// launch of the first device.  Completed quads beyond kTimingPending are folded into `sum` so
// the list stays bounded while timing is on and nobody reads it.  `events` owns every quad's
// events; `pending` and `spare` hold their handles.
struct KernelTiming {
  bool on = false;
  std::vector<Event> events;
  std::vector<std::array<hipEvent_t, 4>> pending, spare;
  double sum[4] = {0, 0, 0, 0};
  long long folded = 0;
};
constexpr size_t kTimingPending = 256;

// The scene on one device: the flattened scene in HBM, the ray counters, and the buffers of
// the calls that run there.
struct Replica {
  int device = 0;
  // One tree's arrays (upload_tree): the flat scene's, or a base mesh's.
  struct TreeBufs {
    DevBuf<DevNode> nodes;
    DevBuf<DevPrim> prims;
    DevBuf<DevLeaf> leaves;
    DevBuf<float> normals;
    DevBuf<DevAncestry> anc;
    DevBuf<int> leaf_object;  // per DFS leaf: its object index (rt_ray_hit::object)
  };
  TreeBufs d_tree;  // the flat scene's (an instanced scene: empty)
  DevBuf<DevMaterial> d_mats;
  DevBuf<DevLight> d_lights;
  // surface data (HostScene::leaf_tri / vertex_normals / vertex_uv), each only when the scene
  // has it; `surf` points at them
  DevBuf<int> d_surf_tri;
  DevBuf<float> d_surf_normals, d_surf_uv;
  SurfParams surf{nullptr, nullptr, nullptr, 0};
  // image textures (HostScene::textures / texels), a textured scene only; `tex` points at them
  DevBuf<DevTexture> d_tex_table;
  DevBuf<uint32_t> d_texels;
  TexParams tex{nullptr, nullptr, 0, -1};
  // an instanced scene: every base mesh's arrays, the mesh and instance tables
  // and the top-level tree; `inst` points at them
  std::vector<TreeBufs> d_mesh;
  DevBuf<DevMesh> d_mesh_table;
  DevBuf<DevInstance> d_instances;
  DevBuf<DevNode> d_top_nodes;
  DevBuf<DevPrim> d_top_prims;
  DevBuf<float> d_top_normals;
  DevBuf<int> d_top_info;
  InstParams inst{};
  // a scene with motion: the moving objects' tables; `motion` points at them
  DevBuf<DevMotionInstance> d_motion_instances;
  DevBuf<DevMotionSphere> d_motion_spheres;
  MotionParams motion{};
  DevBuf<unsigned long long> d_counters;
  // per camera: its whole frame's cold order (seed_cold_orders), sched_words_for(tiles) words
  // laid out as a stream's `sched` (estimated costs, unit order, snapshot); empty: none
  std::vector<DevBuf<unsigned>> d_cold;
  // per camera: its entry cuts (seed_entry_cuts), kEntryCut ints per frame tile; empty: none
  std::vector<DevBuf<int>> d_cuts;
  std::mutex mu;  // ctx pool and stream tables
  std::vector<std::unique_ptr<RenderCtx>> ctx_all;  // every context; the two below point into it
  std::vector<RenderCtx*> ctx_free;
  std::vector<std::unique_ptr<StreamScratch>> streams;
  // multi-device scenes: the context each caller stream renders its shares on (one per caller
  // stream and device, kept across calls), so frames on different caller streams have their
  // own device streams and buffers and overlap (frames in flight, as scratch_for on one device)
  std::vector<std::pair<void*, RenderCtx*>> stream_ctx;
  unsigned long long tick = 0;  // lookups of `streams` (LRU order)
};

// What assemble_scene derived on the host (host, inst, deep, ... most), and the scene's devices.
struct rt_scene : SceneHost {
  int mode = RT_TRAVERSAL_FAST;
  bool tree_frames() const { return needs_recursion || smooth || textured || inst != nullptr; }
  unsigned long long msaa_seed = 0;
  // bytes of ray-tree frames one chunk of a radiance query may hold (rt_set_radiance_scratch_limit)
  std::atomic<size_t> radiance_limit{kRadianceDefaultLimit};
  std::vector<std::unique_ptr<Replica>> rep;  // rep[0]: the first (output) device
  std::mutex timing_mu;
  KernelTiming timing;
  // multi-device scenes: one RCCL communicator per device (single process, ncclCommInitAll);
  // multi_mu serialises the frames that use them.  copy_gather: the shares are gathered by
  // peer copies instead (a device listed twice: the one-GPU rehearsal of the deal / gather /
  // untile path)
  std::mutex multi_mu;
  std::vector<ncclComm_t> comms;
  bool multi = false;  // made by rt_scene_*_multi: frames go through render_multi (any count)
  bool copy_gather = false;
  // the communicators go first, then the timing events and each replica's buffers, events and
  // streams with their device current
  ~rt_scene() {
    for (ncclComm_t c : comms) (void)ncclCommDestroy(c);
    if (!rep.empty()) {
      DeviceGuard g(rep[0]->device, std::nothrow);
      timing.events.clear();
    }
    for (auto& r : rep) {
      DeviceGuard g(r->device, std::nothrow);
      r.reset();
    }
  }
};

namespace {

thread_local std::string g_error;

int set_error(int code, const std::string& msg) {
  g_error = msg;
  return code;
}

struct NcclFailure {
  ncclResult_t err;
  const char* what;
};

void nccl_check(ncclResult_t e, const char* what) {
  if (e != ncclSuccess) throw NcclFailure{e, what};
}

template <typename F>
int guarded(F&& f) {  // (the RCCL failures are this library's alone)
  return guarded_with(set_error, [&]() -> int {
    try {
      return f();
    } catch (const NcclFailure& h) {
      return set_error(RT_E_HIP, std::string(h.what) + ": " + ncclGetErrorString(h.err));
    }
  });
}

constexpr int kFrameFloats = 28;  // rt_kernels.hip kFrFields
constexpr size_t kTileFloats = (size_t)kTile * kTile * 3;

size_t frame_floats(const HostScene& h, int sel_tiles) {
  return (size_t)(h.max_depth + 1) * kFrameFloats * kTile * kTile * (size_t)std::max(1, sel_tiles);
}

int occ_words(const HostScene& h) { return std::max(1, ((int)h.lights.size() + 31) / 32); }

// A counter buffer: kCounterRows x kCounterWidth ray counters.
constexpr size_t kCounterAlloc = (size_t)kCounterWidth * kCounterRows;
// Dispatch order of the traversal kernels: heavy first within each XCD's
// part of the frame (RT_ORDER_REGIONS regions, one per XCD; 0 = block order), each region
// RT_ORDER_CHUNKS contiguous bands of the frame, chunk c in region c mod regions.  Two: an XCD's
// L2 still holds its bands' part of the tree (shadow kernel reads 91 vs 130 MB per C3 frame with
// interleaved half-row chunks, profiles/r03/ab_order_chunks.jsonl), and two bands half a frame
// apart even out the XCDs' shares of the heavy rows (C3 frame kernel 0.352 -> 0.339 ms one at a
// time, 0.327 -> 0.319 six in flight; 4 / 8 / 16 chunks 0.343 / 0.343 / 0.346;
// profiles/r06/ab_order_chunks.json).  The order never changes a result, only which tiles start
// first.  (Macros: A/B builds, `make exp EXTRA=-D...`.)
#ifndef RT_ORDER_REGIONS
#define RT_ORDER_REGIONS 8
#endif
#ifndef RT_ORDER_CHUNKS
#define RT_ORDER_CHUNKS 2
#endif
// Points P's schedule at `sched`, sched_words_for(P.num_sel_tiles) words (layout: rt_internal.h);
// P.num_sel_tiles is final.  (WorkSet::bind; beside it only the MSAA halo rows, which share
// their band's buffer, and a camera's cold order, which has its own.)
void set_schedule(RenderParams& P, unsigned* sched) {
  const int regions = RT_ORDER_REGIONS;
  P.tile_cost = regions ? sched : nullptr;
  P.unit_order = regions ? reinterpret_cast<int*>(sched) + P.num_sel_tiles : nullptr;
  P.order_regions = regions;
  P.order_chunk = RT_ORDER_CHUNKS;
}

// The untile kernel copies 16-B chunks when every frame row and both buffers are 16-B aligned.
int untile_vec(const UntileParams& U) {
  return (U.width % 4 == 0) && ((uintptr_t)U.out % 16 == 0) && ((uintptr_t)U.recv % 16 == 0);
}

// Estimated cost of every tile of camera c's whole frame, for the dispatch order of a frame
// without a previous one (the cold frame): 16 x (1 + the primitives whose
// projected bounds touch the tile, each weighted by 1 / |cos| of the angle between its normal
// and the view direction, at most 20).  Where many primitives project into one tile — surfaces
// seen edge-on — its rays walk more of the tree (C3: correlation 0.62 with measured tile times,
// 0.59 unweighted).  A point X projects to the image-plane point tl + su fx - sv fy that
// e + l (X - e) reaches (Cramer's rule; l > 0: in front of the camera); a primitive with a point
// not in front is left out.  Only the order depends on it, never a pixel.
std::vector<unsigned> cold_costs(const HostScene& h, const rt_camera& c) {
  const int tx = (c.width + kTile - 1) / kTile, ty = (c.height + kTile - 1) / kTile;
  std::vector<double> acc((size_t)tx * ty, 1.0);
  const double e[3] = {c.e[0], c.e[1], c.e[2]};
  const double nu[3] = {-c.s_u[0], -c.s_u[1], -c.s_u[2]}, sv[3] = {c.s_v[0], c.s_v[1], c.s_v[2]};
  const double r[3] = {c.top_left[0] - e[0], c.top_left[1] - e[1], c.top_left[2] - e[2]};
  auto cross = [](const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  double nuxsv[3], rxsv[3], nuxr[3];
  cross(nu, sv, nuxsv);
  cross(r, sv, rxsv);
  cross(nu, r, nuxr);
  const double lnum = dot(r, nuxsv);
  auto project = [&](const double* X, double& fx, double& fy) {
    const double a[3] = {X[0] - e[0], X[1] - e[1], X[2] - e[2]};
    const double det = dot(a, nuxsv);
    if (!(std::fabs(det) > 0.0) || !(lnum / det > 0.0)) return false;
    fx = dot(a, rxsv) / det;
    fy = dot(a, nuxr) / det;
    return std::isfinite(fx) && std::isfinite(fy);
  };
  for (const DevPrim& p : h.prims) {
    double pts[8][3];
    int n = 0;
    double weight = 1.0;
    if (p.kind == kPrimTriangle) {
      for (int k = 0; k < 3; k++) {
        pts[0][k] = p.v0[k];
        pts[1][k] = (double)p.v0[k] - p.a1[k];
        pts[2][k] = (double)p.v0[k] - p.a2[k];
      }
      n = 3;
      const double a1[3] = {p.a1[0], p.a1[1], p.a1[2]}, a2[3] = {p.a2[0], p.a2[1], p.a2[2]};
      double nrm[3];
      cross(a1, a2, nrm);
      const double d[3] = {(pts[0][0] + pts[1][0] + pts[2][0]) / 3 - e[0],
                           (pts[0][1] + pts[1][1] + pts[2][1]) / 3 - e[1],
                           (pts[0][2] + pts[1][2] + pts[2][2]) / 3 - e[2]};
      const double len = std::sqrt(dot(nrm, nrm) * dot(d, d));
      const double cosv = len > 0.0 ? std::fabs(dot(nrm, d)) / len : 1.0;
      weight = 1.0 / std::max(cosv, 0.05);
    } else {
      const double rad = std::fabs((double)p.a1[0]);
      for (int m = 0; m < 8; m++)
        for (int k = 0; k < 3; k++) pts[m][k] = p.v0[k] + (((m >> k) & 1) ? rad : -rad);
      n = 8;
    }
    double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
    bool ok = true;
    for (int m = 0; m < n && ok; m++) {
      double fx, fy;
      ok = project(pts[m], fx, fy);
      if (ok) {
        x0 = std::min(x0, fx), x1 = std::max(x1, fx);
        y0 = std::min(y0, fy), y1 = std::max(y1, fy);
      }
    }
    if (!ok || x1 < 0.0 || y1 < 0.0 || x0 >= c.width || y0 >= c.height) continue;
    const int a0 = std::max(0, (int)(x0 / kTile)), a1 = std::min(tx - 1, (int)(x1 / kTile));
    const int b0 = std::max(0, (int)(y0 / kTile)), b1 = std::min(ty - 1, (int)(y1 / kTile));
    for (int b = b0; b <= b1; b++)
      for (int a = a0; a <= a1; a++) acc[(size_t)b * tx + a] += weight;
  }
  std::vector<unsigned> est(acc.size());
  for (size_t i = 0; i < acc.size(); i++) est[i] = (unsigned)std::min(16.0 * acc[i], 4e9);
  return est;
}

RenderParams make_params(const rt_scene* s, const Replica& r, int cam, int row0, int row_stride,
                         int tile_begin, int tile_step, int tile_major, float* out,
                         unsigned long long* counters);

// Every orderable camera's whole-frame cold order on replica r (the order kernel over
// cold_costs), made once with the scene: a camera's first frame on a stream dispatches by it
// instead of in block order (launch_variant in rt_kernels.hip).
void seed_cold_orders(const rt_scene* s, Replica& r) {
  const HostScene& h = s->host;
  r.d_cold = std::vector<DevBuf<unsigned>>(h.cameras.size());
  if (s->tree_frames() || h.lights.empty()) return;  // (no warm order either)
  for (size_t cam = 0; cam < h.cameras.size(); cam++) {
    const rt_camera& c = h.cameras[cam];
    if (c.num_samples > 1) continue;
    const std::vector<unsigned> est = cold_costs(h, c);
    DevBuf<unsigned> buf;
    buf.reserve(sched_words_for(est.size()), "alloc cold order");
    hip_check(hipMemcpy(buf.p, est.data(), est.size() * sizeof(unsigned), hipMemcpyHostToDevice),
              "upload tile cost estimate");
    RenderParams P = make_params(s, r, (int)cam, 0, 1, 0, 1, 0, nullptr, nullptr);
    set_schedule(P, buf.p);
    if (launch_cold_order(P, nullptr)) r.d_cold[cam] = std::move(buf);
  }
  hip_check(hipDeviceSynchronize(), "cold orders");
}

// Every camera's entry cuts on replica r (entry_cuts.cpp), built on the host with
// the scene like the cold orders: the frame kernel's primary walks of a frame tile start at its
// record's nodes instead of the root.  Cameras whose frames the frame kernel does not render (ray
// trees, MSAA) get none, nor does a scene entry_cuts_apply turns down.  A table that cannot be
// built or uploaded leaves its camera without cuts; the scene is created all the same.
void seed_entry_cuts(const rt_scene* s, Replica& r) {
  const HostScene& h = s->host;
  r.d_cuts = std::vector<DevBuf<int>>(h.cameras.size());
  if (s->tree_frames() || !scene_entry_cuts_apply(h, max_supported_depth())) return;
  for (size_t cam = 0; cam < h.cameras.size(); cam++) {
    if (h.cameras[cam].num_samples > 1) continue;
    try {
      r.d_cuts[cam] = upload(build_entry_cuts(h, h.cameras[cam], nullptr), "upload entry cuts", 0);
    } catch (const std::exception&) {
      (void)hipGetLastError();
      r.d_cuts[cam] = DevBuf<int>();
    }
  }
}

// Tests only (rt_test_entry_cuts): 1 = no launch binds a table.
static std::atomic<int> g_test_entry_cuts{0};

// The camera's table for a launch whose logical tile rows are image tile rows — rows row0,
// row0 + 1, ... with row0 on a tile row — from that tile row on; any other selection of rows
// (strided rows, a band not cut at a tile row) walks from the root.  Tile deals, blocks, records
// and split tiles keep their frame tile and use it.
const int* bind_entry_cuts(const Replica& r, int cam, int row0, int row_stride, int tiles_x) {
  if (g_test_entry_cuts.load() == 1 || row_stride != 1 || row0 % kTile != 0 ||
      cam >= (int)r.d_cuts.size() || !r.d_cuts[cam].p)
    return nullptr;
  return r.d_cuts[cam].p + (size_t)(row0 / kTile) * tiles_x * kEntryCut;
}

// One tree's arrays on the current device (`mesh`: a base mesh's, in the allocation labels).
// +64 B: the kernels may fetch a record with one 64-byte scalar load past its 48 bytes
constexpr size_t kPad = 64;
Replica::TreeBufs upload_tree(const HostScene& h, bool mesh) {
  Replica::TreeBufs b;
  b.nodes = upload(h.nodes, mesh ? "upload mesh nodes" : "upload nodes", kPad);
  b.prims = upload(h.prims, mesh ? "upload mesh prims" : "upload prims", kPad);
  b.leaves = upload(h.leaves, mesh ? "upload mesh culling leaves" : "upload culling leaves", kPad);
  b.normals = upload(h.normals, mesh ? "upload mesh normals" : "upload normals", kPad);
  b.anc = upload(h.ancestry, mesh ? "upload mesh ancestry" : "upload ancestry", kPad);
  b.leaf_object = upload(h.leaf_object, mesh ? "upload mesh leaf objects" : "upload leaf objects", 0);
  return b;
}

// The flat scene's tree, surface data and textures.
void upload_flat(const HostScene& h, Replica& r) {
  r.d_tree = upload_tree(h, false);
  r.surf.num_leaves = (int)h.prims.size();
  if (!h.leaf_tri.empty()) {
    r.d_surf_tri = upload(h.leaf_tri, "upload leaf vertex ids", 0);
    r.surf.tri = r.d_surf_tri.p;
  }
  if (!h.vertex_normals.empty()) {
    r.d_surf_normals = upload(h.vertex_normals, "upload vertex normals", 0);
    r.surf.normals = r.d_surf_normals.p;
  }
  if (!h.vertex_uv.empty()) {
    r.d_surf_uv = upload(h.vertex_uv, "upload vertex uv", 0);
    r.surf.uv = r.d_surf_uv.p;
  }
  if (!h.textures.empty()) {
    r.d_tex_table = upload(h.textures, "upload texture table", 0);
    r.d_texels = upload(h.texels, "upload texels", 0);
    r.tex = TexParams{r.d_tex_table.p, r.d_texels.p, (int)h.textures.size(), h.blank_material};
  }
}

// An instanced scene's: every base mesh's arrays, the tables that point at them and the top-level
// tree.
void upload_instanced(const InstHost& ih, Replica& r) {
  std::vector<DevMesh> table(ih.meshes.size());
  r.d_mesh.resize(ih.meshes.size());
  for (size_t m = 0; m < ih.meshes.size(); m++) {
    const HostScene& h = ih.meshes[m];
    Replica::TreeBufs& b = r.d_mesh[m];
    b = upload_tree(h, true);
    DevMesh& dm = table[m];
    std::memset(&dm, 0, sizeof dm);
    dm.nodes = b.nodes.p;
    dm.leaves = b.leaves.p;
    dm.prims = b.prims.p;
    dm.anc = b.anc.p;
    dm.normals = b.normals.p;
    dm.leaf_object = b.leaf_object.p;
    dm.root_kind = h.root_kind;
    dm.root_ref = h.root_ref;
    // (the rule of use_fast in rt_kernels.hip: a culling tree only over a node root)
    const bool culled = h.accel_root >= 0 && h.root_kind == kRootNode && !h.leaves.empty();
    dm.accel_root = culled ? h.accel_root : -1;
    dm.accel_stride = h.accel_stride;
    std::memcpy(dm.root_box, h.root_box, sizeof dm.root_box);
    std::memcpy(dm.accel_box, h.accel_box, sizeof dm.accel_box);
    dm.quot_ok = h.quot_ok;
    dm.leaf_base = ih.mesh_leaf_base[m];
    dm.object_base = ih.mesh_object_base[m];
  }
  r.d_mesh_table = upload(table, "upload mesh table", kPad);
  r.d_instances = upload(ih.instances, "upload instances", kPad);
  r.d_top_nodes = upload(ih.top_nodes, "upload top-level nodes", kPad);
  r.d_top_prims = upload(ih.top_prims, "upload top-level primitives", kPad);
  r.d_top_normals = upload(ih.top_normals, "upload top-level normals", kPad);
  r.d_top_info = upload(ih.top_info, "upload top-level objects", 0);
  r.inst.top_nodes = r.d_top_nodes.p;
  r.inst.top_prims = r.d_top_prims.p;
  r.inst.top_normals = r.d_top_normals.p;
  r.inst.top_info = r.d_top_info.p;
  r.inst.instances = r.d_instances.p;
  r.inst.meshes = r.d_mesh_table.p;
  r.inst.top_root_kind = ih.top_root_kind;
  r.inst.top_quot_ok = ih.top_quot_ok;
  std::memcpy(r.inst.top_box, ih.top_box, sizeof r.inst.top_box);
  if (ih.has_motion) {  // (a table may be empty: nothing of that kind moves, and nothing reads it)
    r.d_motion_instances = upload(ih.motion_instances, "upload moving instances", kPad);
    r.d_motion_spheres = upload(ih.motion_spheres, "upload moving spheres", kPad);
    r.motion.instances = r.d_motion_instances.p;
    r.motion.spheres = r.d_motion_spheres.p;
  }
}

// The scene on replica r's device: its trees, then what every kind of scene has.  (An instanced
// scene gets no cold orders and no entry cuts: its frames are ray trees.)
void upload_replica(const rt_scene* s, Replica& r) {
  DeviceGuard g(r.device);
  if (s->inst)
    upload_instanced(*s->inst, r);
  else
    upload_flat(s->host, r);
  r.d_mats = upload(s->host.materials, "upload materials", kPad);
  r.d_lights = upload(s->host.lights, "upload lights", kPad);
  r.d_counters.reserve(kCounterAlloc, "alloc counters");
  hip_check(hipMemset(r.d_counters.p, 0, sizeof(unsigned long long) * kCounterAlloc), "zero counters");
  seed_cold_orders(s, r);
  seed_entry_cuts(s, r);
}

// The assembled scene on every device of the list.  `multi`: frames go through render_multi, with
// one RCCL communicator per device for the framebuffer gather.
void upload_scene(rt_scene* s, const std::vector<int>& devices, bool multi) {
  for (int d : devices) {
    s->rep.push_back(std::make_unique<Replica>());
    s->rep.back()->device = d;
    upload_replica(s, *s->rep.back());
  }
  s->multi = multi;
  if (multi) {
    std::vector<int> distinct = devices;
    std::sort(distinct.begin(), distinct.end());
    s->copy_gather = std::unique(distinct.begin(), distinct.end()) != distinct.end();
    if (!s->copy_gather) {
      s->comms.resize(devices.size());
      nccl_check(ncclCommInitAll(s->comms.data(), (int)devices.size(), devices.data()),
                 "ncclCommInitAll");
    }
  }
}

std::vector<int> device_list(int device_count, const int* devices) {
  int n = 0;
  hip_check(hipGetDeviceCount(&n), "hipGetDeviceCount");
  if (device_count < 1) throw std::invalid_argument("device_count must be >= 1");
  std::vector<int> out;
  for (int i = 0; i < device_count; i++) {
    const int d = devices ? devices[i] : i;
    if (d < 0 || d >= n)
      throw std::invalid_argument("device " + std::to_string(d) + " does not exist (" +
                                  std::to_string(n) + " visible)");
    out.push_back(d);
  }
  return out;
}

struct TilePlan {
  int rows, tiles_x, tiles_total;
};

TilePlan plan(const rt_camera& c, int row0, int row_stride) {
  TilePlan p;
  p.rows = row0 < c.height ? (c.height - row0 + row_stride - 1) / row_stride : 0;
  p.tiles_x = (c.width + kTile - 1) / kTile;
  p.tiles_total = p.tiles_x * ((p.rows + kTile - 1) / kTile);
  return p;
}

// The scene's part of the kernel parameters (no camera, no outputs): what a ray query needs.
RenderParams scene_params(const rt_scene* s, const Replica& r) {
  const HostScene& h = s->host;
  RenderParams P;
  std::memset(&P, 0, sizeof P);
  P.nodes = r.d_tree.nodes.p;
  P.leaves = r.d_tree.leaves.p;
  P.prims = r.d_tree.prims.p;
  P.normals = r.d_tree.normals.p;
  P.materials = r.d_mats.p;
  P.lights = r.d_lights.p;
  P.num_lights = (int)h.lights.size();
  P.max_depth = h.max_depth;
  std::memcpy(P.background, h.background, sizeof P.background);
  std::memcpy(P.ambient, h.ambient, sizeof P.ambient);
  P.eps = h.eps;
  P.root_kind = h.root_kind;
  P.root_ref = h.root_ref;
  std::memcpy(P.root_box, h.root_box, sizeof P.root_box);
  P.accel_root = h.accel_root;
  P.accel_stride = h.accel_stride;
  P.quot_ok = s->inst ? s->inst->top_quot_ok : h.quot_ok;  // (instanced: the loose triangles')
  std::memcpy(P.accel_box, h.accel_box, sizeof P.accel_box);
  P.anc = r.d_tree.anc.p;
  P.occ_words = occ_words(h);
  return P;
}

RenderParams make_params(const rt_scene* s, const Replica& r, int cam, int row0, int row_stride,
                         int tile_begin, int tile_step, int tile_major, float* out,
                         unsigned long long* counters) {
  const rt_camera& c = s->host.cameras[cam];
  RenderParams P = scene_params(s, r);
  std::memcpy(P.cam_e, c.e, 12);
  std::memcpy(P.cam_tl, c.top_left, 12);
  std::memcpy(P.cam_su, c.s_u, 12);
  std::memcpy(P.cam_sv, c.s_v, 12);
  P.width = c.width;
  P.height = c.height;
  const TilePlan tp = plan(c, row0, row_stride);
  P.row0 = row0;
  P.row_stride = row_stride;
  P.rows = tp.rows;
  P.tiles_x = tp.tiles_x;
  P.tiles_total = tp.tiles_total;
  P.tile_begin = tile_begin;
  P.tile_step = tile_step;
  P.block_deal = (tile_major & RT_TILE_BLOCKS) ? 1 : 0;
  const int units = P.block_deal ? deal_blocks(tp.tiles_x, tp.tiles_total / tp.tiles_x) : tp.tiles_total;
  const int sel_units = tile_begin < units ? (units - tile_begin + tile_step - 1) / tile_step : 0;
  P.num_sel_tiles = P.block_deal ? 4 * sel_units : sel_units;
  P.tile_major = tile_major & RT_TILE_MAJOR;
  P.records = (tile_major & RT_TILE_RECORDS) ? 1 : 0;
  P.out = out;
  P.counters = counters;
  if (row0 == 0 && row_stride == 1 && tile_begin == 0 && tile_step == 1 && !P.block_deal &&
      cam < (int)r.d_cold.size() && r.d_cold[cam].p) {  // the whole frame: its cold order
    P.cold_order = reinterpret_cast<const int*>(r.d_cold[cam].p) + P.num_sel_tiles;
    P.cold_tiles = P.num_sel_tiles;
  }
  P.entry_cuts = bind_entry_cuts(r, cam, row0, row_stride, tp.tiles_x);
  return P;
}

// P restricted to its first `rows` selected rows (rows row0 .. row0 + rows - 1 at stride 1):
// the band launches of a multi-device MSAA frame.
void limit_rows(RenderParams& P, int rows) {
  P.rows = std::min(P.rows, rows);
  P.tiles_total = P.tiles_x * ((P.rows + kTile - 1) / kTile);
  P.num_sel_tiles = P.tile_begin < P.tiles_total
                        ? (P.tiles_total - P.tile_begin + P.tile_step - 1) / P.tile_step
                        : 0;
}

// Pixel records (RT_TILE_RECORDS) carry the primary hit and up to kRecMaxLights shadow bits:
// pixel-centre cameras of scenes without mirror/dielectric recursion.
bool records_ok(const rt_scene* s, int cam) {
  return !s->inst && s->host.cameras[cam].num_samples <= 1 && !s->tree_frames() &&
         (int)s->host.lights.size() <= kRecMaxLights;
}

void check_render_args(const rt_scene* s, int cam, int row0, int row_stride) {
  if (!s) throw std::invalid_argument("scene is NULL");
  if (cam < 0 || cam >= (int)s->host.cameras.size())
    throw std::invalid_argument("camera index out of range");
  if (row0 < 0 || row_stride < 1) throw std::invalid_argument("bad row selection");
  // MSAA splats every sample into the 3x3 neighbourhood (HW2/Scene.cpp:48-62), so a row subset
  // is not a self-contained piece of the image: only whole frames are rendered.
  if (s->host.cameras[cam].num_samples > 1 && (row0 != 0 || row_stride != 1))
    throw std::domain_error("NumSamples > 1 renders whole frames only (starting_row 0, stride 1)");
}

unsigned powmod_minstd(unsigned a, unsigned e) {
  unsigned long long r = 1, b = a;
  while (e) {
    if (e & 1) r = r * b % kMinstdM;
    b = b * b % kMinstdM;
    e >>= 1;
  }
  return (unsigned)r;
}

// Folds the completed quads at the front of the pending list into the running sums.
void fold_timing(KernelTiming& t) {
  size_t k = 0;
  for (; k < t.pending.size(); k++) {
    auto& q = t.pending[k];
    if (hipEventQuery(q[3]) != hipSuccess) break;
    float a = 0, b = 0, c = 0;
    if (hipEventElapsedTime(&a, q[0], q[1]) != hipSuccess ||
        hipEventElapsedTime(&b, q[1], q[2]) != hipSuccess ||
        hipEventElapsedTime(&c, q[2], q[3]) != hipSuccess)
      break;
    t.sum[0] += a;
    t.sum[1] += b;
    t.sum[2] += c;
    t.sum[3] += (double)a + b + c;
    t.folded++;
    t.spare.push_back(q);
  }
  t.pending.erase(t.pending.begin(), t.pending.begin() + (long)k);
}

// Events for one timed launch (nullptr when timing is off or the launch renders nothing).
const hipEvent_t* timing_marks(rt_scene* s, const RenderParams& P) {
  if (!s->timing.on || P.num_sel_tiles <= 0) return nullptr;
  std::lock_guard<std::mutex> lk(s->timing_mu);
  KernelTiming& t = s->timing;
  if (t.pending.size() >= kTimingPending) fold_timing(t);
  if (t.spare.empty()) {
    std::array<hipEvent_t, 4> q{};
    for (hipEvent_t& e : q) {
      t.events.emplace_back();
      t.events.back().create(hipEventDefault, "timing event");
      e = t.events.back();
    }
    t.spare.push_back(q);
  }
  t.pending.push_back(t.spare.back());
  t.spare.pop_back();
  return t.pending.back().data();
}

// The surface data the SMOOTH kernel instantiations take: a smooth scene's (single-device: the
// surface creators make no other), else null — the flat instantiations.
const SurfParams* smooth_surface(const rt_scene* s) {
  return s->smooth ? &s->rep[0]->surf : nullptr;
}
// What the ray-tree launches take: a textured scene's textures (and then its surface data, smooth
// mesh or not: the TEX instantiations are SMOOTH ones), else null and the surface data as above.
const TexParams* tree_textures(const rt_scene* s) { return s->textured ? &s->rep[0]->tex : nullptr; }
const SurfParams* tree_surface(const rt_scene* s) {
  return s->textured ? &s->rep[0]->surf : smooth_surface(s);
}
// What the INST kernels take: an instanced scene's tables (single-device), else null.
const InstParams* inst_params(const rt_scene* s) { return s->inst ? &s->rep[0]->inst : nullptr; }
// What the motion kernels take beside them: the scene's motion tables with the call's traversal
// mode and whether its rays carry a time (RT_QUERY_RAY_TIME); a scene without motion: null, and
// the flag has no effect.
struct MotionCall {
  MotionParams m;
  bool on;
  const MotionParams* get() const { return on ? &m : nullptr; }
};
MotionCall motion_call(const rt_scene* s, int flags) {
  MotionCall c{};
  c.on = s->inst && s->inst->has_motion;
  if (c.on) {
    c.m = s->rep[0]->motion;
    c.m.fast = s->mode != RT_TRAVERSAL_REFERENCE ? 1 : 0;
    c.m.ray_time = (flags & RT_QUERY_RAY_TIME) ? 1 : 0;
  }
  return c;
}

// The sample passes of an MSAA camera (HW2/Scene.cpp:32-69) over P's rows: pass k renders
// sample k of every selected pixel into d_samples[k] (row-major, full-frame positions).
void enqueue_samples(rt_scene* s, const RenderParams& P, int samples, float* d_samples,
                     hipStream_t stream, bool timed) {
  const bool fast = s->mode != RT_TRAVERSAL_REFERENCE;
  const size_t frame = (size_t)P.width * P.height * 3;
  for (int k = 0; k < samples * samples; k++) {
    RenderParams Q = P;
    Q.msaa_n = samples;
    Q.msaa_s = k;
    Q.msaa_mul[0] = powmod_minstd(kMinstdA, 2 * k + 1);
    Q.msaa_mul[1] = powmod_minstd(kMinstdA, 2 * k + 2);
    Q.msaa_seed = s->msaa_seed;
    Q.tile_major = 0;
    Q.out = d_samples + (size_t)k * frame;
    hip_check(launch_render(Q, fast, s->deep, s->has_spheres, timed ? timing_marks(s, Q) : nullptr,
                            tree_surface(s), inst_params(s), motion_call(s, 0).get(),
                            tree_textures(s), stream),
              "render launch");
  }
}

// The splat + colour / weight of rows [row_lo, row_hi) into out (row-major, full frame).
void enqueue_resolve(rt_scene* s, int width, int height, int samples, const float* d_samples,
                     float* out, int row_lo, int row_hi, hipStream_t stream) {
  MsaaResolveParams M;
  M.samples = d_samples;
  M.out = out;
  M.width = width;
  M.height = height;
  M.n = samples;
  M.seed = s->msaa_seed;
  M.row_lo = row_lo;
  M.row_hi = row_hi;
  hip_check(launch_msaa_resolve(M, stream), "msaa resolve launch");
}

// One frame (or a tile subset of one) of camera `cam` into P.out.  Pixel-centre cameras: the
// render kernels write P.out directly.  MSAA cameras (HW2/Scene.cpp:32-69): one render pass per
// sample index into d_samples[s], then the resolve kernel's splat + colour / weight into P.out
// (row-major).  `timed`: this launch may take kernel-timing events (the first device only).
void enqueue_frame(rt_scene* s, const RenderParams& P, int samples, float* d_samples,
                   hipStream_t stream, bool timed) {
  const bool fast = s->mode != RT_TRAVERSAL_REFERENCE;
  if (samples <= 1) {
    hip_check(launch_render(P, fast, s->deep, s->has_spheres, timed ? timing_marks(s, P) : nullptr,
                            tree_surface(s), inst_params(s), motion_call(s, 0).get(),
                            tree_textures(s), stream),
              "render launch");
    return;
  }
  enqueue_samples(s, P, samples, d_samples, stream, timed);
  enqueue_resolve(s, P.width, P.height, samples, d_samples, P.out, 0, P.height, stream);
}

size_t sample_floats(const rt_camera& c) {
  return c.num_samples > 1 ? (size_t)c.num_samples * c.num_samples * c.width * c.height * 3 : 0;
}

RenderCtx* acquire_ctx(Replica& r) {
  {
    std::lock_guard<std::mutex> lk(r.mu);
    if (!r.ctx_free.empty()) {
      RenderCtx* c = r.ctx_free.back();
      r.ctx_free.pop_back();
      return c;
    }
  }
  DeviceGuard g(r.device);
  auto c = std::make_unique<RenderCtx>();
  c->stream.create();
  c->e0.create();
  c->e1.create();
  c->ev_in.create(hipEventDisableTiming);
  c->ev_out.create(hipEventDisableTiming);
  c->ev_gathered.create(hipEventDisableTiming);
  hip_check(hipEventRecord(c->ev_gathered, c->stream), "event record");  // (complete)
  c->d_cnt.reserve(kCounterAlloc, "alloc counters");
  std::lock_guard<std::mutex> lk(r.mu);
  r.ctx_all.push_back(std::move(c));
  return r.ctx_all.back().get();
}

void release_ctx(Replica& r, RenderCtx* c) {
  std::lock_guard<std::mutex> lk(r.mu);
  r.ctx_free.push_back(c);
}

// The context of caller stream `stream` on replica r (created on first use, then kept; the
// table is capped at kMaxStreamTables: the oldest caller stream's context goes back to the pool
// once its device stream has drained).  Caller holds s->multi_mu (no other multi-device frame
// is being enqueued).
RenderCtx* stream_ctx_for(Replica& r, void* stream) {
  RenderCtx* old = nullptr;
  {
    std::lock_guard<std::mutex> lk(r.mu);
    for (size_t k = 0; k < r.stream_ctx.size(); k++)
      if (r.stream_ctx[k].first == stream) {
        std::rotate(r.stream_ctx.begin() + (long)k, r.stream_ctx.begin() + (long)k + 1,
                    r.stream_ctx.end());  // most recently used last
        return r.stream_ctx.back().second;
      }
    if (r.stream_ctx.size() >= kMaxStreamTables) {
      old = r.stream_ctx.front().second;
      r.stream_ctx.erase(r.stream_ctx.begin());
    }
  }
  if (old) {
    DeviceGuard g(r.device);
    hip_check(hipStreamSynchronize(old->stream), "synchronize evicted context");
    release_ctx(r, old);
  }
  RenderCtx* c = acquire_ctx(r);
  std::lock_guard<std::mutex> lk(r.mu);
  r.stream_ctx.emplace_back(stream, c);
  return c;
}

// The contexts of one call, context d on replica d.
using CtxList = std::vector<RenderCtx*>;

// Pooled contexts of one synchronous call, one on each of the first n replicas: handed back on
// every path, after their streams have drained.
struct CtxLease {
  rt_scene* s;
  CtxList x;
  CtxLease(rt_scene* sc, size_t n) : s(sc) {
    for (size_t d = 0; d < n; d++) x.push_back(acquire_ctx(*s->rep[d]));
  }
  CtxLease(const CtxLease&) = delete;
  ~CtxLease() {
    for (size_t d = 0; d < x.size(); d++) {
      DeviceGuard g(s->rep[d]->device, std::nothrow);
      (void)hipStreamSynchronize(x[d]->stream);
      release_ctx(*s->rep[d], x[d]);
    }
  }
};

}  // namespace

void WorkSet::reserve_tiles(const HostScene& h, size_t tiles) {
  const size_t lanes = (size_t)kTile * kTile * tiles;
  occ.reserve((size_t)occ_words(h) * lanes, "alloc occlusion bits");
  sched.reserve((size_t)sched_words_for(tiles), "alloc tile schedule");
}

void WorkSet::bind(const rt_scene* s, const rt_camera& c, RenderParams& P) {
  reserve_tiles(s->host, (size_t)std::max(1, P.num_sel_tiles));
  P.occ = occ.p;
  set_schedule(P, sched.p);
  if (s->tree_frames()) {
    frames.reserve(frame_floats(s->host, P.num_sel_tiles), "alloc ray-tree frames");
    P.frames = frames.p;
  }
  if (c.num_samples > 1) samples.reserve(sample_floats(c), "alloc MSAA samples");
}

namespace {

void add_counters(const std::vector<unsigned long long>& cnt, rt_stats* stats) {
  for (int r = 0; r < kCounterRows; r++) {
    stats->primary_rays += (long long)cnt[kCounterWidth * r + kCntPrimary];
    stats->shadow_rays += (long long)cnt[kCounterWidth * r + kCntShadow];
    stats->secondary_rays += (long long)cnt[kCounterWidth * r + kCntSecondary];
    stats->primary_hits += (long long)cnt[kCounterWidth * r + kCntHits];
  }
}

// Replica r's ray counters since they were last taken (rt_collect_stats, rt_debug_counters).
std::vector<unsigned long long> take_counters(Replica& r) {
  DeviceGuard g(r.device);
  std::vector<unsigned long long> c(kCounterAlloc);
  hip_check(hipMemcpy(c.data(), r.d_counters.p, c.size() * sizeof c[0], hipMemcpyDeviceToHost),
            "read counters");
  hip_check(hipMemset(r.d_counters.p, 0, c.size() * sizeof c[0]), "reset counters");
  return c;
}

// One synchronous call's own ray counts and kernel time, counted in its contexts' buffers
// instead of the scene's: zeroes them and records e0 on the first context's stream; stop()
// records e1 there; read() waits for every context's stream and fills `stats` (nullable).
struct CallCounters {
  rt_scene* s;
  const CtxList& cx;
  CallCounters(rt_scene* sc, const CtxList& c) : s(sc), cx(c) {
    for (size_t d = 0; d < cx.size(); d++) {
      DeviceGuard g(s->rep[d]->device);
      hip_check(hipMemsetAsync(cx[d]->d_cnt.p, 0, sizeof(unsigned long long) * kCounterAlloc,
                               cx[d]->stream),
                "zero counters");
    }
    hip_check(hipEventRecord(cx[0]->e0, cx[0]->stream), "event record");
  }
  void stop() { hip_check(hipEventRecord(cx[0]->e1, cx[0]->stream), "event record"); }
  void read(rt_stats* stats) {
    std::vector<std::vector<unsigned long long>> cnt(cx.size(),
                                                     std::vector<unsigned long long>(kCounterAlloc));
    for (size_t d = 0; d < cx.size(); d++) {
      DeviceGuard g(s->rep[d]->device);
      hip_check(hipMemcpyAsync(cnt[d].data(), cx[d]->d_cnt.p, kCounterAlloc * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, cx[d]->stream),
                "copy counters");
    }
    for (size_t d = 0; d < cx.size(); d++) {
      DeviceGuard g(s->rep[d]->device);
      hip_check(hipStreamSynchronize(cx[d]->stream), "synchronize");
    }
    if (!stats) return;
    std::memset(stats, 0, sizeof *stats);
    for (auto& v : cnt) add_counters(v, stats);
    float ms = 0;
    hip_check(hipEventElapsedTime(&ms, cx[0]->e0, cx[0]->e1), "elapsed");
    stats->kernel_ms = ms;
  }
};

// Device d's share of a multi-device frame on its way to the first device: `words` 4-B words
// (floats or pixel records; 0: nothing to send) from src on device d to dst on the first.
struct GatherPart {
  const float* src;
  float* dst;
  size_t words;
};

// Orders `later` after what `earlier` holds so far, through event ev (both of the current device).
void order_after(hipStream_t later, hipStream_t earlier, hipEvent_t ev) {
  if (later == earlier) return;
  hip_check(hipEventRecord(ev, earlier), "event record");
  hip_check(hipStreamWaitEvent(later, ev, 0), "wait event");
}

// Lands part(d) of every device d > 0 on the first device, ordered after the work on device d's
// context stream and on the first device's.  Copy gather: ev_out of context d, a wait and a peer
// copy on the first device's stream, then ev_gathered there (the contexts' write-after-read
// fence); else one RCCL group of send / receive pairs.  Caller holds s->multi_mu and has the
// first device current.
template <typename Part>
void gather_parts(rt_scene* s, const CtxList& cx, Part&& part) {
  const int D = (int)s->rep.size();
  RenderCtx* x0 = cx[0];
  if (D == 1) return;  // the one device rendered the frame in place
  if (s->copy_gather) {
    for (int d = 1; d < D; d++) {
      const GatherPart g = part(d);
      if (!g.words) continue;
      {
        DeviceGuard gd(s->rep[d]->device);
        hip_check(hipEventRecord(cx[d]->ev_out, cx[d]->stream), "event record");
      }
      hip_check(hipStreamWaitEvent(x0->stream, cx[d]->ev_out, 0), "wait event");
      hip_check(hipMemcpyPeerAsync(g.dst, s->rep[0]->device, g.src, s->rep[d]->device,
                                   g.words * sizeof(float), x0->stream),
                "gather copy");
    }
    hip_check(hipEventRecord(x0->ev_gathered, x0->stream), "event record");
    return;
  }
  nccl_check(ncclGroupStart(), "ncclGroupStart");
  for (int d = 1; d < D; d++) {
    const GatherPart g = part(d);
    if (!g.words) continue;
    nccl_check(ncclSend(g.src, g.words, ncclFloat, 0, s->comms[d], cx[d]->stream), "ncclSend");
    nccl_check(ncclRecv(g.dst, g.words, ncclFloat, d, s->comms[0], x0->stream), "ncclRecv");
  }
  nccl_check(ncclGroupEnd(), "ncclGroupEnd");
}

// The untile / resolve kernels' view of a frame whose deal units (tiles, or 2x2 blocks with
// RT_UNTILE_BLOCKS) were dealt over `devices` slots of `slot` tiles; recv, out and vec are the
// caller's.
UntileParams untile_params(const rt_camera& c, const TilePlan& tp, int row0, int row_stride,
                           int devices, int slot, int tile_offset, int flags) {
  UntileParams U;
  U.recv = nullptr;
  U.out = nullptr;
  U.width = c.width;
  U.row0 = row0;
  U.row_stride = row_stride;
  U.rows = tp.rows;
  U.tiles_x = tp.tiles_x;
  U.tiles_total = tp.tiles_total;
  U.devices = devices;
  U.slot = slot;
  U.tile_offset = tile_offset % devices;
  U.blocks = (flags & RT_UNTILE_BLOCKS) ? 1 : 0;
  U.skip_root = (flags & RT_UNTILE_SKIP_ROOT) ? 1 : 0;
  U.vec = 0;
  return U;
}

// The argument checks rt_untile_device and rt_resolve_device (`records`) share, under the
// caller's name `fn`; returns the frame's UntileParams (recv, out and vec left to the caller).
UntileParams checked_untile_params(const char* fn, bool records, const rt_scene* s, int cam,
                                   int row0, int row_stride, int devices, int slot,
                                   int tile_offset, int flags, const void* d_gathered,
                                   const float* d_out) {
  check_render_args(s, cam, row0, row_stride);
  if (devices < 1 || slot < 0 || tile_offset < 0 || !d_gathered || !d_out ||
      (flags & ~(RT_UNTILE_BLOCKS | RT_UNTILE_SKIP_ROOT)) || ((flags & RT_UNTILE_BLOCKS) && slot % 4))
    throw std::invalid_argument(std::string(fn) + ": bad argument");
  if (records && !records_ok(s, cam)) throw std::domain_error(std::string(fn) + ": no pixel records here");
  const rt_camera& c = s->host.cameras[cam];
  const TilePlan tp = plan(c, row0, row_stride);
  const bool blocks = flags & RT_UNTILE_BLOCKS;
  const long long units = blocks ? deal_blocks(tp.tiles_x, tp.tiles_total / tp.tiles_x) : tp.tiles_total;
  if ((long long)devices * (blocks ? slot / 4 : slot) < units)
    throw std::invalid_argument(std::string(fn) + ": devices * slot is smaller than the frame's share");
  return untile_params(c, tp, row0, row_stride, devices, slot, tile_offset, flags);
}

// One frame of an MSAA camera over every device of a multi-device scene (the
// Gaussian splat of HW2/Scene.cpp:51-63 reaches the 3x3 neighbours, so pixels do not shard as
// independent tiles).  Device d owns the band of rows [H*d/D, H*(d+1)/D) and renders every
// sample pass over its band plus a one-row halo on each side (the halo rows' samples are
// recomputed, bit for bit: each pixel's generators depend only on the seed and the pixel, §7),
// resolves its band, and one RCCL group of send / receive pairs lands the bands in d_frame on
// the first device.  Halo launches carry no counters, so the ray counts are one frame's.
// Caller holds s->multi_mu.
void render_multi_msaa(rt_scene* s, const CtxList& cx, int cam, float* d_frame, hipStream_t s0,
                       bool per_call) {
  const int D = (int)s->rep.size();
  const rt_camera& c = s->host.cameras[cam];
  const int H = c.height, W = c.width, n = c.num_samples;
  const size_t frame = (size_t)W * H * 3;
  RenderCtx* x0 = cx[0];
  {
    DeviceGuard g(s->rep[0]->device);
    order_after(x0->stream, s0, x0->ev_in);  // d_frame's earlier work
  }
  for (int d = 0; d < D; d++) {
    const int lo = (int)((long long)H * d / D), hi = (int)((long long)H * (d + 1) / D);
    if (hi <= lo) continue;
    Replica& r = *s->rep[d];
    RenderCtx* x = cx[d];
    DeviceGuard g(r.device);
    float* dst = d_frame;
    // copy gather: the previous frame's band copy out of d_image (on the first device's
    // stream) has finished before this frame renders into it
    if (d > 0 && s->copy_gather) hip_check(hipStreamWaitEvent(x->stream, x0->ev_gathered, 0), "wait event");
    if (d > 0) {
      x->d_image.reserve(frame, "alloc band frame");
      dst = x->d_image.p;
    }
    RenderParams P = make_params(s, r, cam, lo, 1, 0, 1, 0, dst, per_call ? x->d_cnt.p : r.d_counters.p);
    limit_rows(P, hi - lo);
    WorkSet& ws = x->work;
    ws.bind(s, c, P);
    enqueue_samples(s, P, n, ws.samples.p, x->stream, d == 0);
    for (const int row : {lo - 1, hi}) {  // the halo rows the splat of the band's edges reads
      if (row < 0 || row >= H) continue;
      RenderParams Q = make_params(s, r, cam, row, 1, 0, 1, 0, dst, nullptr);
      limit_rows(Q, 1);
      Q.occ = P.occ;  // a halo row shares the band's buffers (it has no more tiles)
      Q.frames = P.frames;
      set_schedule(Q, ws.sched.p);
      enqueue_samples(s, Q, n, ws.samples.p, x->stream, false);
    }
    enqueue_resolve(s, W, H, n, ws.samples.p, dst, lo, hi, x->stream);
  }
  DeviceGuard g(s->rep[0]->device);
  gather_parts(s, cx, [&](int d) {  // device d's band (an empty one is skipped)
    const int lo = (int)((long long)H * d / D), hi = (int)((long long)H * (d + 1) / D);
    const size_t off = (size_t)lo * W * 3;
    return GatherPart{cx[d]->d_image.p + off, d_frame + off, (size_t)(hi - lo) * W * 3};
  });
  order_after(s0, x0->stream, x0->ev_out);
}

// One frame (rows row0 + k*row_stride) of a pixel-centre camera over every device of a
// multi-device scene, into the row-major frame d_frame on the first device, ordered on its
// stream s0.  The frame's 2x2-tile blocks are dealt round-robin over the D devices in deal
// order (the reference's row interleave over threads, HW2/main.cpp:33-36, at block
// granularity; block d -> device d mod D, deal_block_tile); each device renders its blocks
// tile-major into a slot of 4 ceil(B / D) tiles on its context's stream — as 32-bit pixel
// records where records_ok (a third of RGB's bytes), else RGB; one RCCL group of send / receive
// pairs (single process, one communicator per device) gathers the slots onto the first device,
// whose resolve kernel shades the records into the rows (or untile kernel copies the RGB).
// Counters: `per_call` adds each device's rays to its context's counters (rt_render's stats),
// else to the replica's (rt_collect_stats).  Caller holds s->multi_mu.
void render_multi(rt_scene* s, const CtxList& cx, int cam, int row0, int row_stride, float* d_frame,
                  hipStream_t s0, bool per_call) {
  const int D = (int)s->rep.size();
  const rt_camera& c = s->host.cameras[cam];
  const TilePlan tp = plan(c, row0, row_stride);
  if (tp.tiles_total == 0) return;
  const int blocks = deal_blocks(tp.tiles_x, tp.tiles_total / tp.tiles_x);
  const int slot = 4 * ((blocks + D - 1) / D);  // tiles: whole 2x2 blocks (block deal)
  // the other devices' shares travel as 32-bit pixel records where the scene allows, else as RGB
  const bool records = records_ok(s, cam);
  const size_t tile_words = records ? (size_t)kTile * kTile : (size_t)kTileFloats;
  RenderCtx* x0 = cx[0];
  {
    // the first device renders its own blocks in place into d_frame (after d_frame's earlier
    // work); the others render tile-major into their slots for the gather
    DeviceGuard g(s->rep[0]->device);
    order_after(x0->stream, s0, x0->ev_in);
  }
  for (int d = 0; d < D; d++) {
    Replica& r = *s->rep[d];
    RenderCtx* x = cx[d];
    DeviceGuard g(r.device);
    // copy gather: the previous frame's peer copy out of d_out (on the first device's stream)
    // has finished before this frame renders into it
    if (d > 0 && s->copy_gather) hip_check(hipStreamWaitEvent(x->stream, x0->ev_gathered, 0), "wait event");
    if (d > 0) x->d_out.reserve((size_t)slot * tile_words, "alloc tile slot");
    RenderParams P = make_params(s, r, cam, row0, row_stride, d, D,
                                 d == 0 ? RT_TILE_BLOCKS
                                        : RT_TILE_MAJOR | RT_TILE_BLOCKS | (records ? RT_TILE_RECORDS : 0),
                                 d == 0 ? d_frame : x->d_out.p, per_call ? x->d_cnt.p : r.d_counters.p);
    x->work.bind(s, c, P);
    enqueue_frame(s, P, 1, nullptr, x->stream, d == 0);
  }
  DeviceGuard g(s->rep[0]->device);
  x0->d_recv.reserve((size_t)D * slot * tile_words, "alloc gathered slots");
  const size_t count = (size_t)slot * tile_words;  // 4-B words (floats or pixel records)
  gather_parts(s, cx, [&](int d) {
    return GatherPart{cx[d]->d_out.p, x0->d_recv.p + (size_t)d * count, count};
  });
  // (skip root: the first device's blocks are already in d_frame)
  UntileParams U = untile_params(c, tp, row0, row_stride, D, slot, 0,
                                 RT_UNTILE_BLOCKS | RT_UNTILE_SKIP_ROOT);
  U.recv = x0->d_recv.p;
  U.out = d_frame;
  U.vec = untile_vec(U);
  if (D > 1 && records) {  // the others' pixel records shaded into the frame
    const RenderParams P0 = make_params(s, *s->rep[0], cam, row0, row_stride, 0, 1, 0, d_frame,
                                        nullptr);
    U.vec = 0;
    hip_check(launch_resolve(P0, U, s->has_spheres, x0->stream), "resolve launch");
  } else if (D > 1) {
    hip_check(launch_untile(U, x0->stream), "untile launch");
  }
  order_after(s0, x0->stream, x0->ev_out);
}

// Frees the least recently used scratch no host thread is enqueueing on (its mutex is free:
// holders of a scratch pointer keep it locked, and new ones need r.mu), after the GPU work of
// its last frame.  Caller holds r.mu.
void evict_scratch(Replica& r) {
  size_t victim = r.streams.size();
  for (size_t k = 0; k < r.streams.size(); k++) {
    if (!r.streams[k]->mu.try_lock()) continue;
    r.streams[k]->mu.unlock();
    if (victim == r.streams.size() || r.streams[k]->used < r.streams[victim]->used) victim = k;
  }
  if (victim == r.streams.size()) return;  // every one in use: let the table grow
  StreamScratch& x = *r.streams[victim];
  if (x.done) hip_check(hipEventSynchronize(x.done), "synchronize evicted scratch");
  r.streams.erase(r.streams.begin() + (long)victim);
}

// The scratch of `stream` on replica r, returned with its mutex held in `held`: allocated on
// first use at the largest camera's size; beyond kMaxStreamTables streams the least recently
// used one is evicted.
StreamScratch* scratch_for(rt_scene* s, Replica& r, void* stream, std::unique_lock<std::mutex>& held) {
  std::lock_guard<std::mutex> lk(r.mu);
  for (auto& x : r.streams)
    if (x->stream == stream) {
      held = std::unique_lock<std::mutex>(x->mu);
      x->used = ++r.tick;
      return x.get();
    }
  if (r.streams.size() >= kMaxStreamTables) evict_scratch(r);
  auto x = std::make_unique<StreamScratch>();
  x->stream = stream;
  x->used = ++r.tick;
  x->done.create(hipEventDisableTiming);
  // (growing them later would free buffers the stream's frames in flight use: hipFree waits)
  x->work.reserve_tiles(s->host, s->most / (kTile * kTile));
  r.streams.push_back(std::move(x));
  held = std::unique_lock<std::mutex>(r.streams.back()->mu);
  return r.streams.back().get();
}

// Where a creation entry puts its scene: on one device (< 0: the current one), or, `multi`, on a
// list of them (`ids` null: 0 .. count - 1).
struct DeviceChoice {
  int device = -1;
  int count = 0;
  const int* ids = nullptr;
  bool multi = false;
};

std::vector<int> resolve_devices(const DeviceChoice& c) {
  if (c.multi) return device_list(c.count, c.ids);
  int device = c.device;
  if (device < 0) hip_check(hipGetDevice(&device), "hipGetDevice");
  return {device};
}

// Every rt_scene_create* / rt_scene_load_xml* entry: the NULL checks (`given`:
// the entry's description or path), what `fill` makes of the entry's arguments (a description
// entry sets f.in, a scene-file entry loads f), the whole host build, and only then the first HIP
// call: the devices, the upload.
template <typename Fill>
int create_scene(const char* entry, bool given, const DeviceChoice& where, rt_scene** out,
                 Fill&& fill) {
  if (!given || !out) return set_error(RT_E_INVALID, std::string(entry) + ": NULL argument");
  *out = nullptr;
  auto s = std::make_unique<rt_scene>();
  const int rc = guarded([&] {
    SceneFile f;
    f.in.entry = entry;
    fill(f);
    assemble_scene(f.in, max_supported_depth(), *s);
    upload_scene(s.get(), resolve_devices(where), where.multi);
    return RT_OK;
  });
  if (rc != RT_OK) return rc;
  *out = s.release();
  return RT_OK;
}

// A description entry: the descriptors as they came (all but `desc` may be null).
int create_from_desc(const char* entry, const DeviceChoice& where, rt_scene** out,
                     const rt_scene_desc* desc, const rt_surface_desc* surface = nullptr,
                     const rt_texture_desc* textures = nullptr,
                     const rt_instance_desc* instances = nullptr,
                     const rt_motion_desc* motion = nullptr) {
  return create_scene(entry, desc != nullptr, where, out, [&](SceneFile& f) {
    f.in.desc = desc;
    f.in.surface = surface;
    f.in.textures = textures;
    f.in.instances = instances;
    f.in.motion = motion;
  });
}

// A scene-file entry: the descriptors load_scene_file makes of the file.
int create_from_file(const char* entry, const DeviceChoice& where, rt_scene** out,
                     const char* xml_path, const SceneFileOptions& opt) {
  return create_scene(entry, xml_path != nullptr, where, out,
                      [&](SceneFile& f) { load_scene_file(entry, xml_path, opt, f); });
}

DeviceChoice on_device(int device) { return {device, 0, nullptr, false}; }
DeviceChoice on_devices(int count, const int* ids) { return {-1, count, ids, true}; }

// Argument rules shared by the ray-query and radiance-query entries; they need no GPU.
void check_query_args(const char* fn, const rt_scene* s, const void* rays, long long n,
                      const void* out, bool out_aligned, int flags, int known_flags) {
  const std::string f(fn);
  if (n < 0) throw std::invalid_argument(f + ": n < 0");
  if (flags & ~known_flags) throw std::invalid_argument(f + ": unknown flag bit");
  if (n > 0 && (!rays || !out)) throw std::invalid_argument(f + ": NULL pointer");
  if ((uintptr_t)rays % 16 != 0 || (out_aligned && (uintptr_t)out % 16 != 0))
    throw std::invalid_argument(f + ": rays and hits must be 16-byte aligned");
  if (!s) throw std::invalid_argument(f + ": scene is NULL");
  if (s->multi) throw std::domain_error(f + ": ray queries on multi-device scenes are not supported");
}

// The caller's light records of a `_lit` entry: n k of them, or k with RT_QUERY_LIGHTS_SHARED.
struct LightList {
  const rt_light_sample* lights;
  int k;
};
constexpr int kLitFlags = RT_QUERY_LIGHTS_SHARED | RT_QUERY_NO_SCENE_LIGHTS;

// The `_lit` entries' own argument rules; they need no GPU.
void check_light_args(const char* fn, const LightList& l, int flags) {
  const std::string f(fn);
  const int most = (flags & RT_QUERY_LIGHTS_SHARED) ? kLitMaxShared : kLitMaxPerRay;
  if (l.k < 0 || l.k > most)
    throw std::invalid_argument(f + ": k must be in [0, 256] per ray, [0, 65535] shared");
  if (l.k > 0 && !l.lights) throw std::invalid_argument(f + ": NULL pointer (lights)");
  if (l.k > 0 && (uintptr_t)l.lights % 16 != 0)
    throw std::invalid_argument(f + ": lights must be 16-byte aligned");
}

size_t light_records(const LightList& l, long long n, int flags) {
  return (flags & RT_QUERY_LIGHTS_SHARED) ? (size_t)l.k : (size_t)n * (size_t)l.k;
}

// One query call: n rays and their n results in device memory; a radiance query's depth; a lit
// radiance query's light records in device memory (k == 0: none).
struct QueryCall {
  const rt_ray* rays;
  long long n;
  void* out;
  int depth, flags;
  LightList lit{nullptr, 0};
};

// What the front ends (query_device, query_host) know of a kind of query.  `enqueue` enqueues a
// call on `stream`, at most kQueryMaxLaunch rays per launch, with the stream's working set.
struct QueryKind {
  size_t stride;     // bytes of one result record
  bool out_aligned;  // results at a 16-byte aligned address
  int known_flags;
  bool radiance;  // takes a depth (radiance_depth) and counts its rays into `counters`
  void (*enqueue)(rt_scene* s, const Replica& r, const QueryCall& q, WorkSet& ws,
                  unsigned long long* counters, hipStream_t stream);
};

// The kernels' view of a batch before its rays: the leaf -> object table and the box the reorder
// stage cuts into origin cells (a root primitive: one cell).
QueryParams query_params(const rt_scene* s, const Replica& r) {
  const HostScene& h = s->host;
  QueryParams Q;
  std::memset(&Q, 0, sizeof Q);
  Q.leaf_object = r.d_tree.leaf_object.p;
  const float* root_box = s->inst ? s->inst->top_box : h.root_box;
  if (s->inst ? s->inst->top_root_kind == kTopNode : h.root_kind == kRootNode)
    for (int a = 0; a < 3; a++) {
      const float ext = root_box[a + 3] - root_box[a];
      Q.box_lo[a] = root_box[a];
      Q.box_scale[a] = ext > 0.0f && std::isfinite(ext) ? 1.0f / ext : 0.0f;  // cells: kernel
    }
  return Q;
}

// Points Q's reorder stage at ws.query for a launch of n rays: the permutation, then the
// histogram, then the totals.  (A call's first launch is its largest.)
void carve_reorder(QueryParams& Q, WorkSet& ws, long long n) {
  ws.query.reserve(query_scratch_words(n), "alloc query scratch");
  Q.perm_out = reinterpret_cast<int*>(ws.query.p);
  Q.hist = ws.query.p + n;
  Q.totals = Q.hist + (size_t(1) << query_bin_bits(n));
}

// Closest hits (rt_ray_hit records) or occlusion flags (bytes).
template <bool OCCLUSION>
void enqueue_hits(rt_scene* s, const Replica& r, const QueryCall& q, WorkSet& ws,
                  unsigned long long*, hipStream_t stream) {
  const RenderParams P = scene_params(s, r);
  const bool reorder = (q.flags & RT_QUERY_REORDER) != 0;
  const size_t stride = OCCLUSION ? 1 : sizeof(rt_ray_hit);
  QueryParams Q = query_params(s, r);
  for (long long done = 0; done < q.n; done += kQueryMaxLaunch) {
    Q.rays = q.rays + done;
    Q.out = static_cast<char*>(q.out) + (size_t)done * stride;
    Q.n = std::min(q.n - done, kQueryMaxLaunch);
    if (reorder) carve_reorder(Q, ws, Q.n);
    if (s->inst) {
      hip_check(launch_inst_query(P, Q, r.inst, OCCLUSION, reorder,
                                  s->mode != RT_TRAVERSAL_REFERENCE, s->has_spheres,
                                  motion_call(s, q.flags).get(), stream),
                "query launch");
      continue;
    }
    hip_check(launch_query(P, Q, r.d_tree.nodes.p, OCCLUSION, reorder, s->mode != RT_TRAVERSAL_REFERENCE,
                           s->deep, s->has_spheres, smooth_surface(s), stream),
              "query launch");
  }
}

// The depth a radiance query runs at: -1 = the scene's maximum.
int radiance_depth(const char* fn, const rt_scene* s, int depth) {
  if (depth < -1 || depth > s->host.max_depth)
    throw std::invalid_argument(std::string(fn) + ": depth must be -1 or 0 .. MaxRecursionDepth");
  return depth < 0 ? s->host.max_depth : depth;
}

size_t round_up_wave(long long n) { return (size_t)((n + 63) / 64 * 64); }

// Radiance (rt_radiance records) at q.depth.  ws.frames holds the ray-tree frames of one chunk;
// a query that cannot recurse touches neither it nor the limit.
void enqueue_radiance(rt_scene* s, const Replica& r, const QueryCall& q, WorkSet& ws,
                      unsigned long long* counters, hipStream_t stream) {
  const long long n = q.n;
  const int depth = q.depth;
  DevBuf<float>& frames = ws.frames;
  RenderParams P = scene_params(s, r);
  P.counters = counters;
  if (q.flags & RT_QUERY_NO_SCENE_LIGHTS) P.num_lights = 0;
  const bool reorder = (q.flags & RT_QUERY_REORDER) != 0;
  const bool shared = (q.flags & RT_QUERY_LIGHTS_SHARED) != 0;
  const bool recurse = depth > 0 && s->needs_recursion;
  QueryParams Q = query_params(s, r);
  long long chunk = kQueryMaxLaunch;  // rays per launch
  if (recurse) {
    const long long fit = (long long)(s->radiance_limit.load() / radiance_frame_bytes(depth)) /
                          kRadianceChunkUnit * kRadianceChunkUnit;
    if (fit < kRadianceChunkUnit)
      throw std::invalid_argument("radiance scratch limit below one wave's ray-tree frames");
    chunk = std::min(chunk, fit);
    frames.reserve(std::min((size_t)chunk, round_up_wave(n)) * kRadianceFrameFloats * (size_t)(depth + 1),
                   "alloc ray-tree frames");
  }
  RadianceParams R;
  R.frames = recurse ? frames.p : nullptr;
  R.lanes = (long long)std::min((size_t)chunk, round_up_wave(n));
  R.depth = depth;
  R.in_medium = (q.flags & RT_QUERY_IN_MEDIUM) ? 1 : 0;
  // one permutation per kQueryMaxLaunch rays (32-bit entries), then that part chunk by chunk
  for (long long done = 0; done < n; done += kQueryMaxLaunch) {
    const long long part = std::min(n - done, kQueryMaxLaunch);
    Q.rays = q.rays + done;
    Q.out = static_cast<rt_radiance*>(q.out) + done;
    Q.n = part;
    Q.perm = nullptr;
    // a ray's records follow its index in this part, whatever chunk or order it is traced in
    const LitParams lit{q.lit.lights + (shared ? 0 : (size_t)done * (size_t)q.lit.k), q.lit.k,
                        shared ? 1 : 0};
    if (reorder) {
      carve_reorder(Q, ws, part);
      hip_check(launch_query_sort(Q, stream), "query sort launch");
      Q.perm = Q.perm_out;
    }
    for (R.first = 0; R.first < part; R.first += chunk) {
      QueryParams C = Q;
      C.n = std::min(part, R.first + chunk);
      hip_check(launch_radiance(P, C, R, q.lit.k > 0 ? &lit : nullptr, r.d_tree.nodes.p,
                                s->mode != RT_TRAVERSAL_REFERENCE, s->deep, s->has_spheres,
                                tree_surface(s), inst_params(s), motion_call(s, q.flags).get(),
                                tree_textures(s), stream),
                "radiance query launch");
    }
  }
}

const QueryKind kClosestHit{sizeof(rt_ray_hit), true, RT_QUERY_REORDER | RT_QUERY_RAY_TIME, false,
                            enqueue_hits<false>};
const QueryKind kOcclusion{1, false, RT_QUERY_REORDER | RT_QUERY_RAY_TIME, false,
                           enqueue_hits<true>};
const QueryKind kRadiance{sizeof(rt_radiance), true,
                          RT_QUERY_REORDER | RT_QUERY_IN_MEDIUM | RT_QUERY_RAY_TIME, true,
                          enqueue_radiance};
const QueryKind kRadianceLit{sizeof(rt_radiance), true,
                             RT_QUERY_REORDER | RT_QUERY_IN_MEDIUM | RT_QUERY_RAY_TIME | kLitFlags,
                             true, enqueue_radiance};

// The front end of the `_device` entries: rays and results in device memory, enqueued on the
// caller's stream with its working set; the ray counts go to the scene's counters.
int query_device(const char* fn, const QueryKind& kind, rt_scene* s, const rt_ray* d_rays,
                 long long n, int depth, void* d_out, int flags, void* stream,
                 const LightList* lit = nullptr) {
  return guarded([&] {
    if (lit) check_light_args(fn, *lit, flags);
    check_query_args(fn, s, d_rays, n, d_out, kind.out_aligned, flags, kind.known_flags);
    if (kind.radiance) depth = radiance_depth(fn, s, depth);
    if (n == 0) return RT_OK;
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    std::unique_lock<std::mutex> lk;
    StreamScratch* sc = scratch_for(s, r, stream, lk);
    QueryCall q{d_rays, n, d_out, depth, flags};
    if (lit) q.lit = *lit;
    kind.enqueue(s, r, q, sc->work, r.d_counters.p, (hipStream_t)stream);
    hip_check(hipEventRecord(sc->done, (hipStream_t)stream), "event record");
    return RT_OK;
  });
}

// The host `_lit` entries' light records, uploaded on the context's stream.
LightList upload_lights(RenderCtx* x, const LightList& l, long long n, int flags) {
  const size_t count = light_records(l, n, flags);
  x->d_lit.reserve(count, "alloc light records");
  hip_check(hipMemcpyAsync(x->d_lit.p, l.lights, count * sizeof(rt_light_sample),
                           hipMemcpyHostToDevice, x->stream), "upload light records");
  return {x->d_lit.p, l.k};
}

// The front end of the host entries: rays up, the query on a pooled context, results down.  A
// radiance query reports its own ray counts and kernel time in `stats` (nullable), as rt_render.
int query_host(const char* fn, const QueryKind& kind, rt_scene* s, const rt_ray* rays, long long n,
               int depth, void* out, int flags, rt_stats* stats, const LightList* lit = nullptr) {
  return guarded([&] {
    if (lit) check_light_args(fn, *lit, flags);
    check_query_args(fn, s, rays, n, out, kind.out_aligned, flags, kind.known_flags);
    if (kind.radiance) depth = radiance_depth(fn, s, depth);
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return RT_OK;
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    CtxLease lease(s, 1);
    RenderCtx* x = lease.x[0];
    const size_t out_bytes = (size_t)n * kind.stride;
    x->d_rays.reserve((size_t)n, "alloc rays");
    x->d_ray_out.reserve((out_bytes + sizeof(rt_ray_hit) - 1) / sizeof(rt_ray_hit), "alloc results");
    hip_check(hipMemcpyAsync(x->d_rays.p, rays, (size_t)n * sizeof(rt_ray), hipMemcpyHostToDevice,
                             x->stream), "upload rays");
    QueryCall q{x->d_rays.p, n, x->d_ray_out.p, depth, flags};
    if (lit && lit->k > 0) q.lit = upload_lights(x, *lit, n, flags);
    std::optional<CallCounters> counted;
    if (kind.radiance) counted.emplace(s, lease.x);
    kind.enqueue(s, r, q, x->work, counted ? x->d_cnt.p : nullptr, x->stream);
    if (counted) counted->stop();
    hip_check(hipMemcpyAsync(out, q.out, out_bytes, hipMemcpyDeviceToHost, x->stream),
              "download results");
    if (counted)
      counted->read(stats);
    else
      hip_check(hipStreamSynchronize(x->stream), "synchronize query");
    return RT_OK;
  });
}

// One rt_render call: rows row0 + k row_stride of camera `cam` into the caller's frame `out`.
struct HostFrame {
  rt_scene* s;
  int cam, row0, row_stride;
  float* out;
  const rt_camera& camera() const { return s->host.cameras[cam]; }
};

// The selection's rows [lr0, lr1) from the device frame to the caller's (strided 2D copies
// leave the rows outside the selection untouched).
void copy_rows(const HostFrame& f, const float* d_frame, int lr0, int lr1, hipStream_t st) {
  if (lr1 <= lr0) return;
  const rt_camera& c = f.camera();
  const size_t row_bytes = (size_t)c.width * 3 * sizeof(float);
  const size_t off = (size_t)(f.row0 + (size_t)lr0 * f.row_stride) * c.width * 3;
  hip_check(hipMemcpy2DAsync(f.out + off, row_bytes * f.row_stride, d_frame + off,
                             row_bytes * f.row_stride, row_bytes, (size_t)(lr1 - lr0),
                             hipMemcpyDeviceToHost, st),
            "copy rows");
}

// The device-visible address of a caller buffer in pinned host memory (hipHostMalloc /
// registered, e.g. torch pin_memory); nullptr for pageable memory.
float* pinned_device_pointer(float* host) {
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, host, 0) == hipSuccess && dp) return static_cast<float*>(dp);
  (void)hipGetLastError();  // pageable memory: not an error here
  return nullptr;
}

// rt_render into pinned memory: the frame kernel writes the caller's buffer itself, through
// its device-visible address `direct`; no copy.
void render_pinned(const HostFrame& f, RenderCtx* x, float* direct, CallCounters& counted) {
  rt_scene* s = f.s;
  Replica& r = *s->rep[0];
  RenderParams P = make_params(s, r, f.cam, f.row0, f.row_stride, 0, 1, 0, direct, x->d_cnt.p);
  x->work.bind(s, f.camera(), P);
  // block order: the frame is bound by its writes over PCIe, which the heavy-first (cold)
  // order scatters (0.674 -> 0.742 ms per C3 frame, profiles/r06/ab_dropin_cold.jsonl)
  P.tile_cost = nullptr;
  P.pair_rows = 1;
  enqueue_frame(s, P, 1, nullptr, x->stream, true);
  counted.stop();
}

// rt_render into pageable memory (the drop-in seam): the frame as `chunks`
// bands of tile rows, one launch each on the context's stream; each band goes to the caller's
// buffer on the copy stream as soon as its launch is done, while the next bands render.
void render_banded(const HostFrame& f, RenderCtx* x, int chunks, CallCounters& counted) {
  rt_scene* s = f.s;
  Replica& r = *s->rep[0];
  const rt_camera& c = f.camera();
  const TilePlan tp = plan(c, f.row0, f.row_stride);
  const int tiles_y = tp.tiles_total / tp.tiles_x;
  auto band = [&](int k) { return (int)((long long)tiles_y * k / chunks); };  // its first tile row
  x->d_out.reserve((size_t)c.width * c.height * 3, "alloc frame");
  x->copy_stream.create("copy stream");
  for (int k = 0; k < chunks; k++) {
    RenderParams P = make_params(s, r, f.cam, f.row0, f.row_stride, band(k) * tp.tiles_x, 1, 0,
                                 x->d_out.p, x->d_cnt.p);
    P.num_sel_tiles = (band(k + 1) - band(k)) * tp.tiles_x;
    x->work.bind(s, c, P);
    P.tile_cost = nullptr;  // no dispatch order for a next frame (nothing reuses it here)
    enqueue_frame(s, P, 1, nullptr, x->stream, true);
    x->ev_chunk[k].create(hipEventDisableTiming);
    hip_check(hipEventRecord(x->ev_chunk[k], x->stream), "event record");
  }
  counted.stop();
  // no copy into the caller's buffer is pending when a failure below leaves this call
  struct Drain {
    hipStream_t st;
    bool armed = true;
    ~Drain() {
      if (armed) (void)hipStreamSynchronize(st);
    }
  } drain{x->copy_stream};
  for (int k = 0; k < chunks; k++) {
    hip_check(hipStreamWaitEvent(x->copy_stream, x->ev_chunk[k], 0), "wait band");
    copy_rows(f, x->d_out.p, kTile * band(k), std::min(tp.rows, kTile * band(k + 1)), x->copy_stream);
  }
  drain.armed = false;
  hip_check(hipStreamSynchronize(x->copy_stream), "synchronize copies");
}

// Every other rt_render (MSAA cameras, multi-device scenes, frames of one tile row): the frame
// into a device buffer, then its rows to the caller's.
void render_then_copy(const HostFrame& f, const CtxList& cx, CallCounters& counted) {
  rt_scene* s = f.s;
  const rt_camera& c = f.camera();
  RenderCtx* x = cx[0];
  // (a multi-device frame's d_out holds the first device's tile slot)
  DevBuf<float>& frame = s->multi ? x->d_image : x->d_out;
  frame.reserve((size_t)c.width * c.height * 3, "alloc frame");
  if (s->multi && c.num_samples > 1) {
    render_multi_msaa(s, cx, f.cam, frame.p, x->stream, true);
  } else if (s->multi) {
    render_multi(s, cx, f.cam, f.row0, f.row_stride, frame.p, x->stream, true);
  } else {
    Replica& r = *s->rep[0];
    RenderParams P = make_params(s, r, f.cam, f.row0, f.row_stride, 0, 1, 0, frame.p, x->d_cnt.p);
    x->work.bind(s, c, P);
    enqueue_frame(s, P, c.num_samples, x->work.samples.p, x->stream, true);
  }
  counted.stop();
  copy_rows(f, frame.p, 0, plan(c, f.row0, f.row_stride).rows, x->stream);
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return CENG795_RT_ABI_VERSION; }
const char* rt_last_error(void) { return g_error.c_str(); }

int rt_camera_from_view(const float position[3], const float gaze[3], const float up[3],
                        const float near_plane[4], float near_distance, int width, int height,
                        int num_samples, rt_camera* out) {
  if (!position || !gaze || !up || !near_plane || !out || width <= 0 || height <= 0)
    return set_error(RT_E_INVALID, "rt_camera_from_view: bad argument");
  camera_from_view(position, gaze, up, near_plane, near_distance, width, height,
                   num_samples < 1 ? 1 : num_samples, *out);
  return RT_OK;
}

// (its messages name rt_scene_create)
int rt_scene_create_multi(const rt_scene_desc* desc, int device_count, const int* devices,
                          rt_scene** out) {
  return create_from_desc("rt_scene_create", on_devices(device_count, devices), out, desc);
}

int rt_scene_create(const rt_scene_desc* desc, int device, rt_scene** out) {
  return create_from_desc("rt_scene_create", on_device(device), out, desc);
}

int rt_scene_load_xml(const char* xml_path, int device, rt_scene** out) {
  return create_from_file("rt_scene_load_xml", on_device(device), out, xml_path, {});
}

int rt_scene_load_xml_multi(const char* xml_path, int device_count, const int* devices,
                            rt_scene** out) {
  return create_from_file("rt_scene_load_xml_multi", on_devices(device_count, devices), out,
                          xml_path, {});
}

int rt_surface_version(void) { return 1; }

int rt_scene_create_surface(const rt_scene_desc* desc, const rt_surface_desc* surface, int device,
                            rt_scene** out) {
  return create_from_desc("rt_scene_create_surface", on_device(device), out, desc, surface);
}

int rt_scene_load_xml_surface(const char* xml_path, int device, rt_scene** out) {
  SceneFileOptions opt;
  opt.shading_mode = true;
  return create_from_file("rt_scene_load_xml_surface", on_device(device), out, xml_path, opt);
}

int rt_scene_has_smooth(const rt_scene* s) { return s && s->smooth ? 1 : 0; }

int rt_textures_version(void) { return 1; }

int rt_scene_create_textured(const rt_scene_desc* desc, const rt_surface_desc* surface,
                             const rt_texture_desc* textures, int device, rt_scene** out) {
  return create_from_desc("rt_scene_create_textured", on_device(device), out, desc, surface,
                          textures);
}

int rt_scene_load_xml_textured(const char* xml_path, const rt_texture_image* images, int num_images,
                               int device, rt_scene** out) {
  SceneFileOptions opt;
  opt.textures = true;
  opt.images = images;
  opt.num_images = num_images;
  return create_from_file("rt_scene_load_xml_textured", on_device(device), out, xml_path, opt);
}

int rt_host_textures_xml(const char* xml_path, char* names, int* modes3, float* normalizer,
                         int texture_capacity, int* mesh_texture, int* triangle_texture,
                         int* sphere_texture, int object_capacity, float* uv2, int uv_capacity,
                         int* counts5) {
  if (!xml_path || texture_capacity < 0 || object_capacity < 0 || uv_capacity < 0)
    return set_error(RT_E_INVALID, "rt_host_textures_xml: bad argument");
  return guarded([&] {
    XmlTextures xt;
    load_textures_xml(xml_path, xt);
    const int nt = (int)xt.image_name.size();
    for (int k = 0; k < std::min(nt, texture_capacity); k++) {
      if (names) std::snprintf(names + 256 * (size_t)k, 256, "%s", xt.image_name[(size_t)k].c_str());
      if (modes3) {
        modes3[3 * k] = xt.interpolation[(size_t)k];
        modes3[3 * k + 1] = xt.decal[(size_t)k];
        modes3[3 * k + 2] = xt.appearance[(size_t)k];
      }
      if (normalizer) normalizer[k] = xt.normalizer[(size_t)k];
    }
    auto ids = [&](const std::vector<int>& from, int* to) {
      if (to) std::copy(from.begin(), from.begin() + std::min((long)from.size(), (long)object_capacity), to);
    };
    ids(xt.mesh_texture, mesh_texture);
    ids(xt.triangle_texture, triangle_texture);
    ids(xt.sphere_texture, sphere_texture);
    const long pairs = (long)(xt.uv.size() / 2);
    if (uv2) std::copy(xt.uv.begin(), xt.uv.begin() + 2 * std::min(pairs, (long)uv_capacity), uv2);
    if (counts5) {
      counts5[0] = nt;
      counts5[1] = (int)xt.mesh_texture.size();
      counts5[2] = (int)xt.triangle_texture.size();
      counts5[3] = (int)xt.sphere_texture.size();
      counts5[4] = (int)pairs;
    }
    return RT_OK;
  });
}

int rt_scene_num_textures(const rt_scene* s) { return s ? (int)s->host.textures.size() : 0; }

// rt_texture_lookup*' argument rules (those of the other query entries); they need no GPU.
static void check_tex_lookup_args(const char* fn, const rt_scene* s, const void* q, long long n,
                                  const void* rgb) {
  const std::string f(fn);
  if (n < 0) throw std::invalid_argument(f + ": n < 0");
  if (n > 0 && (!q || !rgb)) throw std::invalid_argument(f + ": NULL pointer");
  if ((uintptr_t)q % 16 != 0) throw std::invalid_argument(f + ": q must be 16-byte aligned");
  if (!s) throw std::invalid_argument(f + ": scene is NULL");
  if (s->multi) throw std::domain_error(f + ": multi-device scenes are not supported");
}

int rt_texture_lookup_device(rt_scene* s, const rt_tex_query* d_q, long long n, float* d_rgb,
                             void* stream) {
  return guarded([&] {
    check_tex_lookup_args("rt_texture_lookup_device", s, d_q, n, d_rgb);
    if (n == 0) return RT_OK;
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    hip_check(launch_texture_lookup(r.tex, TexLookupParams{d_q, d_rgb, n}, (hipStream_t)stream),
              "texture lookup launch");
    return RT_OK;
  });
}

int rt_texture_lookup(rt_scene* s, const rt_tex_query* q, long long n, float* rgb) {
  return guarded([&] {
    check_tex_lookup_args("rt_texture_lookup", s, q, n, rgb);
    if (n == 0) return RT_OK;
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    CtxLease lease(s, 1);
    RenderCtx* x = lease.x[0];
    // the 16-B queries in the ray buffer (32-B records), the 12-B results in the position buffer
    x->d_rays.reserve(((size_t)n + 1) / 2, "alloc texture queries");
    x->d_xy.reserve(3 * (size_t)n, "alloc texture colours");
    hip_check(hipMemcpyAsync(x->d_rays.p, q, (size_t)n * sizeof(rt_tex_query),
                             hipMemcpyHostToDevice, x->stream), "upload texture queries");
    hip_check(launch_texture_lookup(r.tex, TexLookupParams{x->d_rays.p, x->d_xy.p, n}, x->stream),
              "texture lookup launch");
    hip_check(hipMemcpyAsync(rgb, x->d_xy.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost,
                             x->stream), "download texture colours");
    hip_check(hipStreamSynchronize(x->stream), "synchronize texture lookup");
    return RT_OK;
  });
}

int rt_host_texture_lookup_desc(const rt_texture_desc* textures, const rt_tex_query* q, long long n,
                                float* rgb) {
  return guarded([&] {
    if (!textures) throw std::invalid_argument("rt_host_texture_lookup_desc: textures == NULL");
    if (n < 0) throw std::invalid_argument("rt_host_texture_lookup_desc: n < 0");
    if (n > 0 && (!q || !rgb)) throw std::invalid_argument("rt_host_texture_lookup_desc: NULL pointer");
    std::vector<DevTexture> table;
    std::vector<uint32_t> texels;
    pack_textures(*textures, table, texels);
    host_texture_lookup(table, texels, q, n, rgb);
    return RT_OK;
  });
}

int rt_instances_version(void) { return 1; }

int rt_scene_num_instances(const rt_scene* s) {
  return s && s->inst ? (int)s->inst->instances.size() : 0;
}

int rt_scene_create_instanced(const rt_scene_desc* desc, const rt_instance_desc* instances,
                              int device, rt_scene** out) {
  return create_from_desc("rt_scene_create_instanced", on_device(device), out, desc, nullptr,
                          nullptr, instances);
}

int rt_scene_load_xml_instanced(const char* xml_path, int device, rt_scene** out) {
  SceneFileOptions opt;
  opt.instances = true;
  return create_from_file("rt_scene_load_xml_instanced", on_device(device), out, xml_path, opt);
}

int rt_host_instances_xml(const char* xml_path, int* mesh, int* material, float* transform16,
                          int capacity) {
  if (!xml_path || capacity < 0)
    return set_error(RT_E_INVALID, "rt_host_instances_xml: bad argument");
  return guarded([&] {
    XmlSceneStorage st;
    XmlInstances xi;
    rt_scene_desc d;
    load_instances_xml(xml_path, st, d, xi);
    const int n = (int)xi.mesh.size(), k = std::min(n, capacity);
    for (int i = 0; i < k; i++) {
      if (mesh) mesh[i] = xi.mesh[i];
      if (material) material[i] = xi.material[i];
    }
    if (transform16) std::memcpy(transform16, xi.transform.data(), 16 * (size_t)k * sizeof(float));
    return n;
  });
}

int rt_host_check_accel_instanced_desc(const rt_scene_desc* desc,
                                       const rt_instance_desc* instances, int treelet_leaves,
                                       long long* stats4) {
  if (!desc || !instances)
    return set_error(RT_E_INVALID, "rt_host_check_accel_instanced_desc: NULL argument");
  return guarded([&] {
    check_instance_desc("rt_host_check_accel_instanced_desc", instances);
    InstHost ih;
    build_instanced(*desc, *instances, treelet_leaves, ih);
    if (stats4) std::memcpy(stats4, ih.accel_stats.data(), ih.accel_stats.size() * sizeof(long long));
    return (int)ih.meshes.size();
  });
}

int rt_host_instance_info_desc(const rt_scene_desc* desc, const rt_instance_desc* instances,
                               float* inverse16, float* box6, int* top_dfs) {
  if (!desc || !instances)
    return set_error(RT_E_INVALID, "rt_host_instance_info_desc: NULL argument");
  return guarded([&] {
    check_instance_desc("rt_host_instance_info_desc", instances);
    InstHost ih;
    build_instanced(*desc, *instances, kDefaultTreeletLeaves, ih);
    const size_t n = ih.instances.size();
    if (inverse16) std::memcpy(inverse16, ih.inverse.data(), 16 * n * sizeof(float));
    for (size_t i = 0; i < n; i++) {
      if (box6) std::memcpy(box6 + 6 * i, ih.instances[i].box, 6 * sizeof(float));
      if (top_dfs) top_dfs[i] = ih.inst_top_dfs[i];
    }
    return RT_OK;
  });
}

// ---- scenes with motion
int rt_motion_version(void) { return 1; }

int rt_scene_has_motion(const rt_scene* s) { return s && s->inst && s->inst->has_motion ? 1 : 0; }

int rt_scene_create_moving(const rt_scene_desc* desc, const rt_instance_desc* instances,
                           const rt_motion_desc* motion, int device, rt_scene** out) {
  return create_from_desc("rt_scene_create_moving", on_device(device), out, desc, nullptr, nullptr,
                          instances, motion);
}

int rt_scene_load_xml_moving(const char* xml_path, int device, rt_scene** out) {
  SceneFileOptions opt;
  opt.instances = opt.motion = true;
  return create_from_file("rt_scene_load_xml_moving", on_device(device), out, xml_path, opt);
}

int rt_host_motion_xml(const char* xml_path, float* instance_velocity3, float* sphere_transform16,
                       float* sphere_velocity3, int capacity, int* counts2) {
  if (!xml_path || capacity < 0) return set_error(RT_E_INVALID, "rt_host_motion_xml: bad argument");
  return guarded([&] {
    XmlSceneStorage st;
    XmlInstances xi;
    rt_scene_desc d;
    load_instances_xml(xml_path, st, d, xi, true);
    const size_t ni = std::min(xi.mesh.size(), (size_t)capacity);
    const size_t ns = std::min((size_t)d.num_spheres, (size_t)capacity);
    if (instance_velocity3 && ni)
      std::memcpy(instance_velocity3, xi.velocity.data(), 3 * ni * sizeof(float));
    if (sphere_transform16 && ns)
      std::memcpy(sphere_transform16, xi.sphere_transform.data(), 16 * ns * sizeof(float));
    if (sphere_velocity3 && ns)
      std::memcpy(sphere_velocity3, xi.sphere_velocity.data(), 3 * ns * sizeof(float));
    if (counts2) {
      counts2[0] = (int)xi.mesh.size();
      counts2[1] = d.num_spheres;
    }
    return RT_OK;
  });
}

int rt_host_motion_info_desc(const rt_scene_desc* desc, const rt_instance_desc* instances,
                             const rt_motion_desc* motion, float* inst_box6,
                             float* sphere_inverse16, float* sphere_box6, int* top_dfs) {
  if (!desc) return set_error(RT_E_INVALID, "rt_host_motion_info_desc: NULL argument");
  return guarded([&] {
    check_instance_desc("rt_host_motion_info_desc", instances);
    InstHost ih;
    build_moving(*desc, instances, motion, kDefaultTreeletLeaves, ih);
    for (size_t i = 0; inst_box6 && i < ih.instances.size(); i++)
      std::memcpy(inst_box6 + 6 * i, ih.instances[i].box, 6 * sizeof(float));
    if (sphere_inverse16 && !ih.sphere_inverse.empty())
      std::memcpy(sphere_inverse16, ih.sphere_inverse.data(),
                  ih.sphere_inverse.size() * sizeof(float));
    if (sphere_box6 && !ih.sphere_box.empty())
      std::memcpy(sphere_box6, ih.sphere_box.data(), ih.sphere_box.size() * sizeof(float));
    if (top_dfs && !ih.object_top_dfs.empty())
      std::memcpy(top_dfs, ih.object_top_dfs.data(), ih.object_top_dfs.size() * sizeof(int));
    return RT_OK;
  });
}

int rt_debug_motion_inverse(rt_scene* s, int top_object, const float* times, long long n,
                            float* out12) {
  return guarded([&] {
    if (!s || n < 0 || (n > 0 && (!times || !out12)))
      throw std::invalid_argument("rt_debug_motion_inverse: bad argument");
    if (!rt_scene_has_motion(s))
      throw std::invalid_argument("rt_debug_motion_inverse: not a scene with motion");
    const InstHost& ih = *s->inst;
    if (top_object < 0 || (size_t)top_object >= ih.object_top_dfs.size())
      throw std::invalid_argument("rt_debug_motion_inverse: top_object out of range");
    Replica& r = *s->rep[0];
    const DevPrim& p = ih.top_prims[(size_t)ih.object_top_dfs[(size_t)top_object]];
    const float *fwd = nullptr, *vel = nullptr;
    if (p.kind == kPrimInstance && ih.instances[(size_t)p.material].moving) {
      fwd = r.d_motion_instances.p[p.material].fwd;  // (device addresses: not read here)
      vel = r.d_motion_instances.p[p.material].vel;
    } else if (p.kind == kPrimMovingSphere && ih.motion_spheres[(size_t)p.material].moving) {
      fwd = r.d_motion_spheres.p[p.material].fwd;
      vel = r.d_motion_spheres.p[p.material].vel;
    } else {
      throw std::invalid_argument("rt_debug_motion_inverse: the object does not move");
    }
    if (n == 0) return RT_OK;
    DeviceGuard g(r.device);
    DevBuf<float> d_times, d_out;
    d_times.reserve((size_t)n, "alloc times");
    d_out.reserve(12 * (size_t)n, "alloc inverses");
    hip_check(hipMemcpy(d_times.p, times, (size_t)n * sizeof(float), hipMemcpyHostToDevice),
              "upload times");
    hip_check(launch_motion_inverse(fwd, vel, d_times.p, n, d_out.p, nullptr), "inverse launch");
    hip_check(hipMemcpy(out12, d_out.p, 12 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost),
              "download inverses");
    return RT_OK;
  });
}

int rt_host_vertex_normals_desc(const rt_scene_desc* desc, float* out3n) {
  if (!desc || (!out3n && desc->num_vertices > 0))
    return set_error(RT_E_INVALID, "rt_host_vertex_normals_desc: NULL argument");
  return guarded([&] {
    host_vertex_normals(*desc, out3n);
    return RT_OK;
  });
}

int rt_host_mesh_smooth_xml(const char* xml_path, unsigned char* out, int capacity) {
  if (!xml_path || capacity < 0 || (!out && capacity > 0))
    return set_error(RT_E_INVALID, "rt_host_mesh_smooth_xml: bad argument");
  return guarded([&] {
    XmlSceneStorage st;
    rt_scene_desc d;
    load_scene_xml(xml_path, st, d);
    const int n = (int)st.mesh_smooth.size();
    for (int m = 0; m < std::min(n, capacity); m++) out[m] = st.mesh_smooth[m];
    return n;
  });
}

// rt_hit_attributes*' argument rules (rt_trace_rays*'); they need no GPU.
static void check_attr_args(const char* fn, const rt_scene* s, const void* rays, const void* hits,
                            long long n, const void* attr) {
  const std::string f(fn);
  if (n < 0) throw std::invalid_argument(f + ": n < 0");
  if (n > 0 && (!rays || !hits || !attr)) throw std::invalid_argument(f + ": NULL pointer");
  if ((uintptr_t)rays % 16 != 0 || (uintptr_t)hits % 16 != 0 || (uintptr_t)attr % 16 != 0)
    throw std::invalid_argument(f + ": rays, hits and attr must be 16-byte aligned");
  if (!s) throw std::invalid_argument(f + ": scene is NULL");
  if (s->multi)
    throw std::domain_error(f + ": hit attributes on multi-device scenes are not supported");
  if (s->inst) throw std::domain_error(f + ": hit attributes on instanced scenes are not supported");
}

int rt_hit_attributes_device(rt_scene* s, const rt_ray* d_rays, const rt_ray_hit* d_hits,
                             long long n, rt_hit_attr* d_attr, void* stream) {
  return guarded([&] {
    check_attr_args("rt_hit_attributes_device", s, d_rays, d_hits, n, d_attr);
    if (n == 0) return RT_OK;
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    hip_check(launch_hit_attributes(scene_params(s, r), r.surf, AttrParams{d_rays, d_hits, d_attr, n},
                                    (hipStream_t)stream), "hit attributes launch");
    return RT_OK;
  });
}

int rt_hit_attributes(rt_scene* s, const rt_ray* rays, const rt_ray_hit* hits, long long n,
                      rt_hit_attr* attr) {
  return guarded([&] {
    check_attr_args("rt_hit_attributes", s, rays, hits, n, attr);
    if (n == 0) return RT_OK;
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    CtxLease lease(s, 1);
    RenderCtx* x = lease.x[0];
    // rays, then (in one buffer of 32-B records) the hits followed by the 48-B results
    const size_t attr_recs = ((size_t)n * sizeof(rt_hit_attr) + sizeof(rt_ray_hit) - 1) / sizeof(rt_ray_hit);
    x->d_rays.reserve((size_t)n, "alloc rays");
    x->d_ray_out.reserve((size_t)n + attr_recs, "alloc hits and attributes");
    rt_hit_attr* d_attr = reinterpret_cast<rt_hit_attr*>(x->d_ray_out.p + n);
    hip_check(hipMemcpyAsync(x->d_rays.p, rays, (size_t)n * sizeof(rt_ray), hipMemcpyHostToDevice,
                             x->stream), "upload rays");
    hip_check(hipMemcpyAsync(x->d_ray_out.p, hits, (size_t)n * sizeof(rt_ray_hit),
                             hipMemcpyHostToDevice, x->stream), "upload hits");
    hip_check(launch_hit_attributes(scene_params(s, r), r.surf,
                                    AttrParams{x->d_rays.p, x->d_ray_out.p, d_attr, n}, x->stream),
              "hit attributes launch");
    hip_check(hipMemcpyAsync(attr, d_attr, (size_t)n * sizeof(rt_hit_attr), hipMemcpyDeviceToHost,
                             x->stream), "download attributes");
    hip_check(hipStreamSynchronize(x->stream), "synchronize hit attributes");
    return RT_OK;
  });
}

void rt_scene_destroy(rt_scene* s) {
  delete s;
}

int rt_scene_num_cameras(const rt_scene* s) { return s ? (int)s->host.cameras.size() : 0; }
int rt_scene_num_lights(const rt_scene* s) { return s ? (int)s->host.lights.size() : 0; }
int rt_scene_bvh_depth(const rt_scene* s) { return s ? s->host.depth : 0; }
int rt_scene_device_count(const rt_scene* s) { return s ? (int)s->rep.size() : 0; }

int rt_scene_camera(const rt_scene* s, int cam, rt_camera* out) {
  if (!s || !out || cam < 0 || cam >= (int)s->host.cameras.size())
    return set_error(RT_E_INVALID, "rt_scene_camera: bad argument");
  *out = s->host.cameras[cam];
  return RT_OK;
}

const char* rt_scene_image_name(const rt_scene* s, int cam) {
  if (!s || cam < 0 || cam >= (int)s->host.image_names.size()) return "";
  return s->host.image_names[cam].c_str();
}

int rt_scene_dump_bvh(const rt_scene* s, const char* path) {
  if (!s || !path) return set_error(RT_E_INVALID, "rt_scene_dump_bvh: NULL argument");
  if (s->inst)
    return set_error(RT_E_UNSUPPORTED, "rt_scene_dump_bvh: not for instanced scenes");
  if (!write_text_file(path, dump_bvh(s->host)))
    return set_error(RT_E_IO, std::string("cannot open ") + path);
  return RT_OK;
}

// The host dump entries' file (inside `guarded`).
static void write_dump(const HostScene& h, const char* out_path) {
  if (!write_text_file(out_path, dump_bvh(h)))
    throw std::ios_base::failure(std::string("cannot open ") + out_path);
}

int rt_host_dump_bvh_xml(const char* xml_path, const char* out_path) {
  if (!xml_path || !out_path) return set_error(RT_E_INVALID, "rt_host_dump_bvh_xml: NULL argument");
  return guarded([&] {
    HostScene h;
    load_flat_scene(xml_path, h);
    write_dump(h, out_path);
    return RT_OK;
  });
}

int rt_host_dump_bvh_desc(const rt_scene_desc* desc, const char* out_path) {
  if (!desc || !out_path) return set_error(RT_E_INVALID, "rt_host_dump_bvh_desc: NULL argument");
  return guarded([&] {
    HostScene h;
    build_host_scene(*desc, h);
    write_dump(h, out_path);
    return RT_OK;
  });
}

void* rt_host_alloc(size_t bytes) {
  void* p = nullptr;
  const int rc = guarded([&] {
    hip_check(hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault),
              "rt_host_alloc");
    return RT_OK;
  });
  return rc == RT_OK ? p : nullptr;
}

void rt_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int rt_host_check_accel_xml(const char* xml_path, int treelet_leaves, long long* stats4) {
  if (!xml_path || !stats4) return set_error(RT_E_INVALID, "rt_host_check_accel_xml: NULL argument");
  return guarded([&] {
    HostScene h;
    flat_host_scene(xml_path, treelet_leaves, 0, stats4, h);
    return RT_OK;
  });
}

int rt_host_accel_slot_hist_xml(const char* xml_path, int treelet_leaves, long long* hist9) {
  if (!xml_path || !hist9)
    return set_error(RT_E_INVALID, "rt_host_accel_slot_hist_xml: NULL argument");
  return guarded([&] {
    HostScene h;
    long long stats[4];
    flat_host_scene(xml_path, treelet_leaves, 0, stats, h);
    accel_slot_histogram(h, hist9);
    return RT_OK;
  });
}

int rt_host_accel_kind_hist_xml(const char* xml_path, int treelet_leaves, long long* hist81) {
  if (!xml_path || !hist81)
    return set_error(RT_E_INVALID, "rt_host_accel_kind_hist_xml: NULL argument");
  return guarded([&] {
    HostScene h;
    long long stats[4];
    flat_host_scene(xml_path, treelet_leaves, 0, stats, h);
    accel_kind_histogram(h, hist81);
    return RT_OK;
  });
}

int rt_host_check_wide_node(const void* node, unsigned long long bytes) {
  if (!node || bytes != sizeof(DevNode8))
    return set_error(RT_E_INVALID, "rt_host_check_wide_node: NULL node or not 128 bytes");
  return guarded([&] {
    DevNode8 W;
    std::memcpy(&W, node, sizeof W);
    const std::string err = wide_slot_order_error(W);
    if (!err.empty()) throw std::invalid_argument("wide node: " + err);
    return RT_OK;
  });
}

int rt_host_accel_slots_check(long long ref_slots, long long wide_slots) {
  if (ref_slots < 0 || wide_slots < 0)
    return set_error(RT_E_INVALID, "rt_host_accel_slots_check: bad argument");
  const std::string err = accel_slots_error((size_t)ref_slots, (size_t)wide_slots);
  return err.empty() ? RT_OK : set_error(RT_E_UNSUPPORTED, err);
}

int rt_host_packet_div(int divisor, int first, int count, int* quot) {
  if (divisor < 1 || first < 0 || count < 0 || (long long)first + count > (1ll << 31) || !quot)
    return set_error(RT_E_INVALID, "rt_host_packet_div: bad argument");
  const DivMagic m = div_magic(divisor);
  for (int i = 0; i < count; i++) quot[i] = div_by((int)((long long)first + i), m);
  return RT_OK;
}

int rt_host_packet_coords(int tiles_x, int num_sel_tiles, int tile_begin, int tile_step,
                          int block_deal, int order_regions, int order_stride, int count,
                          int* out4) {
  if (tiles_x < 1 || num_sel_tiles < 0 || tile_begin < 0 || tile_step < 1 || order_regions < 1 ||
      order_stride < 0 || count < 0 || !out4)
    return set_error(RT_E_INVALID, "rt_host_packet_coords: bad argument");
  RenderParams P;
  std::memset(&P, 0, sizeof P);
  P.tiles_x = tiles_x;
  P.num_sel_tiles = num_sel_tiles;
  P.tile_begin = tile_begin;
  P.tile_step = tile_step;
  P.block_deal = block_deal ? 1 : 0;
  P.order_regions = order_regions;
  P.order_stride = order_stride;
  P.tile_block = whole_tile_rows(P);
  const PacketGeom G = packet_geom(P);
  for (int p = 0; p < count; p++) {
    // (a wave's tile as dispatch_sel takes it: logical packet p of a launch in block order)
    int sel = p < G.packets ? packet_sel(P, G, p) : -1;
    if (sel >= P.num_sel_tiles) sel = -1;
    int tx = -1, ty = -1;
    if (sel >= 0) sel_tile(P, G, sel, tx, ty);
    out4[4 * p] = sel;
    out4[4 * p + 1] = tx;
    out4[4 * p + 2] = ty;
    out4[4 * p + 3] = order_slot(P, G, p);
  }
  return G.packets;
}

int rt_host_visit_time_exp(const float* box6, const float* cam3) {
  if (!box6 || !cam3) {
    set_error(RT_E_INVALID, "rt_host_visit_time_exp: NULL argument");
    return INT_MIN;
  }
  return visit_time_exp(box6, cam3);
}

int rt_test_visit_time_exp(int on, int rel) {
  if (rel < -200 || rel > 200) return set_error(RT_E_INVALID, "rt_test_visit_time_exp: bad argument");
  set_test_visit_time_exp(on ? 1 : 0, rel);
  return RT_OK;
}

int rt_test_entry_cuts(int mode) {
  if (mode != 0 && mode != 1) return set_error(RT_E_INVALID, "rt_test_entry_cuts: bad argument");
  g_test_entry_cuts.store(mode);
  return RT_OK;
}

// The scene file's host scene with its culling tree as creation builds it, and whether it gets
// entry cuts (as seed_entry_cuts decides it).
static bool entry_cut_scene(const char* xml_path, int treelet_leaves, int cam, HostScene& h) {
  flat_host_scene(xml_path, treelet_leaves, max_supported_depth(), nullptr, h);
  if (cam < 0 || cam >= (int)h.cameras.size())
    throw std::invalid_argument("camera index out of range");
  return scene_entry_cuts_apply(h, max_supported_depth());
}

int rt_host_entry_cuts_xml(const char* xml_path, int treelet_leaves, int cam, int* out,
                           long long capacity, long long* stats24) {
  if (!xml_path) return set_error(RT_E_INVALID, "rt_host_entry_cuts_xml: NULL argument");
  return guarded([&] {
    HostScene h;
    if (stats24) std::fill(stats24, stats24 + kEntryCutStats, 0ll);
    if (!entry_cut_scene(xml_path, treelet_leaves, cam, h)) return 0;
    const std::vector<int> table = build_entry_cuts(h, h.cameras[cam], stats24);
    if (out && capacity >= (long long)table.size())
      std::memcpy(out, table.data(), table.size() * sizeof(int));
    return (int)table.size();
  });
}

int rt_host_check_entry_cuts_xml(const char* xml_path, int treelet_leaves, int cam,
                                 long long* violations, long long* first4) {
  if (!xml_path || !violations)
    return set_error(RT_E_INVALID, "rt_host_check_entry_cuts_xml: NULL argument");
  return guarded([&] {
    HostScene h;
    *violations = 0;
    if (!entry_cut_scene(xml_path, treelet_leaves, cam, h)) return 0;
    const std::vector<int> table = build_entry_cuts(h, h.cameras[cam], nullptr);
    *violations = check_entry_cuts(h, h.cameras[cam], table, first4);
    if (*violations < 0) throw std::runtime_error("entry cuts: the table does not fit the camera");
    return (int)table.size();
  });
}

int rt_set_traversal(rt_scene* s, int mode) {
  if (!s || (mode != RT_TRAVERSAL_FAST && mode != RT_TRAVERSAL_REFERENCE))
    return set_error(RT_E_INVALID, "rt_set_traversal: bad argument");
  s->mode = mode;
  return RT_OK;
}

int rt_set_msaa_seed(rt_scene* s, unsigned long long seed) {
  if (!s) return set_error(RT_E_INVALID, "rt_set_msaa_seed: NULL scene");
  s->msaa_seed = seed;
  return RT_OK;
}

int rt_num_tiles(const rt_scene* s, int cam, int row0, int row_stride) {
  if (!s || cam < 0 || cam >= (int)s->host.cameras.size() || row0 < 0 || row_stride < 1)
    return set_error(RT_E_INVALID, "rt_num_tiles: bad argument");
  return plan(s->host.cameras[cam], row0, row_stride).tiles_total;
}

int rt_render_device(rt_scene* s, int cam, int row0, int row_stride, int tile_begin,
                     int tile_step, int tile_major, float* d_out, void* stream) {
  return rt_render_device_range(s, cam, row0, row_stride, tile_begin, tile_step, -1, tile_major,
                                d_out, stream);
}

int rt_render_device_range(rt_scene* s, int cam, int row0, int row_stride, int tile_begin,
                           int tile_step, int tile_count, int tile_major, float* d_out,
                           void* stream) {
  return guarded([&] {
    check_render_args(s, cam, row0, row_stride);
    if (tile_begin < 0 || tile_step < 1 || !d_out ||
        (tile_major & ~(RT_TILE_MAJOR | RT_TILE_BLOCKS | RT_TILE_RECORDS)))
      throw std::invalid_argument("rt_render_device: bad tile selection / output");
    if ((tile_major & RT_TILE_RECORDS) && !records_ok(s, cam))
      throw std::domain_error("rt_render_device: pixel records need a pixel-centre camera, no "
                              "mirror/dielectric recursion and at most 4 lights");
    const rt_camera& c = s->host.cameras[cam];
    if (s->multi) {
      // a multi-device scene renders whole frames (rows subsets allowed) split over its devices
      if (tile_begin != 0 || tile_step != 1 || tile_major || tile_count >= 0)
        throw std::domain_error("multi-device scenes render whole row-major frames only");
      std::lock_guard<std::mutex> lk(s->multi_mu);
      // the caller stream's own contexts: consecutive frames on different caller streams run on
      // different device streams, and frames on one caller stream stay ordered
      CtxList cx;
      for (auto& r : s->rep) cx.push_back(stream_ctx_for(*r, stream));
      if (c.num_samples > 1)
        render_multi_msaa(s, cx, cam, d_out, (hipStream_t)stream, false);
      else
        render_multi(s, cx, cam, row0, row_stride, d_out, (hipStream_t)stream, false);
      return RT_OK;
    }
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    std::unique_lock<std::mutex> lk;
    StreamScratch* sc = scratch_for(s, r, stream, lk);
    RenderParams P = make_params(s, r, cam, row0, row_stride, tile_begin, tile_step, tile_major,
                                 d_out, r.d_counters.p);
    const int unit_tiles = P.block_deal ? 4 : 1;  // tile_count counts deal units
    const bool trimmed = tile_count >= 0 && (long long)tile_count * unit_tiles < P.num_sel_tiles;
    if (c.num_samples > 1 && (trimmed || tile_begin != 0 || tile_step != 1 || tile_major))
      throw std::domain_error("NumSamples > 1 renders whole row-major frames only");
    if (trimmed) P.num_sel_tiles = tile_count * unit_tiles;
    sc->work.bind(s, c, P);  // (the selection is final: the schedule's layout depends on it)
    // warm order: a frame of the same selection as the stream's previous one
    // dispatches its primary kernel heaviest-first by that frame's measured tile costs
    const std::array<long long, 7> key{cam, row0, row_stride, tile_begin, tile_step,
                                       P.num_sel_tiles, P.block_deal};
    const bool orderable = c.num_samples <= 1 && !P.frames && P.num_lights > 0;
    P.primary_order = orderable && sc->order_valid && sc->order_key == key ? 1 : 0;
    enqueue_frame(s, P, c.num_samples, sc->work.samples.p, (hipStream_t)stream, true);
    hip_check(hipEventRecord(sc->done, (hipStream_t)stream), "event record");
    sc->order_key = key;
    sc->order_valid = orderable;
    return RT_OK;
  });
}

int rt_untile_device(rt_scene* s, int cam, int row0, int row_stride, int devices, int slot,
                     int tile_offset, int flags, const float* d_gathered, float* d_out,
                     void* stream) {
  return guarded([&] {
    UntileParams U = checked_untile_params("rt_untile_device", false, s, cam, row0, row_stride,
                                           devices, slot, tile_offset, flags, d_gathered, d_out);
    DeviceGuard g(s->rep[0]->device);
    U.recv = d_gathered;
    U.out = d_out;
    U.vec = untile_vec(U);
    hip_check(launch_untile(U, (hipStream_t)stream), "untile launch");
    return RT_OK;
  });
}

int rt_tile_costs(rt_scene* s, void* stream, unsigned* host_out, int capacity) {
  if (!s || !host_out || capacity < 0) return set_error(RT_E_INVALID, "rt_tile_costs: bad argument");
  return guarded([&]() -> int {
    if (s->multi) throw std::domain_error("rt_tile_costs: single-device scenes only");
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    StreamScratch* x = nullptr;
    std::unique_lock<std::mutex> held;
    {
      std::lock_guard<std::mutex> lk(r.mu);
      for (auto& p : r.streams)
        if (p->stream == stream) x = p.get();
      if (x) held = std::unique_lock<std::mutex>(x->mu);
    }
    if (!x || !x->order_valid)
      throw std::domain_error("rt_tile_costs: no ordered frame was rendered on this stream");
    const long long n = x->order_key[5];  // the last selection's tiles
    if (n > capacity) throw std::invalid_argument("rt_tile_costs: capacity below the frame's tiles");
    hip_check(hipStreamSynchronize((hipStream_t)stream), "synchronize stream");
    hip_check(hipMemcpy(host_out, x->work.sched.p + sched_snap_offset((unsigned long long)n),
                        (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost),
              "read tile costs");
    return (int)n;
  });
}

int rt_scene_records_ok(const rt_scene* s, int cam) {
  if (!s || cam < 0 || cam >= (int)s->host.cameras.size())
    return set_error(RT_E_INVALID, "rt_scene_records_ok: bad argument");
  return records_ok(s, cam) ? 1 : 0;
}

int rt_resolve_device(rt_scene* s, int cam, int row0, int row_stride, int devices, int slot,
                      int tile_offset, int flags, const unsigned* d_gathered, float* d_out,
                      void* stream) {
  return guarded([&] {
    UntileParams U = checked_untile_params("rt_resolve_device", true, s, cam, row0, row_stride,
                                           devices, slot, tile_offset, flags, d_gathered, d_out);
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    const RenderParams P = make_params(s, r, cam, row0, row_stride, 0, 1, 0, d_out, nullptr);
    U.recv = reinterpret_cast<const float*>(d_gathered);
    U.out = d_out;
    hip_check(launch_resolve(P, U, s->has_spheres, (hipStream_t)stream), "resolve launch");
    return RT_OK;
  });
}

int rt_resolve_rows(rt_scene* s, int cam, int row_begin, int row_end, const unsigned* d_records,
                    float* d_out, void* stream) {
  return guarded([&] {
    check_render_args(s, cam, 0, 1);
    const rt_camera& c = s->host.cameras[cam];
    if (row_begin < 0 || row_end < row_begin || row_end > c.height || !d_records || !d_out)
      throw std::invalid_argument("rt_resolve_rows: bad argument");
    if (s->multi) throw std::domain_error("rt_resolve_rows: single-device scenes only");
    if (!records_ok(s, cam)) throw std::domain_error("rt_resolve_rows: no pixel records here");
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    const RenderParams P = make_params(s, r, cam, 0, 1, 0, 1, 0, d_out, nullptr);
    hip_check(launch_resolve_rows(P, d_records, row_begin, row_end, s->has_spheres,
                                  (hipStream_t)stream), "resolve launch");
    return RT_OK;
  });
}

int rt_ray_query_version(void) { return 1; }

int rt_trace_rays_device(rt_scene* s, const rt_ray* d_rays, long long n, rt_ray_hit* d_hits,
                         int flags, void* stream) {
  return query_device("rt_trace_rays_device", kClosestHit, s, d_rays, n, 0, d_hits, flags, stream);
}

int rt_occluded_device(rt_scene* s, const rt_ray* d_rays, long long n, unsigned char* d_occ,
                       int flags, void* stream) {
  return query_device("rt_occluded_device", kOcclusion, s, d_rays, n, 0, d_occ, flags, stream);
}

int rt_trace_rays(rt_scene* s, const rt_ray* rays, long long n, rt_ray_hit* hits, int flags) {
  return query_host("rt_trace_rays", kClosestHit, s, rays, n, 0, hits, flags, nullptr);
}

int rt_occluded(rt_scene* s, const rt_ray* rays, long long n, unsigned char* occ, int flags) {
  return query_host("rt_occluded", kOcclusion, s, rays, n, 0, occ, flags, nullptr);
}

int rt_radiance_query_version(void) { return 1; }

int rt_shade_rays_device(rt_scene* s, const rt_ray* d_rays, long long n, int depth,
                         rt_radiance* d_out, int flags, void* stream) {
  return query_device("rt_shade_rays_device", kRadiance, s, d_rays, n, depth, d_out, flags, stream);
}

int rt_shade_rays(rt_scene* s, const rt_ray* rays, long long n, int depth, rt_radiance* out,
                  int flags, rt_stats* stats) {
  return query_host("rt_shade_rays", kRadiance, s, rays, n, depth, out, flags, stats);
}

int rt_light_samples_version(void) { return 1; }

int rt_shade_rays_lit_device(rt_scene* s, const rt_ray* d_rays, long long n, int depth,
                             const rt_light_sample* d_lights, int k, rt_radiance* d_out, int flags,
                             void* stream) {
  const LightList lit{d_lights, k};
  return query_device("rt_shade_rays_lit_device", kRadianceLit, s, d_rays, n, depth, d_out, flags,
                      stream, &lit);
}

int rt_shade_rays_lit(rt_scene* s, const rt_ray* rays, long long n, int depth,
                      const rt_light_sample* lights, int k, rt_radiance* out, int flags,
                      rt_stats* stats) {
  const LightList lit{lights, k};
  return query_host("rt_shade_rays_lit", kRadianceLit, s, rays, n, depth, out, flags, stats, &lit);
}

int rt_set_radiance_scratch_limit(rt_scene* s, size_t bytes) {
  if (!s) return set_error(RT_E_INVALID, "rt_set_radiance_scratch_limit: NULL scene");
  // one wave of rays at the scene's maximum depth must fit (scenes that can recurse)
  if (bytes != 0 && s->needs_recursion &&
      bytes < (size_t)kRadianceChunkUnit * radiance_frame_bytes(s->host.max_depth))
    return set_error(RT_E_INVALID, "rt_set_radiance_scratch_limit: below one wave's ray-tree "
                                   "frames at the scene's MaxRecursionDepth");
  s->radiance_limit.store(bytes ? bytes : kRadianceDefaultLimit);
  return RT_OK;
}

long long rt_stream_frame_scratch_bytes(rt_scene* s, void* stream) {
  if (!s) return set_error(RT_E_INVALID, "rt_stream_frame_scratch_bytes: NULL scene");
  long long bytes = 0;
  for (auto& rp : s->rep) {
    std::lock_guard<std::mutex> lk(rp->mu);
    for (auto& x : rp->streams)
      if (x->stream == stream) bytes += (long long)(x->work.frames.cap * sizeof(float));
  }
  return bytes;
}

int rt_host_leaf_objects_desc(const rt_scene_desc* desc, int* out, int capacity) {
  if (!desc || capacity < 0 || (capacity > 0 && !out))
    return set_error(RT_E_INVALID, "rt_host_leaf_objects_desc: bad argument");
  return guarded([&] {
    HostScene h;
    build_host_scene(*desc, h);
    const int leaves = (int)h.leaf_object.size();
    std::copy_n(h.leaf_object.begin(), std::min(leaves, capacity), out);
    return leaves;
  });
}

int rt_release_stream_scratch(rt_scene* s, void* stream) {
  if (!s) return set_error(RT_E_INVALID, "rt_release_stream_scratch: NULL scene");
  return guarded([&] {
    for (auto& rp : s->rep) {
      Replica& r = *rp;
      std::unique_ptr<StreamScratch> x;
      RenderCtx* sc = nullptr;
      {
        std::lock_guard<std::mutex> lk(r.mu);
        for (size_t k = 0; k < r.streams.size(); k++)
          if (r.streams[k]->stream == stream) {
            x = std::move(r.streams[k]);
            r.streams.erase(r.streams.begin() + (long)k);
            break;
          }
        for (size_t k = 0; k < r.stream_ctx.size(); k++)
          if (r.stream_ctx[k].first == stream) {
            sc = r.stream_ctx[k].second;
            r.stream_ctx.erase(r.stream_ctx.begin() + (long)k);
            break;
          }
      }
      if (sc) {  // a multi-device scene's context of that caller stream: back to the pool
        DeviceGuard g(r.device);
        hip_check(hipStreamSynchronize(sc->stream), "synchronize context stream");
        release_ctx(r, sc);
      }
      if (!x) continue;
      DeviceGuard g(r.device);
      {
        std::lock_guard<std::mutex> lk(x->mu);  // no enqueue on it is in progress
        hip_check(hipStreamSynchronize((hipStream_t)stream), "synchronize stream");
      }
      x.reset();
    }
    return RT_OK;
  });
}

int rt_collect_stats(rt_scene* s, rt_stats* stats) {
  if (!s || !stats) return set_error(RT_E_INVALID, "rt_collect_stats: NULL argument");
  return guarded([&] {
    std::memset(stats, 0, sizeof *stats);
    for (auto& rp : s->rep) add_counters(take_counters(*rp), stats);
    return RT_OK;
  });
}

int rt_debug_counters(rt_scene* s, long long* out16) {
  if (!s || !out16) return set_error(RT_E_INVALID, "rt_debug_counters: NULL argument");
  return guarded([&] {
    for (int k = 0; k < kCounterWidth; k++) out16[k] = 0;
    for (auto& rp : s->rep) {
      const std::vector<unsigned long long> c = take_counters(*rp);
      for (int k = 0; k < kCounterWidth; k++) {
        unsigned long long sum = 0;
        for (int r = 0; r < kCounterRows; r++) sum += c[kCounterWidth * r + k];
        out16[k] += (long long)sum;
      }
    }
    out16[kCntExactBox] = (long long)read_reset_exact_fallbacks();
    return diag_build() ? 1 : 0;
  });
}

long long rt_debug_phases(unsigned long long* out, long long max_values) {
  if (!out || max_values < 0) return set_error(RT_E_INVALID, "rt_debug_phases: bad argument");
  const long long n = read_reset_phases(out, max_values);
  if (n < 0) return set_error(RT_E_INVALID, "rt_debug_phases: buffer too small or copy failed");
  return n;
}

long long rt_debug_timeline(unsigned long long* out, long long max_values) {
  if (!out || max_values < 0) return set_error(RT_E_INVALID, "rt_debug_timeline: bad argument");
  const long long n = read_reset_timeline(out, max_values);
  if (n < 0) return set_error(RT_E_INVALID, "rt_debug_timeline: buffer too small or copy failed");
  return n;
}

int rt_debug_frame_occupancy(int device, int* out4) {
  if (!out4) return set_error(RT_E_INVALID, "rt_debug_frame_occupancy: bad argument");
  return guarded([&] {
    DeviceGuard g(device);
    hip_check(frame_kernel_occupancy(out4), "occupancy query");
    return RT_OK;
  });
}

int rt_debug_quotient_check_mode(int device, int mode, unsigned long long seed, long long count,
                                 long long* out4) {
  if (!out4 || count < 0 || mode < 0 || mode > 1)
    return set_error(RT_E_INVALID, "rt_debug_quotient_check: bad argument");
  return guarded([&] {
    DeviceGuard g(device);
    DevBuf<unsigned long long> buf;
    buf.reserve(4, "alloc");
    unsigned long long* d = buf.p;
    hip_check(hipMemset(d, 0, 4 * sizeof *d), "clear");
    hip_check(launch_quot_check(mode, seed, count, d, nullptr), "quotient check launch");
    unsigned long long h[4];
    hip_check(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost), "read");
    for (int k = 0; k < 4; k++) out4[k] = (long long)h[k];
    return RT_OK;
  });
}

int rt_debug_quotient_check(int device, unsigned long long seed, long long count,
                            long long* out2) {
  if (!out2) return set_error(RT_E_INVALID, "rt_debug_quotient_check: bad argument");
  long long out4[4];
  const int rc = rt_debug_quotient_check_mode(device, 0, seed, count, out4);
  if (rc == RT_OK) {
    out2[0] = out4[0];
    out2[1] = out4[1];
  }
  return rc;
}

int rt_render(rt_scene* s, int cam, int row0, int row_stride, float* out_rgb, rt_stats* stats) {
  return guarded([&] {
    check_render_args(s, cam, row0, row_stride);
    if (!out_rgb) throw std::invalid_argument("rt_render: out_rgb is NULL");
    const rt_camera& c = s->host.cameras[cam];
    const TilePlan tp = plan(c, row0, row_stride);
    if (tp.rows == 0) return RT_OK;
    std::unique_lock<std::mutex> multi_lock(s->multi_mu, std::defer_lock);
    if (s->multi) multi_lock.lock();
    CtxLease lease(s, s->multi ? s->rep.size() : 1);
    DeviceGuard g(s->rep[0]->device);
    CallCounters counted(s, lease.x);
    const HostFrame f{s, cam, row0, row_stride, out_rgb};
    const bool one_pass = !s->multi && c.num_samples <= 1;  // one device, pixel-centre camera
    const int chunks = std::min(kRenderChunks, tp.tiles_total / tp.tiles_x);
    float* direct = one_pass ? pinned_device_pointer(out_rgb) : nullptr;
    if (direct)
      render_pinned(f, lease.x[0], direct, counted);
    else if (one_pass && chunks > 1)
      render_banded(f, lease.x[0], chunks, counted);
    else
      render_then_copy(f, lease.x, counted);
    counted.read(stats);
    return RT_OK;
  });
}

int rt_set_kernel_timing(rt_scene* s, int enable) {
  if (!s) return set_error(RT_E_INVALID, "rt_set_kernel_timing: NULL scene");
  std::lock_guard<std::mutex> lk(s->timing_mu);
  s->timing.on = enable != 0;
  return RT_OK;
}

int rt_read_kernel_times(rt_scene* s, double* ms4, long long* launches) {
  if (!s || !ms4) return set_error(RT_E_INVALID, "rt_read_kernel_times: NULL argument");
  return guarded([&] {
    DeviceGuard g(s->rep[0]->device);
    std::vector<std::array<hipEvent_t, 4>> done;
    double sum[4];
    long long n;
    {
      std::lock_guard<std::mutex> lk(s->timing_mu);
      done.swap(s->timing.pending);
      std::memcpy(sum, s->timing.sum, sizeof sum);
      n = s->timing.folded;
      std::memset(s->timing.sum, 0, sizeof s->timing.sum);
      s->timing.folded = 0;
    }
    for (auto& q : done) {
      hip_check(hipEventSynchronize(q[3]), "timing sync");
      float a = 0, b = 0, c = 0;
      hip_check(hipEventElapsedTime(&a, q[0], q[1]), "elapsed");
      hip_check(hipEventElapsedTime(&b, q[1], q[2]), "elapsed");
      hip_check(hipEventElapsedTime(&c, q[2], q[3]), "elapsed");
      sum[0] += a;
      sum[1] += b;
      sum[2] += c;
      sum[3] += (double)a + b + c;
    }
    std::memcpy(ms4, sum, sizeof sum);
    if (launches) *launches = n + (long long)done.size();
    std::lock_guard<std::mutex> lk(s->timing_mu);
    for (auto& q : done) s->timing.spare.push_back(q);
    return RT_OK;
  });
}

int rt_write_png(const char* path, const float* rgb, int width, int height) {
  if (!path || !rgb) return set_error(RT_E_INVALID, "rt_write_png: NULL argument");
  return guarded([&] {
    write_png(path, rgb, width, height);
    return RT_OK;
  });
}

}  // extern "C"

// ------------------------------------------------------------------ films
// A film owns its Pixels and its two sample counters; everything a call needs besides lives in
// the working set of the stream it runs on.
struct rt_film {
  rt_scene* s = nullptr;
  int width = 0, height = 0, filter = RT_FILM_GAUSSIAN;
  float sigma = 1.0f / 3.0f;
  DevBuf<float> pixels;                // width * height * 4
  DevBuf<unsigned long long> counts;   // samples added, samples dropped
  // rt_film_set_stage_timing: the events around the last timed splat's stages
  std::mutex mu;
  bool timing = false, timed = false;
  Event marks[kFilmStages + 1];
  size_t pixel_count() const { return (size_t)width * (size_t)height; }
};

namespace {

Replica& film_replica(rt_film* f) { return *f->s->rep[0]; }

// Argument rules of the splat entries; they need no GPU.
void check_film_batch(const char* fn, const rt_film* f, const void* xy, const void* other,
                      long long n) {
  const std::string name(fn);
  if (!f) throw std::invalid_argument(name + ": film is NULL");
  if (n < 0) throw std::invalid_argument(name + ": n < 0");
  if (n > kFilmMaxSamples)
    throw std::invalid_argument(name + ": more than 2^28 samples in one call (cut the batch: the "
                                       "cut decides the order)");
  if (n > 0 && (!xy || !other)) throw std::invalid_argument(name + ": NULL pointer");
  if ((uintptr_t)xy % 8 != 0 || (uintptr_t)other % 16 != 0)
    throw std::invalid_argument(name + ": positions must be 8-byte aligned, colours and rays "
                                       "16-byte aligned");
}

void film_clear_on(rt_film* f, hipStream_t stream) {
  hip_check(hipMemsetAsync(f->pixels.p, 0, f->pixel_count() * 4 * sizeof(float), stream),
            "clear film");
  hip_check(hipMemsetAsync(f->counts.p, 0, 2 * sizeof(unsigned long long), stream),
            "clear film counters");
}

// One splat of n > 0 samples on `stream` with its working set; rays: the fused entry's (their
// validity joins the samples'), or null.
void film_splat_on(rt_film* f, const float* xy, const rt_radiance* rad, const rt_ray* rays,
                   long long n, WorkSet& ws, hipStream_t stream) {
  const size_t pixels = f->pixel_count();
  ws.film.reserve(film_scratch_words(pixels, n), "alloc film scratch");
  FilmParams F;
  std::memset(&F, 0, sizeof F);
  F.pixels = f->pixels.p;
  F.counts = f->counts.p;
  F.xy = xy;
  F.rad = rad;
  F.rays = rays;
  F.n = n;
  F.width = f->width;
  F.height = f->height;
  F.filter = f->filter == RT_FILM_BOX ? kFilmBox : kFilmGaussian;
  F.sigma = f->sigma;
  F.offs = ws.film.p;
  F.sums = F.offs + pixels;
  F.list = F.sums + film_scan_words(pixels);
  F.longs = F.list + (size_t)n;
  std::lock_guard<std::mutex> lk(f->mu);
  const hipEvent_t* marks = nullptr;
  hipEvent_t ev[kFilmStages + 1];
  if (f->timing) {
    for (int k = 0; k <= kFilmStages; k++) {
      f->marks[k].create();
      ev[k] = f->marks[k];
    }
    marks = ev;
    f->timed = true;
  }
  hip_check(launch_film_splat(F, marks, stream), "film splat launch");
}

// The fused entry's two halves on `stream`: the radiance query into ws.film_rad, then the splat.
void film_shade_on(rt_film* f, const rt_ray* rays, const float* xy, long long n, int depth,
                   int flags, WorkSet& ws, unsigned long long* counters, hipStream_t stream,
                   const LightList& lit = {nullptr, 0}) {
  ws.film_rad.reserve((size_t)n, "alloc film radiance");
  enqueue_radiance(f->s, film_replica(f), QueryCall{rays, n, ws.film_rad.p, depth, flags, lit}, ws,
                   counters, stream);
  film_splat_on(f, xy, ws.film_rad.p, rays, n, ws, stream);
}

constexpr int kFilmShadeFlags = RT_QUERY_REORDER | RT_QUERY_IN_MEDIUM | RT_QUERY_RAY_TIME;

// A `_device` entry's body on the caller's stream, with that stream's working set.
template <typename Body>
int film_device_call(rt_film* f, void* stream, Body&& body) {
  Replica& r = film_replica(f);
  DeviceGuard g(r.device);
  std::unique_lock<std::mutex> lk;
  StreamScratch* sc = scratch_for(f->s, r, stream, lk);
  body(sc->work, (hipStream_t)stream);
  hip_check(hipEventRecord(sc->done, (hipStream_t)stream), "event record");
  return RT_OK;
}

// The fused `_device` entries: `lit` null (rt_film_shade_rays_device) or the caller's records.
int film_shade_device(const char* fn, rt_film* f, const rt_ray* d_rays, const float* d_xy,
                      long long n, int depth, const LightList* lit, int flags, void* stream) {
  return guarded([&]() -> int {
    if (lit) check_light_args(fn, *lit, flags);
    check_film_batch(fn, f, d_xy, d_rays, n);
    if (flags & ~(kFilmShadeFlags | (lit ? kLitFlags : 0)))
      throw std::invalid_argument(std::string(fn) + ": unknown flag bit");
    depth = radiance_depth(fn, f->s, depth);
    if (n == 0) return RT_OK;
    return film_device_call(f, stream, [&](WorkSet& ws, hipStream_t st) {
      film_shade_on(f, d_rays, d_xy, n, depth, flags, ws, film_replica(f).d_counters.p, st,
                    lit ? *lit : LightList{nullptr, 0});
    });
  });
}

// The fused host entries, likewise.
int film_shade_host(const char* fn, rt_film* f, const rt_ray* rays, const float* xy, long long n,
                    int depth, const LightList* lit, int flags, rt_stats* stats) {
  return guarded([&] {
    if (lit) check_light_args(fn, *lit, flags);
    check_film_batch(fn, f, xy, rays, n);
    if (flags & ~(kFilmShadeFlags | (lit ? kLitFlags : 0)))
      throw std::invalid_argument(std::string(fn) + ": unknown flag bit");
    depth = radiance_depth(fn, f->s, depth);
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return RT_OK;
    DeviceGuard g(film_replica(f).device);
    CtxLease lease(f->s, 1);
    RenderCtx* x = lease.x[0];
    x->d_rays.reserve((size_t)n, "alloc rays");
    x->d_xy.reserve(2 * (size_t)n, "alloc positions");
    hip_check(hipMemcpyAsync(x->d_rays.p, rays, (size_t)n * sizeof(rt_ray), hipMemcpyHostToDevice,
                             x->stream), "upload rays");
    hip_check(hipMemcpyAsync(x->d_xy.p, xy, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice,
                             x->stream), "upload positions");
    LightList d_lit{nullptr, 0};
    if (lit && lit->k > 0) d_lit = upload_lights(x, *lit, n, flags);
    CallCounters counted(f->s, lease.x);
    film_shade_on(f, x->d_rays.p, x->d_xy.p, n, depth, flags, x->work, x->d_cnt.p, x->stream, d_lit);
    counted.stop();
    counted.read(stats);
    return RT_OK;
  });
}

}  // namespace

extern "C" {

int rt_film_version(void) { return 1; }

int rt_film_create(rt_scene* s, int width, int height, int filter, float sigma, rt_film** out) {
  if (out) *out = nullptr;
  return guarded([&] {
    if (!s || !out) throw std::invalid_argument("rt_film_create: NULL argument");
    if (width < 1 || width > kFilmMaxSide || height < 1 || height > kFilmMaxSide)
      throw std::invalid_argument("rt_film_create: width and height must be in [1, 32768]");
    if (filter != RT_FILM_GAUSSIAN && filter != RT_FILM_BOX)
      throw std::invalid_argument("rt_film_create: unknown filter");
    if (!std::isfinite(sigma) || sigma < 0.0f)
      throw std::invalid_argument("rt_film_create: sigma must be finite and >= 0");
    if (s->multi)
      throw std::domain_error("rt_film_create: films on multi-device scenes are not supported");
    auto f = std::make_unique<rt_film>();
    f->s = s;
    f->width = width;
    f->height = height;
    f->filter = filter;
    f->sigma = sigma == 0.0f ? 1.0f / 3.0f : sigma;
    Replica& r = *s->rep[0];
    DeviceGuard g(r.device);
    f->pixels.reserve(f->pixel_count() * 4, "alloc film");
    f->counts.reserve(2, "alloc film counters");
    hip_check(hipMemset(f->pixels.p, 0, f->pixel_count() * 4 * sizeof(float)), "clear film");
    hip_check(hipMemset(f->counts.p, 0, 2 * sizeof(unsigned long long)), "clear film counters");
    *out = f.release();
    return RT_OK;
  });
}

void rt_film_destroy(rt_film* f) {
  if (!f) return;
  DeviceGuard g(film_replica(f).device, std::nothrow);
  (void)hipDeviceSynchronize();  // no call on it is still running
  delete f;
}

int rt_film_clear_device(rt_film* f, void* stream) {
  return guarded([&] {
    if (!f) throw std::invalid_argument("rt_film_clear_device: film is NULL");
    DeviceGuard g(film_replica(f).device);
    film_clear_on(f, (hipStream_t)stream);
    return RT_OK;
  });
}

int rt_film_splat_device(rt_film* f, const float* d_xy, const rt_radiance* d_rad, long long n,
                         void* stream) {
  return guarded([&]() -> int {
    check_film_batch("rt_film_splat_device", f, d_xy, d_rad, n);
    if (n == 0) return RT_OK;
    return film_device_call(f, stream, [&](WorkSet& ws, hipStream_t st) {
      film_splat_on(f, d_xy, d_rad, nullptr, n, ws, st);
    });
  });
}

int rt_film_shade_rays_device(rt_film* f, const rt_ray* d_rays, const float* d_xy, long long n,
                              int depth, int flags, void* stream) {
  return film_shade_device("rt_film_shade_rays_device", f, d_rays, d_xy, n, depth, nullptr, flags,
                           stream);
}

int rt_film_shade_rays_lit_device(rt_film* f, const rt_ray* d_rays, const float* d_xy, long long n,
                                  int depth, const rt_light_sample* d_lights, int k, int flags,
                                  void* stream) {
  const LightList lit{d_lights, k};
  return film_shade_device("rt_film_shade_rays_lit_device", f, d_rays, d_xy, n, depth, &lit, flags,
                           stream);
}

int rt_film_resolve_device(rt_film* f, float* d_rgb, void* stream) {
  return guarded([&] {
    if (!f || !d_rgb) throw std::invalid_argument("rt_film_resolve_device: NULL argument");
    DeviceGuard g(film_replica(f).device);
    hip_check(launch_film_resolve(f->pixels.p, d_rgb, f->width, f->height, (hipStream_t)stream),
              "film resolve launch");
    return RT_OK;
  });
}

int rt_film_clear(rt_film* f) {
  return guarded([&] {
    if (!f) throw std::invalid_argument("rt_film_clear: film is NULL");
    DeviceGuard g(film_replica(f).device);
    CtxLease lease(f->s, 1);
    film_clear_on(f, lease.x[0]->stream);
    hip_check(hipStreamSynchronize(lease.x[0]->stream), "synchronize film clear");
    return RT_OK;
  });
}

int rt_film_splat(rt_film* f, const float* xy, const rt_radiance* rad, long long n) {
  return guarded([&] {
    check_film_batch("rt_film_splat", f, xy, rad, n);
    if (n == 0) return RT_OK;
    DeviceGuard g(film_replica(f).device);
    CtxLease lease(f->s, 1);
    RenderCtx* x = lease.x[0];
    x->d_xy.reserve(2 * (size_t)n, "alloc positions");
    x->d_ray_out.reserve(((size_t)n + 1) / 2, "alloc colours");
    rt_radiance* d_rad = reinterpret_cast<rt_radiance*>(x->d_ray_out.p);
    hip_check(hipMemcpyAsync(x->d_xy.p, xy, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice,
                             x->stream), "upload positions");
    hip_check(hipMemcpyAsync(d_rad, rad, (size_t)n * sizeof(rt_radiance), hipMemcpyHostToDevice,
                             x->stream), "upload colours");
    film_splat_on(f, x->d_xy.p, d_rad, nullptr, n, x->work, x->stream);
    hip_check(hipStreamSynchronize(x->stream), "synchronize film splat");
    return RT_OK;
  });
}

int rt_film_shade_rays(rt_film* f, const rt_ray* rays, const float* xy, long long n, int depth,
                       int flags, rt_stats* stats) {
  return film_shade_host("rt_film_shade_rays", f, rays, xy, n, depth, nullptr, flags, stats);
}

int rt_film_shade_rays_lit(rt_film* f, const rt_ray* rays, const float* xy, long long n, int depth,
                           const rt_light_sample* lights, int k, int flags, rt_stats* stats) {
  const LightList lit{lights, k};
  return film_shade_host("rt_film_shade_rays_lit", f, rays, xy, n, depth, &lit, flags, stats);
}

int rt_film_resolve(rt_film* f, float* rgb) {
  return guarded([&] {
    if (!f || !rgb) throw std::invalid_argument("rt_film_resolve: NULL argument");
    DeviceGuard g(film_replica(f).device);
    CtxLease lease(f->s, 1);
    RenderCtx* x = lease.x[0];
    const size_t floats = f->pixel_count() * 3;
    x->d_xy.reserve(floats, "alloc resolved frame");
    hip_check(launch_film_resolve(f->pixels.p, x->d_xy.p, f->width, f->height, x->stream),
              "film resolve launch");
    hip_check(hipMemcpyAsync(rgb, x->d_xy.p, floats * sizeof(float), hipMemcpyDeviceToHost,
                             x->stream), "download frame");
    hip_check(hipStreamSynchronize(x->stream), "synchronize film resolve");
    return RT_OK;
  });
}

int rt_film_read(rt_film* f, float* color_weight4) {
  return guarded([&] {
    if (!f || !color_weight4) throw std::invalid_argument("rt_film_read: NULL argument");
    DeviceGuard g(film_replica(f).device);
    hip_check(hipDeviceSynchronize(), "synchronize device");
    hip_check(hipMemcpy(color_weight4, f->pixels.p, f->pixel_count() * 4 * sizeof(float),
                        hipMemcpyDeviceToHost), "read film");
    return RT_OK;
  });
}

int rt_film_counts(rt_film* f, long long out2[2]) {
  return guarded([&] {
    if (!f || !out2) throw std::invalid_argument("rt_film_counts: NULL argument");
    DeviceGuard g(film_replica(f).device);
    hip_check(hipDeviceSynchronize(), "synchronize device");
    unsigned long long c[2];
    hip_check(hipMemcpy(c, f->counts.p, sizeof c, hipMemcpyDeviceToHost), "read film counters");
    out2[0] = (long long)c[0];
    out2[1] = (long long)c[1];
    return RT_OK;
  });
}

int rt_film_set_stage_timing(rt_film* f, int enable) {
  if (!f) return set_error(RT_E_INVALID, "rt_film_set_stage_timing: film is NULL");
  std::lock_guard<std::mutex> lk(f->mu);
  f->timing = enable != 0;
  return RT_OK;
}

int rt_film_stage_times(rt_film* f, double ms5[5]) {
  return guarded([&] {
    if (!f || !ms5) throw std::invalid_argument("rt_film_stage_times: NULL argument");
    std::lock_guard<std::mutex> lk(f->mu);
    if (!f->timed) throw std::invalid_argument("rt_film_stage_times: no splat was timed");
    DeviceGuard g(film_replica(f).device);
    hip_check(hipEventSynchronize(f->marks[kFilmStages]), "synchronize film stages");
    for (int k = 0; k < kFilmStages; k++) {
      float ms = 0;
      hip_check(hipEventElapsedTime(&ms, f->marks[k], f->marks[k + 1]), "elapsed");
      ms5[k] = ms;
    }
    return RT_OK;
  });
}

}  // extern "C"
