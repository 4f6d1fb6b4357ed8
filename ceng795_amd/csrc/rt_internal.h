// Internal layouts shared by the host scene builder and the HIP kernels.
//
// HBM layout (see DESIGN.md §Data layout):
//   nodes   : DevNode[num_nodes]    64 B, BVH2 internal nodes in DFS preorder; each holds
//                                    both CHILD boxes, so one s_load_dwordx16 per visit tests
//                                    both children (the reference tests a node's own box on
//                                    entry, HW2/Bounding_volume_hierarchy.cpp:32-35 — same set).
//   prims   : DevPrim[num_leaves]   48 B, leaves in DFS order: leaf index == the reference's
//                                    DFS leaf order, which is the closest-hit tie-break key.
//   normals : float4[num_leaves]     flat normal (Triangle.cpp:14) + material id, read once
//                                    per pixel for the winning leaf only.
#ifndef CENG795_RT_INTERNAL_H_
#define CENG795_RT_INTERNAL_H_

#include <stdint.h>

namespace rt {

constexpr int kTile = 8;          // one wavefront = one 8x8 pixel packet
constexpr int kWavesPerBlock = 4; // 256-thread workgroups
constexpr int kLaneStack = 64;    // per-wave traversal stack held one entry per VGPR lane
constexpr int kCounterRows = 64;  // ray-counter rows (spread atomics)
constexpr int kCounterWidth = 16; // u64 counters per row
// counter columns
enum : int {
  kCntPrimary = 0, kCntShadow = 1, kCntSecondary = 2, kCntHits = 3,
  // RT_DIAG builds only: packet-level traversal work
  kCntPrimNodes = 4, kCntPrimNodeLanes = 5, kCntPrimLeaves = 6, kCntPrimLeafLanes = 7,
  kCntShadNodes = 8, kCntShadNodeLanes = 9, kCntShadLeaves = 10, kCntShadLeafLanes = 11,
  kCntExactBox = 12,
  kCntGuardTests = 13,  // RT_DIAG: leaf-batch guard tests (primary + shadow)
  // RT_DIAG builds: the node visits above that were 8-wide culling nodes (128 B each)
  kCntPrimWide = 14, kCntShadWide = 15
};

// RT_DIAG per-phase attribution (rt_debug_phases, tools/phases.py): per traversal kind (primary,
// shadow) the visit loop's events, then shader-clock cycle sums.
enum : int {
  kPhVisits = 0, kPhSlotsTested = 1, kPhSlotHits = 2, kPhLeafyHits = 3, kPhPairHits = 4,
  kPhInnerHits = 5, kPhPushes = 6, kPhPops = 7, kPhFlushes = 8, kPhFlushIters = 9,
  kPhaseEvents = 10
};
enum : int {
  kPhCycPrimTotal = 2 * kPhaseEvents, kPhCycPrimVisit, kPhCycPrimLoad, kPhCycPrimFlush,
  kPhCycShadTotal, kPhCycShadVisit, kPhCycShadLoad, kPhCycShadFlush, kPhCycShade,
  kPhCycFrame, kPhWaves,
  // mid-walk leaf flushes (primary + shadow) by the remainder they carried: 0, 1-16, 48-63
  kPhCarryZero, kPhCarryLow, kPhCarryHigh,
  // the leaf batch's deferred guard, kDeferEvents values per traversal kind:
  // primary from kPhDeferPrim, shadow from kPhDeferShad
  kPhDeferPrim, kPhDeferShad = kPhDeferPrim + 4,
  // the frame kernel's octant loop: packets with an active lane and their sub-walks (one per
  // direction-sign octant among the active lanes), primary then shadow (per light)
  kPhOctPrimPackets = kPhDeferShad + 4, kPhOctPrimWalks, kPhOctShadPackets, kPhOctShadWalks,
  // a packet's time outside its walks: the prologue (kernel entry until the wave has its tile),
  // then per traversal kind the set-up before the walks (pixel, ray; per light in the shadow
  // phase), the walks themselves and the tail after them (record / occlusion store, the ray
  // counters); stamped before the diagnostic atomics, which fall into no section (the phase
  // totals above still enclose them)
  kPhCycPrologue, kPhCycPrimSetup, kPhCycPrimWalk, kPhCycPrimTail, kPhCycShadSetup,
  kPhCycShadWalk, kPhCycShadTail,
  // the shading phase (kPhCycShade) in three: until the hit record is back, the dependent
  // normal -> material loads, and the arithmetic with the colour store
  kPhCycShadeRecord, kPhCycShadeLoads, kPhCycShadeMath,
  kPhaseSlots
};
// Per traversal kind: queued tests whose triangle / sphere test hit in range (the only ones whose
// guard decision is used), the 64-survivor guard iterations, the guard batches in which one
// 64-test iteration's survivors fell on both sides of the full survivor buffer, and the
// survivors the guard rejected.  (A walk that takes the guard decision before the triangle test
// counts the first and the last and leaves the other two at 0.)
enum : int {
  kDfSurvivors = 0, kDfGuardIters = 1, kDfSplitDrains = 2, kDfRejected = 3, kDeferEvents = 4
};

constexpr int kDefaultTreeletLeaves = 2;  // culling-tree treelets: lone leaves and leaf pairs

struct alignas(16) DevNode {
  // Both CHILD boxes, interleaved per coordinate ([axis][child]).  Unused for a leaf child (a
  // +-1e30 box every normalised ray accepts, scene_build.cpp).
  float lo[3][2];
  float hi[3][2];
  int32_t child[2];  // >= 0: internal node index; < 0: leaf index ~child
  int32_t axis;      // split dimension of THIS node (Bounding_volume_hierarchy.cpp:8)
  int32_t pad;       // 0 (reference nodes; the culling tree has its own record, DevNode8)
};
static_assert(sizeof(DevNode) == 64, "node must be one 64-byte scalar load");

// 8-wide culling node (accel_build.cpp): two consecutive DevNode slots of
// `nodes`, referred to as (index of the first slot) | kWideTag.  Slot c is valid when bit c of
// `kinds` is set; it is then either LEAFY (bit 8 + c: one treelet = a lone leaf, or with bit
// 16 + c a leaf pair; its leaves are DevLeaf records leaf_base + (offs >> 4c & 15) and the next
// one) or INNER (a child node: inner_base + 2c).  The slots are sorted by kind: the inner slots
// lie at 0, 1, ... and the leafy slots at 7, 6, ..., the invalid ones between them, so a visit
// runs up the inner slots and down the leafy ones and never asks a slot's kind (visit_wide);
// the top byte of `kinds` holds the two counts.  Every slot
// carries a CONSERVATIVE box in fp16, relative to `origin` and scaled by 2^k per axis:
//   plane = origin[a] + h * 2^(scale byte a, signed)
// rounded outward and inflated by the scene's culling margin (HostScene::cull_margin), so a
// plain slab test (no decision band) never culls a treelet the reference would enter; the
// exact decision (the treelet's guard box) is taken per ray in the leaf batch.  An invalid
// slot holds NaN planes, which every slab test rejects.
constexpr int32_t kWideTag = 1 << 30;
// The culling nodes exist once per direction-sign octant (round 11, §4.3):
// copy k = (1/d_x < 0) | (1/d_y < 0) << 1 | (1/d_z < 0) << 2 follows copy k - 1 at a stride of
// HostScene::accel_stride node slots (RenderParams::accel_stride).  In copy k the slot words
// box[c][x] of every axis x whose bit of k is set have their halves swapped — the ENTRY plane of
// a ray of octant k is the low half of every word — and inner_base points into the same copy, so
// a walk that starts at accel_root + k * stride stays in copy k.  leaf_base, kinds, offs and the
// leaf records are the same in every copy.  The frame kernel walks a packet per octant and reads
// the halves as they lie; every other kernel walks copy 0 and orders the planes per lane.
constexpr int kOctantCopies = 8;
// node slots a scene may have: the traversal loads a wide node at the 32-bit byte offset
// (ref << 6) (rt_kernels.hip load_node8), so reference slots + kOctantCopies x culling slots
// stay below 2^26 (about 22 M triangles with eight copies); a larger scene is refused
// (accel_build.cpp accel_slots_error)
constexpr size_t kMaxNodeSlots = size_t(1) << 26;
constexpr int kWideSlots = 8;
// Entry cuts (entry_cuts.cpp): node references per frame tile at which the frame
// kernel's primary walks start — one 16-byte record, one scalar load.  (A/B builds: 1, 2.)
#ifndef RT_ENTRY_CUT
#define RT_ENTRY_CUT 4
#endif
constexpr int kEntryCut = RT_ENTRY_CUT;
static_assert(kEntryCut == 1 || kEntryCut == 2 || kEntryCut == 4, "a record is one scalar load");
enum : int32_t { kSlotValid = 1, kSlotLeafy = 1 << 8, kSlotPair = 1 << 16 };
constexpr int kSlotInnerCountShift = 24, kSlotLeafyCountShift = 28;  // counts 0..8, 4 bits each
struct alignas(16) DevNode8 {
  float origin[3];
  uint32_t scale;      // byte a: k_a as a signed byte
  int32_t inner_base;  // DevNode index of slot 0's child (children contiguous, 2 slots each)
  int32_t leaf_base;   // DevLeaf index of the node's first leaf (slot 7's, the first visited)
  int32_t kinds;       // kSlotValid << c | kSlotLeafy << c | kSlotPair << c | the two counts
  uint32_t offs;       // 4 bits per slot: its first leaf's offset from leaf_base (leafy slots)
  uint32_t box[kWideSlots][3];  // per slot and axis: lo fp16 (bits 0-15), hi fp16 (16-31)
};
static_assert(sizeof(DevNode8) == 128, "a wide node is two s_load_dwordx16");
static_assert(sizeof(DevNode8) == 2 * 64, "a wide node is two node slots");

// A leaf as the fast traversal tests it, in culling-tree order (each wide node's leaves
// contiguous): the primitive (as DevPrim), its DFS leaf index — the reference's tie-break key
// and the index of every per-leaf array — and the GUARD box, the box of the reference node
// holding the leaf.  A ray may test the leaf iff every reference ancestor box accepts it
// (HW2/Bounding_volume_hierarchy.cpp:31-55); the guard accepting with margin implies that
// (DESIGN.md §4.1), else the kernel walks the ancestry (guard_exact).
//   q[0] = v0.xyz, dfs | kLeafSphere      q[1] = a1.xyz (sphere: radius, 0, 0), guard lo.x
//   q[2] = a2.xyz, guard lo.y              q[3] = guard lo.z, hi.xyz
constexpr int32_t kLeafSphere = 1 << 30;
struct alignas(16) DevLeaf {
  float v0[3];
  int32_t dfs;  // | kLeafSphere for a sphere
  float a1[3];
  float g0;
  float a2[3];
  float g1;
  float g2, g3, g4, g5;
};
static_assert(sizeof(DevLeaf) == 64, "leaf record is four 16-byte loads");

enum PrimKind : int32_t { kPrimTriangle = 0, kPrimSphere = 1 };

struct alignas(16) DevPrim {
  // triangle: v0, a1 = v0 - v1, a2 = v0 - v2 (Triangle.cpp:43-44, same fp32 rounding)
  // sphere:   v0 = center, a1[0] = radius
  float v0[3];
  float a1[3];
  float a2[3];
  int32_t kind;
  int32_t material;
  float cx;  // triangle: a1.y*a2.z - a2.y*a1.z (the d-free minor of Triangle.h:35-37)
};
static_assert(sizeof(DevPrim) == 48, "prim record is three 16-byte loads");

// Range in which the triangle test's three divisions (v0 - o) / det may share one reciprocal
// (tri_quotients in rt_kernels.hip): a coordinate is 0 or 2^-26 <= |x| <= 2^48, so every
// difference v0 - o is 0 or 2^-49 <= |v0 - o| <= 2^49.
inline bool quot_coord_ok(float x) {
  const float a = x < 0 ? -x : x;
  return a == 0.0f || (a >= 0x1p-26f && a <= 0x1p48f);
}

// Reference ancestry for the culling tree's exact guard (accel_build.cpp): entry i holds
// reference node i's own box and parent (-1 at the root), and the node holding leaf i.
struct alignas(16) DevAncestry {
  float box[6];
  int32_t parent;
  int32_t leaf_parent;
};
static_assert(sizeof(DevAncestry) == 32, "");

struct DevMaterial {  // HW2/Material.h
  float ambient[3], diffuse[3], specular[3], mirror[3], transparency[3];
  float refraction_index, phong_exponent;
  float pad[3];
};
static_assert(sizeof(DevMaterial) == 80, "");

struct DevLight {
  float position[3];
  float intensity[3];
  float pad[2];
};

enum RootKind : int32_t { kRootNode = 0, kRootTriangle = 1, kRootSphere = 2 };

constexpr unsigned kMinstdM = 2147483647u;  // minstd_rand0 modulus (std::default_random_engine)
constexpr unsigned kMinstdA = 16807u;

// Resolve of the Gaussian MSAA splat: samples[s][h][w][3] -> out[h][w][3] = color / weight.
struct MsaaResolveParams {
  const float* samples;
  float* out;
  int width, height, n;
  unsigned long long seed;
  int row_lo, row_hi;  // the rows resolved: [row_lo, row_hi) (a multi-device band)
};

// Untile of a multi-device frame (rt_api.hip render_multi): the frame's tiles were dealt
// round-robin over `devices` (tile t -> device t mod devices, slot position t / devices) and
// gathered as recv[devices][slot][64 pixels][3]; writes the selected rows of the row-major
// frame out[h][w][3] (logical row k = image row row0 + k*row_stride).
#if defined(__HIPCC__)
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

// Pixel record (rt_render_device with RT_TILE_RECORDS; rt_resolve_device): what a share of a
// multi-GPU frame sends to the gathering rank instead of 12 B of colour — the primary hit's DFS
// leaf index (bits 0..25) and the shadow bits of lights 0..3 (bits 26..29); or a miss (the
// background) or a pixel outside the image.  The gathering rank re-derives the hit's t with the
// same intersection arithmetic (bit for bit) and shades it there.
constexpr unsigned kRecLeafMask = (1u << 26) - 1u;
constexpr int kRecLightShift = 26;
constexpr unsigned kRecLightMask = 15u;  // lights 0..3
constexpr int kRecMaxLights = 4;
constexpr unsigned kRecMiss = 1u << 30;
constexpr unsigned kRecOutside = 2u << 30;

// Block deal (rt_render_device with RT_TILE_BLOCKS, multi-device frames): the unit dealt over
// devices is a 2x2 block of tiles (the traversal workgroup's unit, so a share keeps the
// in-place frame's coherence), numbered with each block row rotated by its row index —
// d = by * nbx + (bx - by) mod nbx — so that a deal d = r (mod N) takes diagonal stripes of
// blocks rather than the same columns in every row (nbx is often a multiple of N).  Selected
// block k holds tiles 4k .. 4k + 3 of the selection (w = 2 * (ty & 1) + (tx & 1)).
RT_HD inline int deal_blocks_x(int tiles_x) { return (tiles_x + 1) >> 1; }
RT_HD inline int deal_blocks(int tiles_x, int tiles_y) {
  return deal_blocks_x(tiles_x) * ((tiles_y + 1) >> 1);
}
RT_HD inline void deal_block_tile(int tiles_x, int d, int w, int& tx, int& ty) {
  const int nbx = deal_blocks_x(tiles_x), by = d / nbx;
  int bx = d - by * nbx + by % nbx;
  if (bx >= nbx) bx -= nbx;
  tx = 2 * bx + (w & 1);
  ty = 2 * by + (w >> 1);
}
RT_HD inline int deal_block_index(int tiles_x, int tx, int ty, int& w) {
  const int nbx = deal_blocks_x(tiles_x), bx = tx >> 1, by = ty >> 1;
  w = ((ty & 1) << 1) | (tx & 1);
  int c = bx - by % nbx;
  if (c < 0) c += nbx;
  return by * nbx + c;
}

struct UntileParams {
  const float* recv;
  float* out;
  int width, row0, row_stride, rows, tiles_x, tiles_total, devices, slot;
  int tile_offset;  // deal unit u went to rank (u + tile_offset) mod devices (rt_untile_device)
  int blocks;       // 1: the units are 2x2 blocks in deal order (deal_block_index), else tiles
  int vec;          // 1: rows and buffers 16-B aligned (untile by 16-B chunks)
  int skip_root;    // 1: rank 0's units are left alone (it rendered them in place)
};

// The schedule buffer (`sched`) of a launch of `tiles` selected tiles, sched_words_for(tiles)
// words, `tiles` being the launch's final num_sel_tiles:
//   [0, tiles)                         tile costs the frame kernel measures (RenderParams::tile_cost)
//   [tiles, sched_snap_offset(tiles))  the unit order lists, regions x order_stride words
//                                      (RenderParams::unit_order; order_geometry in rt_kernels.hip
//                                      runs a launch whose lists would not fit in block order)
//   [sched_snap_offset(tiles), +tiles) the snapshot of the costs the order kernel sorted
//                                      (rt_tile_costs)
constexpr unsigned long long sched_words_for(unsigned long long tiles) { return 10 * tiles + 64; }
constexpr unsigned long long sched_snap_offset(unsigned long long tiles) { return 9 * tiles + 64; }

// Traversal workgroups (the frame kernel's): kTraceWaves packets, which with
// RenderParams::tile_block form a kBlockW x kBlockH block of tiles (rt_kernels.hip).
#ifndef RT_TRACE_WAVES
#define RT_TRACE_WAVES 2
#endif
constexpr int kTraceWaves = RT_TRACE_WAVES;
static_assert(kTraceWaves == 1 || kTraceWaves == 2 || kTraceWaves == 4, "1, 2 or 4 waves");
constexpr int kBlockW = kTraceWaves >= 2 ? 2 : 1, kBlockH = kTraceWaves / kBlockW;

// n / d for every 0 <= n < 2^31 as one 32 x 32 -> 64-bit multiply and a shift, the divisor being
// wave-uniform but known only at launch (the compiler expands such a division into ~28 dependent
// instructions).  With s = ceil(log2 d), k = 31 + s and mul = ceil(2^k / d) < 2^32:
// mul d = 2^k + e, 0 <= e < d <= 2^s, so n mul / 2^k = n / d + n e / (d 2^k) and the excess is
// below 1 / d because n e < 2^31 2^s = 2^k — the floor is the quotient's.
struct DivMagic {
  unsigned mul;
  int shift;  // k: 31 .. 62
};
RT_HD inline DivMagic div_magic(int d) {
  const unsigned long long ud = d < 1 ? 1ull : (unsigned long long)d;
  int s = 0;
  while ((1ull << s) < ud) s++;
  DivMagic m;
  m.shift = 31 + s;
  m.mul = (unsigned)(((1ull << m.shift) + ud - 1) / ud);
  return m;
}
RT_HD inline int div_by(int n, DivMagic m) {
  return (int)(((unsigned long long)(unsigned)n * m.mul) >> m.shift);
}

// The frame kernel's coherent visits run in scaled time t' = t 2^-E (visit_wide, DESIGN.md
// §4.2): the slot test's zero bound is the clamp of axis 0's entry plane to [0, 1], which leaves
// every entry distance below 1 as it is.  E is the launch's: the smallest exponent with 2^E at
// least kVisitTimeFactor times the larger of the camera's distance to the farthest corner of the
// culling tree's root box (a primary ray enters every box inside it earlier than that, its
// direction being a unit vector) and the box's diagonal (a shadow ray starts inside the box).
// Kept within +-kVisitTimeExpMax, where a reciprocal of any |d| >= 1e-6 (at most 2^20, and at least
// 1 for a unit vector) times 2^-E stays normal and finite; a box beyond that range, like a
// distance above 1 of any other cause, only costs culling (the clamp lowers an entry distance).
// A box or camera that is not finite gives 0.
constexpr int kVisitTimeFactor = 2, kVisitTimeExpMax = 64;
RT_HD inline int visit_time_exp(const float* box6, const float* cam3) {
  double far2 = 0.0, diag2 = 0.0;
  for (int x = 0; x < 3; x++) {
    const double lo = box6[x], hi = box6[x + 3], c = cam3[x];
    if (!(lo - lo == 0.0 && hi - hi == 0.0 && c - c == 0.0)) return 0;  // an inf or a NaN
    const double a = c - lo < 0 ? lo - c : c - lo, b = c - hi < 0 ? hi - c : c - hi;
    const double f = a > b ? a : b;
    far2 += f * f;
    diag2 += (hi - lo) * (hi - lo);
  }
  const double r2 = far2 > diag2 ? far2 : diag2;
  if (!(r2 > 0.0)) return 0;  // a box and a camera at one point: nothing to scale
  // the smallest E with 4^E >= kVisitTimeFactor^2 r2 (the doubles hold every fp32 square exactly
  // enough: a root that rounds up only makes E one larger)
  const double need = (double)(kVisitTimeFactor * kVisitTimeFactor) * r2;
  int e = -kVisitTimeExpMax;
  double p = 1.0;
  for (int k = 0; k < 2 * kVisitTimeExpMax; k++) p *= 0.5;  // 4^-kVisitTimeExpMax
  while (e < kVisitTimeExpMax && p < need) {
    p *= 4.0;
    e++;
  }
  return e;
}

// What a traversal launch's index arithmetic divides by, worked out once on the host
// (packet_geom below, called by order_geometry in rt_kernels.hip) instead of by every wave, and
// the frame kernel's time scale: an argument of its own of the kernels that use it, so
// RenderParams keeps its layout.
struct PacketGeom {
  DivMagic by_tiles_x;    // a tile's row and column
  DivMagic by_deal_nbx;   // block deal: blocks per block row (deal_blocks_x)
  DivMagic by_block_nbx;  // tile_block: workgroup blocks per block row
  DivMagic by_regions;    // ordered dispatch: a workgroup's region and list entry
  int block_nbx;          // ceil(tiles_x / kBlockW)
  int sel_rows;           // the selection's tile rows, num_sel_tiles / tiles_x (tile_block)
  int packets;            // trace_packets
  int neg_t_exp;          // -E of the frame kernel's scaled visit time (visit_time_exp)
};

struct RenderParams {
  const DevNode* nodes;
  const DevLeaf* leaves;  // culling-tree order (DevLeaf), FAST traversal
  const DevPrim* prims;
  const float* normals;  // float4 per leaf: nx ny nz material(bits)
  const DevMaterial* materials;
  const DevLight* lights;
  int num_lights;
  int max_depth;
  float background[3];
  float ambient[3];
  float eps;
  int root_kind;
  int root_ref;           // kRootNode: node index; else leaf index
  float root_box[6];
  // culling tree (FAST traversal): root node index or -1, its conservative box, and the
  // reference ancestry a guard walks when its fast test cannot decide
  int accel_root;
  float accel_box[6];
  // every triangle's v0 coordinate is 0 or in [2^-26, 2^48] (quot_coord_ok): the triangle
  // test may take the shared-reciprocal quotient path (rt_kernels.hip, tri_quotients)
  int quot_ok;
  // node slots between the culling tree's octant copies (0: there are none); the root of octant k
  // is accel_root + k * accel_stride.  (In what was padding: no other field moved.)
  int accel_stride;
  const struct DevAncestry* anc;
  // camera (rt_camera)
  float cam_e[3], cam_tl[3], cam_su[3], cam_sv[3];
  int width, height;
  // row subset: image row of logical row k = row0 + k*row_stride
  int row0, row_stride, rows;
  // tiles over (rows x width), row-major; this launch does tile_begin + i*tile_step
  int tiles_x, tiles_total, tile_begin, tile_step, num_sel_tiles;
  int tile_major;
  int block_deal;  // the selection counts 2x2 blocks in deal order (deal_block_tile)
  int tile_block;  // traversal kernels: workgroups take 2-D blocks of tiles (rt_kernels.hip)
  // jittered MSAA (HW2/Scene.cpp:32-69): 0 = pixel centres; else this launch traces sample
  // msaa_s = x*n + y of every pixel, whose minstd_rand0 draws 2s+1, 2s+2 are
  // u0 * msaa_mul[0], u0 * msaa_mul[1] (mod 2^31-1), u0 the pixel's seeded state.
  int msaa_n, msaa_s;
  unsigned msaa_mul[2];
  unsigned long long msaa_seed;
  float* out;
  // Entry cuts (entry_cuts.cpp; null: every primary walk starts at the root): the camera's table
  // from the launch's first tile row on, kEntryCut node references per frame tile — record
  // ty * tiles_x + tx of the packet's tile.  Bound only when the launch's logical tile rows are
  // image tile rows (rt_api.hip bind_entry_cuts).  (In the place of the hit records' pointer of old,
  // which had stayed as a null word: no other field moves.)
  const int* entry_cuts;
  unsigned* occ;  // num_sel_tiles * 64 * occ_words light-occlusion bits: trace_shadow -> shade
  int occ_words;  // ceil(num_lights / 32)
  // heavy-first dispatch (null: off).  tile_cost[sel] holds each selected
  // tile's cost: the primary kernel's measured time (100 MHz ticks), read before the shadow
  // kernel.  order_kernel sorts the traversal
  // workgroups' units (kTraceWaves packets each) heaviest first within each of order_regions
  // regions into unit_order[region * order_stride + i] (-1 pads); region r holds the chunks of
  // order_chunk consecutive units c with c mod order_regions == r, and block b of an ordered
  // launch takes unit_order[(b mod regions) * stride + b / regions] — with 8 regions, the
  // blocks the hardware deals to one XCD walk one spatially coherent part of the frame,
  // heaviest first, so its L2 serves neighbouring packets.  use_order: this launch reads it.
  unsigned* tile_cost;
  int* unit_order;
  int order_regions, order_chunk, order_stride, order_units;
  int order_split;  // units per region the order kernel may split into quadrant waves per tile
  int use_order;
  // cold_order: the camera's whole-frame unit order seeded at scene creation from estimated tile
  // costs (rt_api.hip seed_cold_orders), for a frame without a previous one (no split entries);
  // used when the launch selects cold_tiles tiles (the whole frame), else nullptr
  const int* cold_order;
  int cold_tiles;
  // pair_rows: a row-major frame in host memory written over PCIe (rt_render, pinned): the two
  // tiles of a workgroup are written together as whole rows of 16 pixels (launch_variant
  // checks the layout; 0 = each wave writes its own tile)
  int pair_rows;
  int primary_order;  // the primary kernel too dispatches by unit_order: the order the previous
                      // frame of the same selection left on this stream (rt_api.hip warm order)
  int records;    // RT_TILE_RECORDS: the shading phase writes 32-bit pixel records, not RGB
  float* frames;  // recursive scenes only: (max_depth+1) * 28 * lanes ray-tree frames, else null
  // kCounterRows rows of kCounterWidth u64 (columns: kCnt*)
  unsigned long long* counters;
};

// ------------------------------------------------------------------ packet index arithmetic
// Which tile a wave of a traversal launch takes: shared by the kernels and the host (the CPU
// test runs these very functions, rt_host_packet_coords).  No run-time division on the device:
// the quotients come from the launch's PacketGeom G.

// RenderParams::tile_block of a launch: its selection is whole tile rows in frame order.
inline int whole_tile_rows(const RenderParams& P) {
  return P.tile_step == 1 && !P.block_deal && P.tile_begin % P.tiles_x == 0 &&
         P.num_sel_tiles % P.tiles_x == 0;
}

// Logical packets of a traversal launch (with tile_block, padded to whole blocks).  Host side:
// the device reads G.packets.
RT_HD inline int trace_packets(const RenderParams& P) {
  if (!P.tile_block) return P.num_sel_tiles;
  const int tiles_y = P.num_sel_tiles / P.tiles_x;
  return ((P.tiles_x + kBlockW - 1) / kBlockW) * ((tiles_y + kBlockH - 1) / kBlockH) * kTraceWaves;
}

// The PacketGeom of P's tiles_x, num_sel_tiles, tile_block and order_regions, and of its camera
// and culling-tree root box (neg_t_exp).
RT_HD inline PacketGeom packet_geom(const RenderParams& P) {
  PacketGeom g;
  g.block_nbx = (P.tiles_x + kBlockW - 1) / kBlockW;
  g.by_tiles_x = div_magic(P.tiles_x);
  g.by_deal_nbx = div_magic(deal_blocks_x(P.tiles_x));
  g.by_block_nbx = div_magic(g.block_nbx);
  g.by_regions = div_magic(P.order_regions);
  g.sel_rows = P.tiles_x > 0 ? P.num_sel_tiles / P.tiles_x : 0;
  g.packets = P.tiles_x > 0 ? trace_packets(P) : 0;
  g.neg_t_exp = P.accel_root >= 0 ? -visit_time_exp(P.accel_box, P.cam_e) : 0;
  return g;
}

// Tile (= sel, tile_step 1) of logical packet p; -1 for a padding packet of an edge block.
// With P.tile_block the workgroup's packets form a kBlockW x kBlockH block of tiles (blocks
// row-major over the frame) instead of a run along a tile row.
RT_HD inline int packet_sel(const RenderParams& P, const PacketGeom& G, int p) {
  if (!P.tile_block) return p;
  const int w = p % kTraceWaves, b = p / kTraceWaves;
  const int by = div_by(b, G.by_block_nbx), bx = b - by * G.block_nbx;
  const int tx = bx * kBlockW + w % kBlockW, ty = by * kBlockH + w / kBlockW;
  return (tx < P.tiles_x && ty < G.sel_rows) ? ty * P.tiles_x + tx : -1;
}

// Unit u = the kTraceWaves packets of logical packets u*kTraceWaves .. (a 2x2 tile block in
// tile_block mode).  Wave w's selected tile, or -1.
RT_HD inline int unit_sel(const RenderParams& P, const PacketGeom& G, int unit, int w) {
  const int p = unit * kTraceWaves + w;
  if (p >= G.packets) return -1;
  const int sel = packet_sel(P, G, p);
  return sel < P.num_sel_tiles ? sel : -1;
}

// Ordered dispatch: workgroup b takes entry b / regions of region b mod regions' list.
RT_HD inline int order_slot(const RenderParams& P, const PacketGeom& G, int b) {
  const int i = div_by(b, G.by_regions);
  return (b - i * P.order_regions) * P.order_stride + i;
}

// Tile column and row of selected tile `sel` (deal_block_tile's, or tile % and / tiles_x).
RT_HD inline void sel_tile(const RenderParams& P, const PacketGeom& G, int sel, int& tx,
                          int& ty) {
  if (P.block_deal) {  // selected block sel / 4, its tile sel % 4
    const int d = P.tile_begin + (sel >> 2) * P.tile_step, w = sel & 3;
    const int nbx = deal_blocks_x(P.tiles_x), by = div_by(d, G.by_deal_nbx);
    int bx = d - by * nbx + (by - div_by(by, G.by_deal_nbx) * nbx);
    if (bx >= nbx) bx -= nbx;
    tx = 2 * bx + (w & 1);
    ty = 2 * by + (w >> 1);
  } else {
    const int tile = P.tile_begin + sel * P.tile_step;
    ty = div_by(tile, G.by_tiles_x);
    tx = tile - ty * P.tiles_x;
  }
}

// Ray queries (rt_trace_rays_device / rt_occluded_device): one launch over rays
// [0, n) of `rays` (rt_ray, two 16-B words each).  Wave w traces rays perm[64 w .. 64 w + 63]
// (perm == nullptr: the identity) and writes result slot perm[i]: an rt_ray_hit (closest hit) or
// one byte (occlusion).
// The reorder key (rt_kernels.hip query_key): 3 bits of cube face, kQueryOriginBits per axis of
// origin cell, kQueryDirBits per face axis of direction — 20 bits, at most 2^20 bins.
#ifndef RT_QUERY_ORIGIN_BITS  // (A/B builds: 2 = a 4x4x4 origin grid and 64x64 direction cells)
#define RT_QUERY_ORIGIN_BITS 1
#endif
constexpr int kQueryOriginBits = RT_QUERY_ORIGIN_BITS;
constexpr int kQueryDirBits = (18 - 3 * kQueryOriginBits) / 2;
constexpr int kQueryKeyBits = 3 + 3 * kQueryOriginBits + 2 * kQueryDirBits;
static_assert(kQueryOriginBits >= 1 && kQueryDirBits >= 1 && kQueryDirBits <= 8 &&
              kQueryKeyBits <= 21, "reorder key layout");
constexpr int kQueryMinBinBits = 11;  // ... and at least one scan chunk
constexpr int kQueryScanChunk = 1 << kQueryMinBinBits;  // bins one scan workgroup takes
constexpr long long kQueryMaxLaunch = 1ll << 28;        // rays per launch (32-bit perm entries)
struct QueryParams {
  const void* rays;
  void* out;
  const int* perm;
  const int* leaf_object;  // per DFS leaf: its index in the object lists
  long long n;
  // RT_QUERY_REORDER: the key's origin cell = (o - box_lo) * box_scale (0..1 across the scene
  // box) times the cells per axis, clamped; `bins` = 2^(kQueryKeyBits - shift) counters in
  // hist, one total per scan chunk in totals
  float box_lo[3], box_scale[3];
  int shift, bins;
  unsigned* hist;
  unsigned* totals;
  int* perm_out;
};
// words of reorder scratch for a launch of n rays: perm, then hist, then totals
constexpr int query_bin_bits(long long n) {
  int b = kQueryMinBinBits;
  while (b < kQueryKeyBits && (1ll << b) < n) b++;
  return b;
}
constexpr size_t query_scratch_words(long long n) {
  return (size_t)n + (size_t(1) << query_bin_bits(n)) + (size_t(1) << (kQueryKeyBits - kQueryMinBinBits));
}


// Radiance queries (rt_shade_rays_device): one launch traces the rays
// [first, Q.n) of the order in use — one chunk of the batch — from (o, d, in_medium, depth).
// A recursing launch keeps its ray-tree frames in `frames`: (depth + 1) levels of
// kRadianceFrameFloats fields of `lanes` floats, a lane's slot being its index within the chunk.
constexpr int kRadianceFrameFloats = 28;         // rt_kernels.hip kFrFields
constexpr long long kRadianceChunkUnit = 64;     // chunks are whole waves
struct RadianceParams {
  float* frames;  // nullptr: the launch cannot recurse (depth 0, or no mirror / glass material)
  long long first;
  long long lanes;
  int depth;      // the reference's current_recursion_depth of every ray
  int in_medium;  // RT_QUERY_IN_MEDIUM
};
// bytes of frame scratch one ray needs at `depth`
constexpr size_t radiance_frame_bytes(int depth) {
  return sizeof(float) * kRadianceFrameFloats * (size_t)(depth + 1);
}

// The caller's light records of a lit radiance query (rt_shade_rays_lit_device; DESIGN.md
// §4.14): ray i of the caller's batch owns records [i k, i k + k) of `lights` (rt_light_sample,
// 48 B each); shared: every ray owns [0, k).  LitArg<LIT> is what the radiance kernel takes:
// nothing in the instantiations without light records.
constexpr int kLitMaxPerRay = 256;
constexpr int kLitMaxShared = 65535;
struct LitParams {
  const void* lights;
  int k;
  int shared;
};
template <bool LIT>
struct LitArg {};
template <>
struct LitArg<true> : LitParams {};

// Surface data (rt_scene_create_surface), found by DFS leaf and by vertex id.
// A scene has `tri` when a mesh is smooth or it has uv, `normals` when a mesh is smooth, `uv` when
// the caller gave texture coordinates; a scene with none of them has all three null.
// SurfArg<SMOOTH> is what the ray-tree and closest-hit code takes: empty in the flat
// instantiations, whose kernels take no surface argument at all (rt_kernels.hip surf_of), so their
// code is that of a build without surface data.
constexpr int kSurfSmooth = 1;  // leaf flag: a face of a smooth mesh
struct SurfParams {
  const int* tri;        // int4 per DFS leaf: i0 i1 i2 flags; a sphere: zeros
  const float* normals;  // float4 per vertex: the vertex normal, 0
  const float* uv;       // float2 per vertex
  int num_leaves;        // rt_hit_attributes' bound on rt_ray_hit::leaf
};
template <bool SMOOTH>
struct SurfArg {};
template <>
struct SurfArg<true> : SurfParams {};

// Image textures (rt_scene_create_textured).  A textured scene always has the
// per-leaf record of SurfParams::tri; a leaf's texture id + 1 sits in its flags word above the
// smooth bit (0: no texture), on sphere leaves too.  The texels of every texture lie in one blob,
// 4 bytes per texel (R, G, B in the low three bytes), rows of `w` texels, top row first.
// TexArg<TEX> is what the ray-tree code takes beside SurfArg<true>: nothing in the other
// instantiations.
constexpr int kSurfTexShift = 1;  // leaf flags >> kSurfTexShift: texture id + 1
enum : int32_t { kTexNearest = 0, kTexBilinear = 1 };                     // RT_TEX_NEAREST ...
enum : int32_t { kTexReplaceKd = 0, kTexBlendKd = 1, kTexReplaceAll = 2 };  // RT_TEX_REPLACE_KD ...
enum : int32_t { kTexRepeat = 0, kTexClamp = 1 };                         // RT_TEX_REPEAT ...
constexpr int kTexMaxSide = 16384;
struct alignas(16) DevTexture {
  uint32_t offset;  // of its first texel in the blob
  int32_t w, h;
  int32_t interpolation, decal, appearance;
  float normalizer;
  int32_t pad;
};
static_assert(sizeof(DevTexture) == 32, "texture record is two 16-byte words");
struct TexParams {
  const DevTexture* table;
  const uint32_t* texels;
  int num_textures;
  int blank_material;  // a material the host appends: no mirror, no transparency (REPLACE_ALL hits)
};
template <bool TEX>
struct TexArg {};
template <>
struct TexArg<true> : TexParams {};

// Texture::get_color_at(u, v) (HW4/src/Texture.cpp:57-134) restated line for line: raw channel
// values 0..255 as floats.  All fp32, every product and sum rounded (every file that includes this
// compiles with contraction off); fmin / fmax return the operand that is not NaN, so a NaN
// coordinate becomes 1.  One departure: a term of the clamped bilinear form whose linear texel
// index lies at or past w * h — where the reference reads past its buffer — is skipped.  One
// definition for the device's ray trees and lookups and the host's lookup.
RT_HD inline void tex_get_color(const DevTexture& T, const uint32_t* texels, float u, float v,
                                float rgb[3]) {
  if (T.appearance == kTexClamp) {  // :58-60
    u = __builtin_fmaxf(0.0f, __builtin_fminf(1.0f, u));
    v = __builtin_fmaxf(0.0f, __builtin_fminf(1.0f, v));
  } else {  // :62-63
    u = __builtin_fmaxf(0.0f, __builtin_fminf(1.0f, u - __builtin_floorf(u)));
    v = __builtin_fmaxf(0.0f, __builtin_fminf(1.0f, v - __builtin_floorf(v)));
  }
  const float fw = (float)T.w, fh = (float)T.h;
  u = u * fw;  // :65-68
  if (u >= fw) u = u - 1.0f;
  v = v * fh;
  if (v >= fh) v = v - 1.0f;
  const uint32_t w = (uint32_t)T.w, h = (uint32_t)T.h;
  const uint32_t* tx = texels + T.offset;
  auto channel = [](uint32_t texel, int c) { return (float)((texel >> (8 * c)) & 255u); };
  if (T.interpolation == kTexNearest) {  // :71-74
    const uint32_t t = tx[w * (uint32_t)v + (uint32_t)u];
    for (int c = 0; c < 3; c++) rgb[c] = channel(t, c);
    return;
  }
  if (T.appearance == kTexRepeat) {  // :77-100
    const uint32_t p = (uint32_t)u % w, pn = (p + 1) % w;
    const uint32_t q = (uint32_t)v % h, qn = (q + 1) % h;
    const float dx = u - (float)p, dy = v - (float)q;
    const uint32_t t00 = tx[w * q + p], t10 = tx[w * q + pn], t11 = tx[w * qn + pn],
                   t01 = tx[w * qn + p];
    for (int c = 0; c < 3; c++) {
      float x = channel(t00, c) * (1.0f - dx) * (1.0f - dy);
      x += channel(t10, c) * dx * (1.0f - dy);
      x += channel(t11, c) * dx * dy;
      x += channel(t01, c) * (1.0f - dx) * dy;
      rgb[c] = x;
    }
    return;
  }
  // :102-129: the reference's guards, texels by linear index
  const uint32_t p = (uint32_t)u, pn = p + 1, q = (uint32_t)v, qn = (uint32_t)(v + 1.0f);
  const float dx = u - (float)p, dy = v - (float)q;
  const uint32_t count = w * h;
  const bool g10 = pn < w, g11 = qn < h && w * qn + pn < count, g01 = pn < w && qn < h;
  const uint32_t t00 = tx[w * q + p];
  const uint32_t t10 = g10 ? tx[w * q + pn] : 0u;
  const uint32_t t11 = g11 ? tx[w * qn + pn] : 0u;
  const uint32_t t01 = g01 ? tx[w * qn + p] : 0u;
  for (int c = 0; c < 3; c++) {
    float x = channel(t00, c) * (1.0f - dx) * (1.0f - dy);
    if (g10) x += channel(t10, c) * dx * (1.0f - dy);
    if (g11) x += channel(t11, c) * dx * dy;
    if (g01) x += channel(t01, c) * (1.0f - dx) * dy;
    rgb[c] = x;
  }
}

// rt_texture_lookup*: q holds n rt_tex_query records (16 B), rgb 3 n floats.
struct TexLookupParams {
  const void* q;
  float* rgb;
  long long n;
};

// Instanced scenes (rt_scene_create_instanced).  The top-level reference tree
// (top_nodes, DevNode records whose leaf children are ~top-level DFS position) holds the
// instances and the loose primitives; top_prims[pos] is the loose primitive at that position, or
// for an instance a record of kind kPrimInstance whose `material` is the instance index.  Each
// base mesh is a scene of its own (DevMesh: the fields of RenderParams a walk reads), entered with
// the ray taken through the instance's inverse matrix.  The instance kernels take InstParams as
// an argument of their own; no other kernel's argument list changes.
constexpr int32_t kPrimInstance = 2;
struct alignas(16) DevInstance {
  float inv[12];  // rows 0..2 of the inverse matrix, four columns each
  float box[6];   // Bounding_box::apply_transform of the base mesh's root box
  int32_t mesh, material;
  int32_t moving;  // a scene with motion (below): the instance has a velocity; else 0
  int32_t pad[3];
};
static_assert(sizeof(DevInstance) == 96, "instance record is six 16-byte words");
struct alignas(16) DevMesh {
  const DevNode* nodes;
  const DevLeaf* leaves;
  const DevPrim* prims;
  const DevAncestry* anc;
  const float* normals;    // float4 per mesh leaf
  const int* leaf_object;  // per mesh leaf: the face's index within the mesh
  int32_t root_kind, root_ref, accel_root, accel_stride;  // accel_root < 0: no culling tree
  float root_box[6];
  float accel_box[6];
  int32_t quot_ok;
  int32_t leaf_base;    // scene-wide leaf id of the mesh's leaf 0
  int32_t object_base;  // object-list index of the mesh's face 0
  int32_t pad;
};
static_assert(sizeof(DevMesh) == 128, "mesh record is two 64-byte scalar loads");
enum : int32_t { kTopNode = 0, kTopSingle = 1 };
struct InstParams {
  const DevNode* top_nodes;
  const DevPrim* top_prims;
  const float* top_normals;  // float4 per top-level position (loose triangles: the flat normal)
  const int* top_info;       // int2 per top-level position: object index, scene-wide leaf id
  const DevInstance* instances;
  const DevMesh* meshes;
  int top_root_kind;         // kTopNode, or kTopSingle: the list is the one object at position 0
  int top_quot_ok;           // quot_coord_ok of every loose triangle's v0
  float top_box[6];
};

// Scenes with motion (rt_scene_create_moving).  A ray carries a time tau; an
// instance or sphere with a velocity v is met through the inverse of A = T(tau v) * M, built per
// ray by motion_inverse below.  What a moving object needs beyond its 96-byte DevInstance sits in
// tables of their own, read only on the moving branch.  A sphere with a matrix other than the
// identity, or with a velocity, is a top-level kind of its own: kPrimMovingSphere, its DevPrim's
// `material` the index of its DevMotionSphere.  The motion kernels take MotionParams as one more
// argument; no other kernel's argument list changes.
constexpr int32_t kPrimMovingSphere = 3;
struct alignas(16) DevMotionInstance {
  float fwd[16];  // M, row-major (object -> world)
  float vel[3];
  int32_t pad;
};
static_assert(sizeof(DevMotionInstance) == 80, "");
struct alignas(16) DevMotionSphere {
  float fwd[16];  // M
  float inv[12];  // rows 0..2 of Mat4::inverse(M): the walk's matrix when the sphere does not move
  float vel[3];
  int32_t moving;  // vel != 0
  float center[3];
  float radius;
  int32_t material;
  int32_t pad[3];
};
static_assert(sizeof(DevMotionSphere) == 160, "");
struct MotionParams {
  const DevMotionInstance* instances;  // per instance
  const DevMotionSphere* spheres;      // per kPrimMovingSphere record
  int fast;      // the base meshes that have a culling tree are walked through it
  int ray_time;  // RT_QUERY_RAY_TIME: the rays' fourth direction word is their time, else 0
};

// Rows 0..2 of the inverse of T(tau * vel) * fwd, in the reference's order (HW3 Mesh.h:77-82,
// Sphere.h:114-119): delta = tau * vel per component; Matrix4x4::operator* with T(delta) written
// out, every result[i][j] from 0 through its four products, the ones with 0 and 1 included (they
// turn a -0 entry into +0); then Matrix4x4::invert_matrix as Mat4::inverse restates it (mat4.h),
// but only the twelve cofactors of rows 0..2 and the one that completes the determinant.  One
// definition for the device's walk and the host's checks; every file that includes this compiles
// with contraction off.  det == 0: twelve NaNs and false (the object is missed: a NaN local ray
// is no valid ray).
RT_HD inline bool motion_inverse(const float* fwd, const float* vel, float tau, float* inv) {
  const float delta[3] = {tau * vel[0], tau * vel[1], tau * vel[2]};
  float m[16];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float acc = 0.0f;
      for (int k = 0; k < 4; k++) {
        const float tik = k == 3 ? (i < 3 ? delta[i] : 1.0f) : (i == k ? 1.0f : 0.0f);
        acc += tik * fwd[4 * k + j];
      }
      m[4 * i + j] = acc;
    }
  float c[13];
  c[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] +
         m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  c[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] -
         m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  c[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] +
         m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  c[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] -
          m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  c[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] -
         m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  c[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] +
         m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  c[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] -
         m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  c[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] +
         m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  c[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] -
         m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  c[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] +
          m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  c[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] -
         m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  c[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] +
         m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  c[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] -
          m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  float det = m[0] * c[0] + m[1] * c[4] + m[2] * c[8] + m[3] * c[12];
  if (det == 0.0f) {
    for (int k = 0; k < 12; k++) inv[k] = __builtin_nanf("");
    return false;
  }
  det = 1.0f / det;
  for (int k = 0; k < 12; k++) inv[k] = c[k] * det;
  return true;
}

// rt_hit_attributes*: rays, hits and attr hold n records each.
struct AttrParams {
  const void* rays;
  const void* hits;
  void* attr;
  long long n;
};

#if defined(__HIPCC__)
// The reference's splat weight (HW2/Scene.cpp:12-14): double exp of a float argument, double
// division, narrowed.  One definition for the MSAA resolve (rt_kernels.hip) and the films
// (film_kernels.hip); both files compile with contraction off.
__device__ __forceinline__ float gaussian_filter(float x, float y, float sigma) {
  return (float)(exp((double)(-(x * x + y * y) / (2 * sigma * sigma))) /
                 (2 * M_PI * (double)sigma));
}
#endif

// Films (rt_film_*): one splat call over samples [0, n).  A sample is a film
// position xy[i] and the rgb of rad[i]; its source pixel is (floor x, floor y), and it is valid
// iff 0 <= x < width and 0 <= y < height (and, in the fused entry, rays[i] is a valid query ray).
// The call sorts the valid samples by (source pixel, index) — count per pixel, scan, scatter
// through cursors, order every list — and then one lane per destination pixel adds the samples
// of its 3x3 neighbourhood's lists in that order.
constexpr long long kFilmMaxSamples = 1ll << 28;  // per call (32-bit list entries and offsets)
constexpr int kFilmMaxSide = 32768;               // (float)width is exact, width * height < 2^31
constexpr int kFilmScanChunk = 2048;              // counters one scan workgroup takes
constexpr int kFilmShortList = 64;                // longer lists are sorted by a workgroup each
enum : int { kFilmGaussian = 0, kFilmBox = 1 };
enum : int { kFilmBin = 0, kFilmScan, kFilmScatter, kFilmOrder, kFilmGather, kFilmStages };
struct FilmParams {
  float* pixels;               // width * height Pixels: color[3], weight
  unsigned long long* counts;  // samples added, samples dropped
  const float* xy;             // n x 2
  const void* rad;             // n rt_radiance (t ignored)
  const void* rays;            // fused entry: n rt_ray, an invalid ray's sample is dropped; or null
  long long n;
  int width, height, filter;
  float sigma;
  // per-call scratch, film_scratch_words(width * height, n) words:
  unsigned* offs;   // per pixel: its count, then (scan) its list's start, then (scatter) its end
  unsigned* sums;   // the scan's chunk totals, film_scan_words(width * height)
  unsigned* list;   // n sample indices grouped by source pixel
  unsigned* longs;  // [0]: the number of lists longer than kFilmShortList, then their pixels
};
// words the scan of `bins` counters keeps beside them: one total per chunk, level by level
constexpr size_t film_scan_words(size_t bins) {
  size_t words = 0;
  while (true) {
    bins = (bins + kFilmScanChunk - 1) / kFilmScanChunk;
    words += bins;
    if (bins <= 1) return words;
  }
}
constexpr size_t film_long_words(long long n) { return (size_t)(n / (kFilmShortList + 1)) + 2; }
constexpr size_t film_scratch_words(size_t pixels, long long n) {
  return pixels + film_scan_words(pixels) + (size_t)n + film_long_words(n);
}

}  // namespace rt

#endif
