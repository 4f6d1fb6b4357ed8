// MI355X (gfx950) render kernels: HW2's Scene::render_image -> trace_ray -> BVH::intersect ->
// Triangle/Sphere::intersect -> Point_light shading + shadow rays.
//
// Execution model:
//   * one wavefront = one 8x8 pixel packet; 4 packets per 256-thread workgroup;
//   * the wave walks the BVH TOGETHER: the current node index and the 64-bit lane mask of
//     the rays that accepted every box on the path are wave-uniform (SGPRs), so node and
//     primitive records come in through the scalar cache (s_load) once per wave, not once
//     per lane;
//   * the traversal stack is one entry per VGPR lane (lane-select push, v_readlane pop, 64 deep);
//     trees deeper than that use a per-wave LDS stack (kDeepStack entries);
//   * per-lane masks reproduce the reference's per-ray semantics exactly: a ray tests a node
//     iff it accepted every ancestor's box (HW2/Bounding_volume_hierarchy.cpp:31-55);
//   * closest hit = lexicographic minimum of (t, DFS leaf index) over accepted leaves, which
//     is what the reference's left-first recursion with strict `<` returns (appendix A.5), so
//     any visiting order gives the reference's answer;
//   * leaf tests are queued per wave in LDS and run 64 at a time, one (ray, leaf) pair per lane.
//
// Numerics: compiled with -ffp-contract=off and this file's pragma; '/' is the correctly
// rounded fp32 division and sqrtf is correctly rounded on gfx950 (HIP defaults), pow / exp
// / log are the fp64 ocml functions, matching the reference's double libm islands.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "rt_internal.h"

#pragma clang fp contract(off)

namespace rt {

#define RT_INF __builtin_huge_valf()
constexpr float kEps = 0.000001f;  // HW2/Vector3.h:7 kEpsilon

constexpr int kCounterSlots = kCounterRows;

#ifdef RT_DIAG
#define DIAG(stmt) stmt
#else
#define DIAG(stmt)
#endif
struct Diag {  // per-wave traversal work (RT_DIAG builds)
  unsigned long long nodes = 0, node_lanes = 0, leaves = 0, leaf_lanes = 0, wide = 0, guard = 0;
  // per-phase attribution (rt_debug_phases): events of the visit loop, and shader-clock cycles
  // (s_memrealtime, 100 MHz) of this wave spent in its phases
  unsigned long long ev[kPhaseEvents] = {};
  unsigned long long cyc_visit = 0, cyc_load = 0, cyc_flush = 0;
  unsigned long long carry[3] = {};  // mid-walk flushes that carried 0 / 1-16 / 48-63 entries
  unsigned long long defer[kDeferEvents] = {};  // the deferred guard's kDf* counts
  unsigned long long oct_packets = 0, oct_walks = 0;  // octant_walks: loops entered, sub-walks
  unsigned long long cyc_setup = 0, cyc_walk = 0, cyc_tail = 0;  // outside / inside the walks
};
#ifdef RT_DIAG
// [0, kPhaseEvents): primary events, [kPhaseEvents, 2 kPhaseEvents): shadow events, then the
// cycle counters (kPhCyc*)
__device__ unsigned long long g_phase[kPhaseSlots];
__device__ __forceinline__ unsigned long long clock_now() {
  unsigned long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  return t;
}
#endif

// Packets (8x8 tiles, one wave each) per traversal workgroup.  Two: a workgroup's LDS (leaf
// queues, ~5.6 KiB per wave, which like the VGPRs caps a CU at 28 waves) stays allocated until
// its slowest wave ends, so the finished waves of a 4-wave workgroup hold slots a new workgroup
// cannot use; with two, half as much sits idle behind a heavy packet (C3: frame 0.335 -> 0.327
// ms with six in flight, a 1/8 band 0.047 -> 0.045 ms; profiles/r06/ab_trace_waves.json).
// (A/B builds: RT_TRACE_WAVES 1, 2 or 4; kTraceWaves is rt_internal.h's.)
// A split tile's quadrants take kSplitEntries workgroups of kTraceWaves waves.
constexpr int kQuadrants = 4, kSplitEntries = kQuadrants / kTraceWaves;

// ------------------------------------------------------------------ vector helpers
struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 v3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x) + (a.y * b.y) + (a.z * b.z); }
__device__ __forceinline__ float length(V3 a) { return __builtin_sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ V3 normalize(V3 a) { return a / length(a); }
__device__ __forceinline__ V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ bool finite3(V3 a) {  // (a NaN fails the compares)
  return (__builtin_fabsf(a.x) < RT_INF) & (__builtin_fabsf(a.y) < RT_INF) &
         (__builtin_fabsf(a.z) < RT_INF);
}

struct LaneRay {
  V3 o, d;
  V3 r;       // v_rcp_f32 reciprocals (<= 1 ulp): the approximate slab test only
  V3 m;       // 2^-18 |o| / d per axis: the ray's share of the culling margin (visit_wide)
  // The COHERENT visit's r and m, in scaled time t' = t 2^-E: r 2^-E and m 2^-E (coherent_ray;
  // nobody else reads them, and make_ray leaves them unset) — DESIGN.md §4.2.
  V3 vr, vm;
  bool skip0, skip1, skip2;  // |d_i| < 1e-6: axis ignored (HW2/bounding_box.cpp:21)
  bool quot;  // origin and scene in the shared-reciprocal range (tri_quotients)
  int sh0, sh1, sh2;  // 16 where 1/d_i < 0 (the slot's hi plane is the entry plane), else 0
};

__device__ __forceinline__ bool quot_coord(float x) {  // quot_coord_ok of rt_internal.h
  const float a = __builtin_fabsf(x);
  return a == 0.0f || (a >= 0x1p-26f && a <= 0x1p48f);
}

__device__ __forceinline__ LaneRay make_ray(V3 o, V3 d, int scene_quot_ok) {
  LaneRay r;
  r.o = o;
  r.d = d;
  r.r = v3(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
  r.m = v3(0x1p-18f * __builtin_fabsf(o.x) * r.r.x, 0x1p-18f * __builtin_fabsf(o.y) * r.r.y,
           0x1p-18f * __builtin_fabsf(o.z) * r.r.z);
  r.skip0 = __builtin_fabsf(d.x) < kEps;
  r.skip1 = __builtin_fabsf(d.y) < kEps;
  r.skip2 = __builtin_fabsf(d.z) < kEps;
  r.quot = scene_quot_ok && quot_coord(o.x) && quot_coord(o.y) && quot_coord(o.z);
  r.sh0 = (int)((__float_as_uint(r.r.x) >> 27) & 16u);
  r.sh1 = (int)((__float_as_uint(r.r.y) >> 27) & 16u);
  r.sh2 = (int)((__float_as_uint(r.r.z) >> 27) & 16u);
  return r;
}

// The frame kernel's packets: the COHERENT visit's constants of `r`, in the launch's scaled time
// (neg_e = -E, PacketGeom::neg_t_exp, wave-uniform).  The scaling is by a power of two, so every
// product and sum of the visit is 2^-E times what it would be at E = 0, bit for bit, while nothing
// is subnormal (E is kept where the reciprocal of a tested axis stays normal, visit_time_exp; a
// subnormal plane distance is below 2^(E-126) in t, far inside the margin), and the compares do
// not change.  r, m, o and d stay as they are for every other reader: the root box's test has an
// absolute term in its band, and the leaf batch rebuilds its reciprocals from d.
__device__ __forceinline__ void coherent_ray(LaneRay& r, int neg_e) {
  r.vr = v3(__builtin_amdgcn_ldexpf(r.r.x, neg_e), __builtin_amdgcn_ldexpf(r.r.y, neg_e),
            __builtin_amdgcn_ldexpf(r.r.z, neg_e));
  r.vm = v3(__builtin_amdgcn_ldexpf(r.m.x, neg_e), __builtin_amdgcn_ldexpf(r.m.y, neg_e),
            __builtin_amdgcn_ldexpf(r.m.z, neg_e));
}

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }
__device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
// This lane's bit of a wave-uniform mask, as the exec mask itself (s_and_saveexec) — written as
// (m >> lane) & 1 the compiler keeps a 64-bit 1 << lane per lane (two VGPRs, spilled in the
// traversal kernels) and tests it with v_and + v_cmp_u64 at every queue push.
__device__ __forceinline__ bool lane_in(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// Lane masks of one fp32 compare, straight from the v_cmp (ballot of a combined boolean makes
// the compiler round-trip it through a VGPR: v_cndmask + v_cmp per mask).  LLVM FCmp
// predicates; ordered, so NaN gives false as the C++ operators do.
enum : int { kFcmpOGT = 2, kFcmpOGE = 3, kFcmpOLT = 4 };
__device__ __forceinline__ uint64_t lanes_gt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOGT); }
__device__ __forceinline__ uint64_t lanes_ge(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOGE); }
__device__ __forceinline__ uint64_t lanes_lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOLT); }
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
// v_writelane_b32 (the LLVM intrinsic; clang has no builtin for it): `old` with lane `lane`
// (wave-uniform) replaced by the wave-uniform `v`.  Ignores EXEC.
__device__ int writelane(int v, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// ------------------------------------------------------------------ slab test
// Literal HW2/bounding_box.cpp:15-35 + the caller's reject rule (BVH.cpp:32-35).  Used when
// the fast test below cannot decide.  Its comparisons are the reference's, so NaN / inf
// inputs behave as there.
__device__ __forceinline__ bool box_exact(const float* b, const LaneRay& r) {
  float tmin = -RT_INF, tmax = RT_INF;
  const float o[3] = {r.o.x, r.o.y, r.o.z};
  const float d[3] = {r.d.x, r.d.y, r.d.z};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if (__builtin_fabsf(d[i]) < kEps) continue;
    float t0 = (b[i] - o[i]) / d[i];
    float t1 = (b[i + 3] - o[i]) / d[i];
    if (d[i] < 0) {
      const float s = t0;
      t0 = t1;
      t1 = s;
    }
    if (t0 > tmin) tmin = t0;
    if (t1 < tmax) tmax = t1;
    if (tmin > tmax) return false;
  }
  const float bt = tmin > 0.0f ? tmin : tmax;
  return !(bt < 0.0f || bt == RT_INF);
}

#ifdef RT_DIAG
__device__ unsigned long long g_exact_fallbacks;  // lanes that needed box_exact
#endif

// Fast slab test.  With q = RN(RN(m - o) / d) the reference's quotient and q' = RN(RN(m - o)
// * rcp(d)) ours, |q' - q| <= 2^-22 |q| and sign(q') == sign(q) exactly.  The reference
// accepts iff tmin <= tmax and tmax >= 0 (tmin, tmax finite here): the sign test is exact, and
// the order test is decided here only outside a 2^-20 relative band; inside it the lane is
// flagged for box_exact.  tnear (approximate entry distance) only orders.
template <bool SKIP>
__device__ __forceinline__ void slab_span(const float* b, const LaneRay& r, float& tn, float& tf) {
  const float ax = (b[0] - r.o.x) * r.r.x, bx = (b[3] - r.o.x) * r.r.x;
  const float ay = (b[1] - r.o.y) * r.r.y, by = (b[4] - r.o.y) * r.r.y;
  const float az = (b[2] - r.o.z) * r.r.z, bz = (b[5] - r.o.z) * r.r.z;
  float nx = __builtin_fminf(ax, bx), fx = __builtin_fmaxf(ax, bx);
  float ny = __builtin_fminf(ay, by), fy = __builtin_fmaxf(ay, by);
  float nz = __builtin_fminf(az, bz), fz = __builtin_fmaxf(az, bz);
  if (SKIP) {
    nx = r.skip0 ? -RT_INF : nx;
    fx = r.skip0 ? RT_INF : fx;
    ny = r.skip1 ? -RT_INF : ny;
    fy = r.skip1 ? RT_INF : fy;
    nz = r.skip2 ? -RT_INF : nz;
    fz = r.skip2 ? RT_INF : fz;
  }
  tn = __builtin_fmaxf(__builtin_fmaxf(nx, ny), nz);
  tf = __builtin_fminf(__builtin_fminf(fx, fy), fz);
}

// sure_in: the reference accepts (tf >= 0, and tn <= tf decided outside a 2^-20 relative
// band); sure_out: it rejects.  Neither: box_exact decides (NaN lands here too).  The sign of
// each bound is exact (RN(b - o) * rcp(d) has the sign of the reference's quotient), and
// d = RN(tn - tf) is within 2^-24 of tn - tf, so a decided case keeps a true margin above
// 2^-21 relative.
__device__ __forceinline__ void decide_sure(float tn, float tf, bool& sure_in, bool& sure_out) {
  const float band = __builtin_fmaf(__builtin_fabsf(tn) + __builtin_fabsf(tf), 0x1p-20f, 0x1p-120f);
  const float d = tn - tf;
  sure_in = (d < -band) & (tf >= 0.0f);
  sure_out = (tf < 0.0f) | (d > band);
}

template <bool SKIP>
__device__ __forceinline__ void slab_fast(const float* b, const LaneRay& r, float& tn,
                                          bool& accept, bool& undecided) {
  float tf;
  slab_span<SKIP>(b, r, tn, tf);
  bool out;
  decide_sure(tn, tf, accept, out);
  undecided = !(accept | out);
}

// Culling-tree boxes (accel_build.cpp) contain every reference box below them.  If the
// reference test accepts a contained box, the exact t-intervals nest and every computed
// bound is within 2^-22 relative of its exact value, so the container is never `sure_out`
// (2^-20 band, same skipped axes): a culling node never drops a treelet the reference would
// enter.  Its test is therefore just !sure_out.
__device__ __forceinline__ bool decide_cull(float tn, float tf) {
  bool in, out;
  decide_sure(tn, tf, in, out);
  return !out;
}

// ------------------------------------------------------------------ primitives
// HW2/Triangle.cpp:35-65 with determinant() = Triangle.h:33-38, v0 - v1 / v0 - v2 precomputed
// on the host with the same fp32 rounding.
__device__ __forceinline__ float det3(V3 c1, V3 c2, V3 c3) {
  return c1.x * (c2.y * c3.z - c3.y * c2.z) + c2.x * (c3.y * c1.z - c1.y * c3.z) +
         c3.x * (c1.y * c2.z - c2.y * c1.z);
}

// Correctly rounded n / det for the three numerators with ONE reciprocal.  gfx950's IEEE
// division is v_div_scale (num, den), y = v_rcp, e = fma(-den, y, 1), y1 = fma(e, y, y),
// q = num * y1, r = fma(-den, q, num), q1 = fma(r, y1, q), r1 = fma(-den, q1, num),
// v_div_fmas(r1, y1, q1), v_div_fixup(q2, den, num).  When no operand is near the exponent
// limits, v_div_scale returns its operand unchanged with VCC = 0 and v_div_fmas is a plain
// fma, so the sequence below (which keeps v_div_fixup: it gives a zero numerator the sign
// num ^ den) yields the bits of `/`; only the reciprocal refinement y1 depends on det alone,
// and it is shared.  Range: 2^-40 <= |det| <= 2^40 is checked here; numerators are 0 or
// 2^-49 <= |n| <= 2^49 by r.quot (every v0 and origin coordinate is 0 or in [2^-26, 2^48]).
// Then |n / det| lies in [2^-89, 2^89], exponent differences stay below 96 and nothing is
// subnormal, so none of v_div_scale's scaling cases can arise.  Any other lane takes `/`.
__device__ __forceinline__ float quot_step(float n, float det, float y1) {
  const float q = n * y1;
  const float r = __builtin_fmaf(-det, q, n);
  const float q1 = __builtin_fmaf(r, y1, q);
  const float r1 = __builtin_fmaf(-det, q1, n);
  return __builtin_amdgcn_div_fixupf(__builtin_fmaf(r1, y1, q1), det, n);
}

__device__ __forceinline__ V3 tri_quotients(V3 n, float det, bool quot) {
  const float ad = __builtin_fabsf(det);
  if (quot && ad >= 0x1p-40f && ad <= 0x1p40f) {
    const float y = __builtin_amdgcn_rcpf(det);
    const float e = __builtin_fmaf(-det, y, 1.0f);
    const float y1 = __builtin_fmaf(e, y, y);
    return v3(quot_step(n.x, det, y1), quot_step(n.y, det, y1), quot_step(n.z, det, y1));
  }
  return n / det;
}

// The same sharing for the divisions outside the walks (round 13): the three quotients of a
// normalize by its length, and a light's six diffuse and specular terms by d2.  The operand
// range is tri_quotients': divisor in [2^-40, 2^40], numerators 0 or in [2^-49, 2^49]; the
// range is tested per vector here, and any lane outside it takes `/`.
__device__ __forceinline__ bool quot_divisor_ok(float d) {
  const float ad = __builtin_fabsf(d);
  return (ad >= 0x1p-40f) & (ad <= 0x1p40f);
}
__device__ __forceinline__ float refined_rcp(float d) {
  const float y = __builtin_amdgcn_rcpf(d);
  return __builtin_fmaf(__builtin_fmaf(-d, y, 1.0f), y, y);
}
// A normalize's components are at most its length (times 1 + 2^-22), so only the smallest
// magnitude is tested; a vector with a zero component takes `/`.
__device__ __forceinline__ bool normalize_in_range(V3 a, float len) {
  const float lo = __builtin_fminf(__builtin_fminf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)),
                                   __builtin_fabsf(a.z));
  return (lo >= 0x1p-49f) & quot_divisor_ok(len);
}
// Any three numerators: 2 * bits - 1 drops the sign and wraps a zero to the top, so one unsigned
// minimum tests "0 or >= 2^-49"; the maximum magnitude tests the upper end (and fails an inf).
__device__ __forceinline__ bool numerators_in_range(V3 n) {
  const unsigned ux = (__float_as_uint(n.x) << 1) - 1u, uy = (__float_as_uint(n.y) << 1) - 1u,
                 uz = (__float_as_uint(n.z) << 1) - 1u;
  const unsigned lo = min(min(ux, uy), uz);
  const float hi = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(n.x), __builtin_fabsf(n.y)),
                                   __builtin_fabsf(n.z));
  return (lo >= (0x27000000u << 1) - 1u) & (hi <= 0x1p49f);  // 0x27000000: 2^-49
}
// a / length(a).  dead: a lane whose result nobody reads counts as in range, so that it does not
// send its wave through the `/` path as well.
__device__ __forceinline__ V3 normalize_shared(V3 a, bool dead = false) {
  const float len = length(a);
  const bool in_range = normalize_in_range(a, len);
  if (dead | in_range) {
    const float y1 = refined_rcp(len);
    return v3(quot_step(a.x, len, y1), quot_step(a.y, len, y1), quot_step(a.z, len, y1));
  }
  return a / len;
}
__device__ __forceinline__ bool light_terms_in_range(V3 a, V3 b, float d2) {
  const bool da = numerators_in_range(a), db = numerators_in_range(b), dd = quot_divisor_ok(d2);
  return da & db & dd;
}
// a / d2 and b / d2
__device__ __forceinline__ void light_quotients(V3 a, V3 b, float d2, V3& qa, V3& qb) {
  if (light_terms_in_range(a, b, d2)) {
    const float y1 = refined_rcp(d2);
    qa = v3(quot_step(a.x, d2, y1), quot_step(a.y, d2, y1), quot_step(a.z, d2, y1));
    qb = v3(quot_step(b.x, d2, y1), quot_step(b.y, d2, y1), quot_step(b.z, d2, y1));
  } else {
    qa = a / d2;
    qb = b / d2;
  }
}

// Branch-free: every value is computed and the reference's early exits (Triangle.cpp:46-62)
// become one predicate with the same comparisons (a NaN fails them as there).  With det == 0
// the quotients are inf/NaN and unused.
__device__ __forceinline__ bool tri_test(V3 v0, V3 a1, V3 a2, const LaneRay& r, float& t) {
  const float det = det3(a1, a2, r.d);
  const V3 b = tri_quotients(v0 - r.o, det, r.quot);
  const float beta = det3(b, a2, r.d);
  const float gamma = det3(a1, b, r.d);
  const float tt = det3(a1, a2, b);
  t = tt;
  return (det != 0.0f) & !((beta < 0.0f) | (beta > 1.0f)) &
         !((gamma < 0.0f) | (beta + gamma > 1.0f)) & (tt > 0.0f);
}

// HW2/Sphere.h:26-52 — true for any real root, including a negative one.
__device__ __forceinline__ bool sphere_test(V3 c, float radius, const LaneRay& r, float& t) {
  const V3 co = r.o - c;
  const float a = dot(r.d, r.d);
  const float b = 2 * dot(r.d, co);
  const float cc = dot(co, co) - radius * radius;
  const float disc = b * b - 4 * a * cc;
  if (disc < -kEps) return false;
  if (disc < kEps) {
    t = -b / (2 * a);
  } else {
    const float sq = __builtin_sqrtf(disc);  // == (float)sqrt((double)disc)
    const float t1 = (-b + sq) / (2 * a);
    const float t2 = (-b - sq) / (2 * a);
    t = t2 < 0.0f ? t1 : t2;
  }
  return true;
}

// Shape::intersect of one leaf.  SPHERES == false: the scene has no spheres (host flag), so
// the sphere code is not compiled into the traversal loop.
template <bool SPHERES>
__device__ __forceinline__ bool leaf_test(const DevPrim* __restrict__ prims, int leaf,
                                          const LaneRay& r, float& t) {
  const DevPrim& p = prims[leaf];
  const V3 v0 = ld3(p.v0);
  if (!SPHERES || p.kind == kPrimTriangle) return tri_test(v0, ld3(p.a1), ld3(p.a2), r, t);
  return sphere_test(v0, p.a1[0], r, t);
}

// ------------------------------------------------------------------ surface data
// Where inside its triangle a ray hit: tri_test's beta and gamma
// (HW2/Triangle.cpp:51, 53), computed again after the walk from the winning leaf's record and the
// same ray by the same functions, shared-reciprocal quotients included — the same bits, as
// resolve_pixel re-derives t.
typedef float f4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void tri_barycentrics(const DevPrim& p, const LaneRay& r, float& beta,
                                                 float& gamma) {
  const V3 a1 = ld3(p.a1), a2 = ld3(p.a2);
  const float det = det3(a1, a2, r.d);
  const V3 b = tri_quotients(ld3(p.v0) - r.o, det, r.quot);
  beta = det3(b, a2, r.d);
  gamma = det3(a1, b, r.d);
}

// ((x0 * w) + (x1 * beta)) + (x2 * gamma) per component, w = (1 - beta) - gamma: every product and
// sum rounded (the file compiles without contraction).
__device__ __forceinline__ float bary_mix(float x0, float x1, float x2, float w, float beta,
                                          float gamma) {
  return ((x0 * w) + (x1 * beta)) + (x2 * gamma);
}

// Mesh_triangle.cpp:101-106: the interpolated vertex normal, normalised by a true division.
__device__ __forceinline__ V3 smooth_normal(const SurfParams& S, i4 tr, float beta, float gamma) {
  const f4* vn = reinterpret_cast<const f4*>(S.normals);
  const f4 n0 = vn[tr.x], n1 = vn[tr.y], n2 = vn[tr.z];
  const float w = (1.0f - beta) - gamma;
  const V3 N = v3(bary_mix(n0.x, n1.x, n2.x, w, beta, gamma), bary_mix(n0.y, n1.y, n2.y, w, beta, gamma),
                  bary_mix(n0.z, n1.z, n2.z, w, beta, gamma));
  return N / length(N);
}

// Hit_data::normal of a triangle leaf: `flat`, or on a face of a smooth mesh the normal above.
// Nothing in the flat instantiations.
template <bool SMOOTH>
__device__ __forceinline__ V3 triangle_normal(const SurfArg<SMOOTH>& S, const DevPrim& p, int leaf,
                                              const LaneRay& r, V3 flat) {
  if constexpr (SMOOTH) {
    const i4 tr = reinterpret_cast<const i4*>(S.tri)[leaf];
    if (tr.w & kSurfSmooth) {
      float beta, gamma;
      tri_barycentrics(p, r, beta, gamma);
      return smooth_normal(S, tr, beta, gamma);
    }
  }
  return flat;
}

// The kernels that read Hit_data::normal take the scene's surface data as a parameter pack: empty
// in the flat instantiations, whose argument list (and implicit-argument offsets) is then that of
// a build without surface data, and one SurfArg<true> in the SMOOTH ones.
__device__ __forceinline__ SurfArg<false> surf_of() { return {}; }
__device__ __forceinline__ const SurfArg<true>& surf_of(const SurfArg<true>& s) { return s; }
// ... and in the TEX ones a TexArg<true> after it.
__device__ __forceinline__ const SurfArg<true>& surf_of(const SurfArg<true>& s, const TexArg<true>&) {
  return s;
}
__device__ __forceinline__ TexArg<false> tex_of() { return {}; }
__device__ __forceinline__ TexArg<false> tex_of(const SurfArg<true>&) { return {}; }
__device__ __forceinline__ const TexArg<true>& tex_of(const SurfArg<true>&, const TexArg<true>& t) {
  return t;
}

// ------------------------------------------------------------------ textures
// Image textures.  Both functions are out of line, as phong_pow_f64 is: they
// run once per hit after the walk, and inlined into the 20 TEX instantiations ocml's fp64 acos and
// atan2 and the lookup's four cases would set those kernels' register budgets and build time.
typedef float f2 __attribute__((ext_vector_type(2)));

// Sphere.cpp:100-105: (u, v) of the point center + lc on a sphere of `radius`.
__device__ __attribute__((noinline)) f2 sphere_uv_f64(float lx, float ly, float lz, float radius) {
  const float theta = (float)acos((double)(ly / radius));
  const float phi = (float)atan2((double)lz, (double)lx);
  f2 uv;
  uv.x = (float)((M_PI - (double)phi) / (2 * M_PI));
  uv.y = (float)((double)theta / M_PI);
  return uv;
}

// Texture::get_color_at of texture `id` (in range: the host checked the leaf records): the raw
// colour, and in w the texture's decal mode.
__device__ __attribute__((noinline)) f4 tex_color(const DevTexture* __restrict__ table,
                                                  const uint32_t* __restrict__ texels, int id,
                                                  float u, float v) {
  const DevTexture T = table[id];
  float rgb[3];
  tex_get_color(T, texels, u, v, rgb);
  return (f4){rgb[0], rgb[1], rgb[2], __int_as_float(T.decal)};
}

// Hit_data of a hit on `leaf` in a textured scene: the normal as triangle_normal / the sphere rule
// give it, and HW4's texture step (HW4/src/Scene.cpp:154-170).  kd: the diffuse colour the light
// loops take — the material's, or on a textured leaf tex / normalizer (REPLACE_KD) or
// ((tex / normalizer) + kd) / 2 (BLEND_KD).  all: a REPLACE_ALL texture; kd is then the raw texel,
// the ray's whole colour.  One tri_barycentrics serves the smooth normal and the (u, v) of
// Mesh_triangle.cpp:107-111.
__device__ __forceinline__ void textured_hit(const SurfArg<true>& S, const TexArg<true>& X,
                                             const DevPrim& pr, int leaf, const LaneRay& r, V3 p,
                                             V3 flat, const DevMaterial* __restrict__ mats, V3& n,
                                             V3& kd, bool& all) {
  const i4 tr = reinterpret_cast<const i4*>(S.tri)[leaf];
  const int id = (tr.w >> kSurfTexShift) - 1;
  float u = 0.0f, v = 0.0f;
  if (pr.kind == kPrimTriangle) {
    n = flat;
    if ((tr.w & kSurfSmooth) || id >= 0) {
      float beta, gamma;
      tri_barycentrics(pr, r, beta, gamma);
      if (tr.w & kSurfSmooth) n = smooth_normal(S, tr, beta, gamma);
      if (id >= 0) {
        const f2* uv = reinterpret_cast<const f2*>(S.uv);
        const f2 a = uv[tr.x], b = uv[tr.y], c = uv[tr.z];
        u = (a.x + beta * (b.x - a.x)) + gamma * (c.x - a.x);
        v = (a.y + beta * (b.y - a.y)) + gamma * (c.y - a.y);
      }
    }
  } else {
    const V3 lc = p - ld3(pr.v0);
    n = normalize(lc);
    if (id >= 0) {
      const f2 s = sphere_uv_f64(lc.x, lc.y, lc.z, pr.a1[0]);
      u = s.x;
      v = s.y;
    }
  }
  kd = ld3(mats[pr.material].diffuse);
  all = false;
  if (id >= 0) {
    const f4 c = tex_color(X.table, X.texels, id, u, v);
    const V3 tex = v3(c.x, c.y, c.z);
    const int decal = __float_as_int(c.w);
    if (decal == kTexReplaceAll) {
      all = true;
      kd = tex;
    } else {
      const float nz = X.table[id].normalizer;
      const V3 tc = v3(tex.x / nz, tex.y / nz, tex.z / nz);
      kd = decal == kTexBlendKd ? (tc + kd) / 2.0f : tc;
    }
  }
}

// ------------------------------------------------------------------ traversal stack
// Wave-uniform (node, lane-mask) entries.  DEEP == false: entry i lives in VGPR lane i
// (v_writelane push / v_readlane pop, no memory traffic, 64 deep).  DEEP == true: a
// per-wave LDS array of kDeepStack entries for trees deeper than 64 levels (lane 0 writes,
// all lanes read the broadcast word; LDS ops of one wave complete in order).
constexpr int kDeepStack = 1024;
constexpr int kDeepWords = 3;  // node, mask lo, mask hi

template <bool DEEP>
struct WaveStack {
  int node = 0;
  unsigned mlo = 0, mhi = 0;
  int sp = 0;  // wave-uniform
  int* lds = nullptr;
  DIAG(unsigned long long pushes = 0; unsigned long long pops = 0;)

  __device__ __forceinline__ void push(int n, uint64_t m) {
    if (!DEEP) {
      // Lane sp takes the entry: three v_writelane_b32, the values in SGPRs and the lane select
      // in M0 (gfx9 allows a v_writelane one SGPR besides M0).  (Round 7: was a v_cmp and three
      // v_mov + v_cndmask, seven VALU)
      node = writelane(n, sp, node);
      mlo = (unsigned)writelane((int)(unsigned)m, sp, (int)mlo);
      mhi = (unsigned)writelane((int)(unsigned)(m >> 32), sp, (int)mhi);
    } else if (lane_id() == 0) {
      lds[kDeepWords * sp] = n;
      lds[kDeepWords * sp + 1] = (int)(unsigned)m;
      lds[kDeepWords * sp + 2] = (int)(unsigned)(m >> 32);
    }
    sp++;
    DIAG(pushes++);
  }
  __device__ __forceinline__ void pop(int& n, uint64_t& m) {
    sp--;
    DIAG(pops++);
    if (!DEEP) {
      n = __builtin_amdgcn_readlane(node, sp);
      m = (uint64_t)(unsigned)__builtin_amdgcn_readlane(mlo, sp) |
          ((uint64_t)(unsigned)__builtin_amdgcn_readlane(mhi, sp) << 32);
    } else {
      n = uniform(lds[kDeepWords * sp]);
      m = (uint64_t)(unsigned)uniform(lds[kDeepWords * sp + 1]) |
          ((uint64_t)(unsigned)uniform(lds[kDeepWords * sp + 2]) << 32);
    }
  }
  // Pop entries until one still has a lane of `alive`; false when the stack runs empty.
  __device__ __forceinline__ bool pop_live(int& n, uint64_t& m, uint64_t alive) {
    for (;;) {
      if (sp == 0) return false;
      pop(n, m);
      m &= alive;
      if (m) return true;
    }
  }
};

__device__ __forceinline__ bool child_box_exact(const DevNode& N, int c, const LaneRay& r) {
  const float b[6] = {N.lo[0][c], N.lo[1][c], N.lo[2][c], N.hi[0][c], N.hi[1][c], N.hi[2][c]};
  return box_exact(b, r);
}

// A leaf's guard that the fast test could not decide: the reference's literal test on the
// holder's box and on every enclosing reference box (the ancestry of BVH.cpp:31-55).
// child: a reference node index, or ~leaf (its holder's box first).
__device__ bool guard_exact(const RenderParams& P, int child, const LaneRay& r) {
  int v = child >= 0 ? child : P.anc[~child].leaf_parent;
  while (v >= 0) {
    if (!box_exact(P.anc[v].box, r)) return false;
    v = P.anc[v].parent;
  }
  return true;
}

// One packet visit of a reference node (RT_TRAVERSAL_REFERENCE, or a scene without culling
// tree), per child: a leaf child is tested by every lane in the node (leaves have no box; the
// slot holds a +-1e30 box that every normalised ray accepts); an inner child's box takes the
// reference's test (fast, else box_exact).  h0/h1: lanes that enter (inner) or test (leaf).
template <bool SKIP>
__device__ __forceinline__ void visit_node(const DevNode& N, const LaneRay& r, bool in, bool& h0,
                                           bool& h1, float& t0, float& t1) {
  const float b0[6] = {N.lo[0][0], N.lo[1][0], N.lo[2][0], N.hi[0][0], N.hi[1][0], N.hi[2][0]};
  const float b1[6] = {N.lo[0][1], N.lo[1][1], N.lo[2][1], N.hi[0][1], N.hi[1][1], N.hi[2][1]};
  float f0, f1;
  slab_span<SKIP>(b0, r, t0, f0);
  slab_span<SKIP>(b1, r, t1, f1);
  bool in0, out0, in1, out1;
  decide_sure(t0, f0, in0, out0);
  decide_sure(t1, f1, in1, out1);
  h0 = in & in0;
  h1 = in & in1;
  const bool u0 = in & !(in0 | out0);
  const bool u1 = in & !(in1 | out1);
  if (ballot(u0 | u1)) {
    if (u0) h0 = child_box_exact(N, 0, r);
    if (u1) h1 = child_box_exact(N, 1, r);
    DIAG(if (u0 | u1) atomicAdd(&g_exact_fallbacks, 1ull));
  }
}

// Pick the next node after a binary visit: near child first (judged by the first lane that
// enters both), the far one pushed; with neither, pop (masks restricted to `alive`).  Returns
// false when the traversal is over.
template <bool DEEP>
__device__ __forceinline__ bool advance(WaveStack<DEEP>& st, int c0, int c1, uint64_t m0,
                                        uint64_t m1, float t0, float t1, int& node, uint64_t& m,
                                        uint64_t alive) {
  if (m0 && m1) {
    const uint64_t both = m0 & m1;
    bool near1 = false;
    if (both) {
      const int f = __builtin_ctzll(both);
      const float f0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t0), f));
      const float f1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t1), f));
      near1 = f1 < f0;
    }
    if (near1) {
      st.push(c0, m0);
      node = c1;
      m = m1;
    } else {
      st.push(c1, m1);
      node = c0;
      m = m0;
    }
    return true;
  }
  if (m0 || m1) {
    node = m0 ? c0 : c1;
    m = m0 ? m0 : m1;
    return true;
  }
  return st.pop_live(node, m, alive);
}

// ------------------------------------------------------------------ batched leaf tests
// A packet reaches a leaf with only the few lanes whose rays pass over that triangle (C3:
// ~14 of 64), so testing leaves one at a time runs the triangle test at ~20% SIMD efficiency.
// The traversal instead queues (lane, leaf) pairs in a per-wave LDS list and runs them 64 at a
// time, one pair per lane (the owner's ray fetched with ds_bpermute, the leaf with a per-lane
// load), once kBatchFlush are pending and when the walk ends.  Results land per ray by LDS
// atomics: closest hit = atomic min of the key (t bits << 32 | DFS leaf), which for 0 < t
// orders exactly like the reference's (t, DFS leaf) rule; shadow = a flag.
// CULL (the culling tree): an entry is a DevLeaf, and its lane takes the reference's decision on
// the leaf's GUARD box (before the triangle test here, after it for the tests that hit in
// batch_flush_deferred below) — the fast slab test with the 2^-20 band, which on accept
// implies every enclosing reference box accepts, else guard_exact over the
// ancestry — so exactly the tests the reference makes count.  Without CULL (reference
// walk) an entry is a DFS leaf whose boxes the walk has already decided.
// The queue is flushed only between visits, once kBatchFlush tests are pending, and holds a whole
// wide visit's pushes (8 slots x 2 leaves x 64 lanes) above that: no flush inside the slot loop.
// (Round 5: the in-loop check inlined the batch test into every slot and held 69 SGPRs in VGPR
// lanes; without it 7 spill and the C3 frame kernel runs 0.406 -> 0.395 ms, four in flight
// 0.385 -> 0.374, profiles/r05/ab_visit_flush.json.  LDS: 22.6 KB per 4-wave workgroup, seven
// workgroups per CU.)
// A mid-walk flush runs whole 64-test batches only and carries the n & 63 left-over entries to
// the front of the queue (leaf_flush_full); only the walk's last flush runs a partial batch, so a
// traversal of T tests takes ceil(T / 64) batch iterations instead of one half-empty iteration
// per flush (round 9).  Queue bound: a visit starts with fewer than the threshold
// pending — at most 63 after a mid-walk flush — and adds at most a wide visit's pushes.
// (Round 10: 88, not 128 — the 160 B per queue pay for most of the survivor buffer below; round 9
// had measured thresholds down to 96 neutral, profiles/r09/ab_thresholds.json.)
#ifndef RT_BATCH_FLUSH  // primary walk (A/B builds)
#define RT_BATCH_FLUSH 88
#endif
#ifndef RT_SHADOW_FLUSH  // shadow walk (A/B builds)
#define RT_SHADOW_FLUSH 88
#endif
constexpr int kBatchFlush = RT_BATCH_FLUSH;
constexpr int kShadowFlush = RT_SHADOW_FLUSH;
static_assert(kBatchFlush >= 64 && kShadowFlush >= 64, "a mid-walk flush runs a whole batch");
constexpr int kBatchCap =
    (kBatchFlush > kShadowFlush ? kBatchFlush : kShadowFlush) + kWideSlots * 2 * 64;

// The primary traversal's queue pushes write every lane: lanes outside the push mask write a
// junk entry past the queue (q[kBatchCap + ...], never read) instead of taking an exec-mask
// branch (the shadow traversal keeps the branch: junk writes cost it VGPR spills).  A lane's junk
// word is q[kBatchCap + lane], a pair's second one the next lane's first (both garbage): 65
// words, one more to keep the keys 8-byte aligned.
constexpr int kPushJunk = 66;

// Survivors of the leaf batch's triangle tests wait here for their guard decision (batch_flush):
// kSurvivorCap records of (t bits << 32 | queue entry).  Capacity rule: a 64-test iteration
// appends its survivors below the cap; when the buffer is full the guard batch runs on all
// kSurvivorCap of them, and the iteration's survivors that did not fit — the buffer is empty
// again and one iteration has at most 64 — are appended then.  So any number of survivors per
// iteration, 0 to 64, is held, and every guard batch but a walk's last runs on a full wave.
constexpr int kSurvivorCap = 64;

// A queue entry is one 32-bit word: the owner lane above kQueueLeafBits, the leaf (DevLeaf or
// DFS index, < 2^26: assemble_scene refuses larger scenes) below.
constexpr int kQueueLeafBits = 26;
constexpr unsigned kQueueLeafMask = (1u << kQueueLeafBits) - 1u;
struct WaveLeafLds {
  unsigned q[kBatchCap + kPushJunk];  // lane << kQueueLeafBits | leaf
  unsigned long long key[64];       // per lane: closest-hit key, or shadow flag
  unsigned long long sv[kSurvivorCap];  // t bits << 32 | queue entry (see kSurvivorCap)
  int sub;  // the wave's quadrant of a split tile, -1: whole packet (trace_frame_kernel)
  unsigned start;  // the packet's start time, low word (trace_frame_kernel; the struct's padding)
  int tx, ty;  // the packet's tile column and row (sel_tile), worked out once (trace_frame_kernel)
};
// 28 waves per CU = 14 two-wave workgroups.  The frame kernel's workgroup holds
// two of these and 8 B more, and must stay within 11,520 B: 14 of them fit the CU's 160 KiB
// whether the hardware hands LDS out byte-exact (14 x 11,702) or in 512-B or 1,280-B granules
// (11,520 is a multiple of both) — the pre-round-10 workgroup (11,288 B) rounds up to the same.
static_assert(2 * sizeof(WaveLeafLds) + 8 <= 11520, "WaveLeafLds: 14 workgroups per CU");

constexpr unsigned long long kNoHitKey = (0x7f800000ull << 32) | 0xffffffffull;  // (+inf, -1)

// The two 32-bit words of a lane's key: [0] the leaf of a closest-hit key, [1] its t bits.
typedef unsigned __attribute__((may_alias)) key_word_t;
__device__ __forceinline__ key_word_t* key_words(WaveLeafLds& L, int lane) {
  return reinterpret_cast<key_word_t*>(&L.key[lane]);
}
__device__ __forceinline__ const key_word_t* key_words(const WaveLeafLds& L, int lane) {
  return reinterpret_cast<const key_word_t*>(&L.key[lane]);
}
// A shadow walk's commit: the owner's any-hit flag (any writer: same value).  HIGH: the flag is
// the key's high word alone, and the low word — the frame kernel's primary leaf — is left as it
// is (occluded KEEP).
template <bool HIGH>
__device__ __forceinline__ void set_shadow_flag(WaveLeafLds& L, int src) {
  if constexpr (HIGH)
    key_words(L, src)[1] = 1u;
  else
    L.key[src] = 1ull;
}

// This lane's index computed afresh (asm-opaque), so that it is not kept live (and spilled)
// across a traversal: the shadow phase's light loop.
__device__ __forceinline__ int fresh_lane() {
  int lane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
  return lane;
}

// Queue leaf `leaf` for the lanes of `m` (wave-uniform); n = pending entries (wave-uniform).
// (Round 5: 32-bit entries, and lane_id() left to the compiler instead of an asm-opaque
// recomputation per push: C3 frame 0.3905 -> 0.3802 ms four in flight, profiles/r05/ab_queue32.json.)

template <bool ALL = false>
__device__ __forceinline__ void batch_push(WaveLeafLds& L, int& n, int leaf, uint64_t m) {
  const int lane = lane_id();
  const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  const unsigned e = ((unsigned)lane << kQueueLeafBits) | (unsigned)leaf;
  if (ALL) {
    L.q[lane_in(m) ? n + below : kBatchCap + lane] = e;
  } else if (lane_in(m)) {
    L.q[n + below] = e;
  }
  n += __builtin_popcountll(m);
}

// A wide slot's lone leaf (p = 0) or leaf pair (p = 1, wave-uniform) in one branch-free push: a
// lane's rank among the lanes of `m` is shifted by p, the first word goes to its entry and the
// word `leaf + p` to entry + p — the pair's second entry, or for a lone leaf the same word to
// the same place again (LDS writes of one wave complete in order).  ALL: the junk / queue
// select is one v_cndmask on the mask itself (written `lane_in(m) ? :` the compiler wraps the
// rank in an s_and_saveexec / s_or exec pair).  (Round 7, DESIGN.md §5.1: against a branch on
// the pair bit around batch_push / batch_push_pair, 5 scalar-side instructions fewer per leafy
// hit and 1.8 KB less code.)
template <bool ALL = false>
__device__ __forceinline__ void batch_push_n(WaveLeafLds& L, int& n, int leaf, uint64_t m,
                                             unsigned p) {
  const int lane = lane_id();
  const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  const unsigned e = ((unsigned)lane << kQueueLeafBits) | (unsigned)leaf;
  if (ALL) {
    int at;
    asm("v_cndmask_b32 %0, %1, %2, %3"
        : "=v"(at) : "v"(kBatchCap + lane), "v"(n + (below << p)), "s"(m));
    L.q[at] = e;
    L.q[at + (int)p] = e + p;
  } else if (lane_in(m)) {
    const int at = n + (below << p);
    L.q[at] = e;
    L.q[at + (int)p] = e + p;
  }
  n += __builtin_popcountll(m) << p;
}

__device__ __forceinline__ float lane_f(int src, float v) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
}

// Runs the n queued tests; SHADOW: 0 < t < thr of the owner sets its flag, else the owner's
// key takes min(key, (t, leaf)) for 0 < t < inf.  All lanes of the wave take part.  SKIP:
// some lane of the wave skips an axis (else the guard test needs no skip flags).  CAMERA: every
// lane's ray starts at the same point (the frame kernel's primary rays), so the owner's origin —
// and `quot`, which depends on the origin and the scene only — is this lane's own: no fetch.
// WHOLE: only the whole 64-entry batches run (every lane of an iteration holds an entry); returns
// the number of entries run, n & ~63 (else n rounded up).
template <bool SHADOW, bool SPHERES, bool CULL, bool SKIP = true, bool CAMERA = false,
          bool WHOLE = false, bool HIGH = false>
__device__ __forceinline__ int batch_flush(const RenderParams& P, WaveLeafLds& L, int n,
                                           const LaneRay& r, float thr, Diag& dg) {
  static_assert(!CULL || SHADOW, "a culling primary walk defers its guard (leaf_batches)");
  const int lane = lane_id();
  int base = 0;
  for (; WHOLE ? base + 64 <= n : base < n; base += 64) {
    const int i = base + lane;
    const bool valid = WHOLE || i < n;
    const unsigned e = valid ? L.q[i] : 0u;
    const int src = (int)(e >> kQueueLeafBits), idx = (int)(e & kQueueLeafMask);
    LaneRay rr;
    if constexpr (CAMERA) {
      rr.o = r.o;
      rr.quot = r.quot;
    } else {
      rr.o = v3(lane_f(src, r.o.x), lane_f(src, r.o.y), lane_f(src, r.o.z));
      rr.quot = __builtin_amdgcn_ds_bpermute(src << 2, (int)r.quot) != 0;
    }
    rr.d = v3(lane_f(src, r.d.x), lane_f(src, r.d.y), lane_f(src, r.d.z));
    const float othr = SHADOW ? lane_f(src, thr) : 0.0f;
    float t = 0.0f;
    bool hit;
    int leaf;
    if constexpr (CULL) {
      const f4* q = reinterpret_cast<const f4*>(P.leaves + idx);  // idle lanes: record 0, unused
      const f4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
      const int tag = __float_as_int(q0.w);
      leaf = tag & ~kLeafSphere;
      // the guard: the holder box {q1.w, q2.w, q3.x, q3.y, q3.z, q3.w}
      rr.r = v3(__builtin_amdgcn_rcpf(rr.d.x), __builtin_amdgcn_rcpf(rr.d.y),
                __builtin_amdgcn_rcpf(rr.d.z));
      rr.skip0 = SKIP && __builtin_fabsf(rr.d.x) < kEps;
      rr.skip1 = SKIP && __builtin_fabsf(rr.d.y) < kEps;
      rr.skip2 = SKIP && __builtin_fabsf(rr.d.z) < kEps;
      const float g[6] = {q1.w, q2.w, q3.x, q3.y, q3.z, q3.w};
      float tn, tf;
      slab_span<SKIP>(g, rr, tn, tf);
      bool in, out;
      decide_sure(tn, tf, in, out);
      bool ok = valid & in;
      const bool und = valid & !(in | out);
      if (ballot(und)) {
        if (und) ok = guard_exact(P, ~leaf, rr);
        DIAG(if (und) atomicAdd(&g_exact_fallbacks, 1ull));
      }
      DIAG(dg.guard += __builtin_popcountll(ballot(valid)));
      const V3 v0 = v3(q0.x, q0.y, q0.z);
      if (!SPHERES || !(tag & kLeafSphere))
        hit = tri_test(v0, v3(q1.x, q1.y, q1.z), v3(q2.x, q2.y, q2.z), rr, t);
      else
        hit = sphere_test(v0, q1.x, rr, t);
      DIAG(const bool sv = valid & hit & (t > 0.0f) & (t < othr);
           dg.defer[kDfSurvivors] += __builtin_popcountll(ballot(sv));
           dg.defer[kDfRejected] += __builtin_popcountll(ballot(sv & !ok)));
      hit &= ok;
    } else {
      hit = leaf_test<SPHERES>(P.prims, idx, rr, t);  // leaf 0 for idle lanes: unused
      leaf = idx;
    }
    if (SHADOW) {
      if (valid & hit & (t > 0.0f) & (t < othr)) set_shadow_flag<HIGH>(L, src);
    } else if (valid & hit & (t > 0.0f) & (t < RT_INF)) {
      atomicMin(&L.key[src], ((unsigned long long)__float_as_uint(t) << 32) | (unsigned)leaf);
    }
  }
  return base;
}

// ---- the guard deferred to the tests that hit (round 10; culling tree only)
// The guard's outcome is used only where the triangle test hits in range — on C3 one queued
// test in eight to ten — and a wave issues an instruction if any lane needs it, so masking the
// guard inside the iteration saves nothing.  Instead the batch runs in two stages.  Stage 1, per
// 64 queue entries: the owner's ray, three of the DevLeaf's four 16-B words, the triangle or
// sphere test, and the survivors (hit, 0 < t, t in range) appended, compacted by their ballot,
// to WaveLeafLds::sv.  Stage 2 (guard_batch), per kSurvivorCap survivors: the guard decision
// exactly as batch_flush takes it, and the commit for the lanes it accepts.  The committed set
// {guard ok, hit, in range} is the same, and atomicMin does not depend on the order.  The
// survivor count `ns` is wave-uniform and lives across the walk like `pending`: survivors wait
// across flushes for a full guard batch, and only the walk's last guard batch is partial.
// The culling tree's primary walk runs this way; its shadow walk and the reference walks take the
// guard first (batch_flush).  (Round 10 measured both walks in every mode: the primary walk gained
// 3 %, the shadow walk nothing — DESIGN.md §4.5, profiles/r10/ab_defer.json.)

// What the frame kernel's phases hand to each other instead of rebuilding it (rounds 13 and 14,
// DESIGN.md §4.3); every value handed over is the expression the later phase evaluated itself.
//   * the hit point p = e + d * t, computed where the primary walk ends and parked in LDS;
//   * the primary hit's leaf, which stays where the walk left it, in the low word of the lane's
//     L.key (-1 a miss, -2 a lane outside the image or the packet): the shadow walks keep their
//     any-hit flag in the key's high word (occluded KEEP), which the parked point has made free;
//   * the last light's normalize(light - p), taken from its shadow ray (ShadowHand);
//   * the occlusion word, kept in a register when there is one (occ_words == 1).
// The parked point waits in words of the wave's LDS block that are idle from the end of the
// primary walk on: sv (x, y), which only the primary walk's deferred guard uses and which that
// walk drains before it ends, and the junk words past the queue (z), which only the primary
// walk's pushes write.
__device__ __forceinline__ void park_point(WaveLeafLds& L, int lane, V3 p) {
  L.sv[lane] = ((unsigned long long)__float_as_uint(p.y) << 32) | __float_as_uint(p.x);
  L.q[kBatchCap + lane] = __float_as_uint(p.z);
}
__device__ __forceinline__ V3 parked_point(const WaveLeafLds& L, int lane) {
  const unsigned long long xy = L.sv[lane];
  return v3(__uint_as_float((unsigned)xy), __uint_as_float((unsigned)(xy >> 32)),
            __uint_as_float(L.q[kBatchCap + lane]));
}

// Stage 2: the guard decision of the first ns (<= kSurvivorCap) waiting survivors, one per lane,
// and their commit.
template <bool SKIP, bool CAMERA>
__device__ __forceinline__ void guard_batch(const RenderParams& P, WaveLeafLds& L, int ns,
                                            const LaneRay& r, Diag& dg) {
  const int lane = lane_id();
  const bool valid = lane < ns;
  const unsigned long long s = valid ? L.sv[lane] : 0ull;
  const unsigned e = (unsigned)s;
  const int src = (int)(e >> kQueueLeafBits), idx = (int)(e & kQueueLeafMask);
  LaneRay rr;
  if constexpr (CAMERA)
    rr.o = r.o;
  else
    rr.o = v3(lane_f(src, r.o.x), lane_f(src, r.o.y), lane_f(src, r.o.z));
  rr.d = v3(lane_f(src, r.d.x), lane_f(src, r.d.y), lane_f(src, r.d.z));
  const float* q = reinterpret_cast<const float*>(P.leaves + idx);  // idle lanes: record 0, unused
  const int leaf = __float_as_int(q[3]) & ~kLeafSphere;
  const float g0 = q[7], g1 = q[11];
  const f4 q3 = reinterpret_cast<const f4*>(q)[3];
  // the guard: the holder box {q1.w, q2.w, q3.x, q3.y, q3.z, q3.w}
  rr.r = v3(__builtin_amdgcn_rcpf(rr.d.x), __builtin_amdgcn_rcpf(rr.d.y),
            __builtin_amdgcn_rcpf(rr.d.z));
  rr.skip0 = SKIP && __builtin_fabsf(rr.d.x) < kEps;
  rr.skip1 = SKIP && __builtin_fabsf(rr.d.y) < kEps;
  rr.skip2 = SKIP && __builtin_fabsf(rr.d.z) < kEps;
  const float g[6] = {g0, g1, q3.x, q3.y, q3.z, q3.w};
  float tn, tf;
  slab_span<SKIP>(g, rr, tn, tf);
  bool in, out;
  decide_sure(tn, tf, in, out);
  bool ok = valid & in;
  const bool und = valid & !(in | out);
  if (ballot(und)) {
    if (und) ok = guard_exact(P, ~leaf, rr);
    DIAG(if (und) atomicAdd(&g_exact_fallbacks, 1ull));
  }
  DIAG(dg.defer[kDfGuardIters]++;
       dg.defer[kDfRejected] += __builtin_popcountll(ballot(valid & !ok)));
  if (ok) atomicMin(&L.key[src], (s & 0xffffffff00000000ull) | (unsigned)leaf);
}

// Stage 1 over the n queued tests and the guard batches that fill up on the way.  WHOLE (a
// mid-walk flush): the whole 64-entry batches only, as batch_flush, and the survivors still
// waiting at the end stay; else (the walk's last flush) they are drained.
// ns: survivors waiting, in and out.  Returns the number of queue entries run.
template <bool SPHERES, bool SKIP, bool CAMERA, bool WHOLE>
__device__ __forceinline__ int batch_flush_deferred(const RenderParams& P, WaveLeafLds& L, int n,
                                                    int& nsurv, const LaneRay& r, Diag& dg) {
  const int lane = lane_id();
  int base = 0, ns = nsurv;
  for (;;) {
    const bool more = WHOLE ? base + 64 <= n : base < n;
    if (!more && (WHOLE || ns == 0)) break;
    bool late = false;  // this lane's survivor waits for the full buffer's guard batch
    int rank = 0;
    unsigned long long rec = 0ull;
    if (more) {
      const int i = base + lane;
      const bool valid = WHOLE || i < n;
      const unsigned e = valid ? L.q[i] : 0u;
      const int src = (int)(e >> kQueueLeafBits), idx = (int)(e & kQueueLeafMask);
      LaneRay rr;
      if constexpr (CAMERA) {
        rr.o = r.o;
        rr.quot = r.quot;
      } else {
        rr.o = v3(lane_f(src, r.o.x), lane_f(src, r.o.y), lane_f(src, r.o.z));
        rr.quot = __builtin_amdgcn_ds_bpermute(src << 2, (int)r.quot) != 0;
      }
      rr.d = v3(lane_f(src, r.d.x), lane_f(src, r.d.y), lane_f(src, r.d.z));
      // (the guard words q1.w and q2.w ride along unused; q[3] is not loaded)
      const f4* q = reinterpret_cast<const f4*>(P.leaves + idx);  // idle lanes: record 0, unused
      const f4 q0 = q[0], q1 = q[1], q2 = q[2];
      const V3 v0 = v3(q0.x, q0.y, q0.z);
      float t = 0.0f;
      bool hit;
      if (!SPHERES || !(__float_as_int(q0.w) & kLeafSphere))
        hit = tri_test(v0, v3(q1.x, q1.y, q1.z), v3(q2.x, q2.y, q2.z), rr, t);
      else
        hit = sphere_test(v0, q1.x, rr, t);
      const bool surv = valid & hit & (t > 0.0f) & (t < RT_INF);
      DIAG(dg.guard += __builtin_popcountll(ballot(valid)));
      base += 64;
      const uint64_t sm = ballot(surv);
      if (sm) {
        rank = ns + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(sm >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((unsigned)sm, 0u));
        rec = ((unsigned long long)__float_as_uint(t) << 32) | e;
        if (surv && rank < kSurvivorCap) L.sv[rank] = rec;
        late = surv && rank >= kSurvivorCap;
        ns += __builtin_popcountll(sm);
        DIAG(dg.defer[kDfSurvivors] += __builtin_popcountll(sm));
      }
    }
    if (ns >= kSurvivorCap || !more) {
      guard_batch<SKIP, CAMERA>(P, L, ns < kSurvivorCap ? ns : kSurvivorCap, r, dg);
      DIAG(dg.defer[kDfSplitDrains] += ns > kSurvivorCap);
      ns = ns > kSurvivorCap ? ns - kSurvivorCap : 0;
      if (late) L.sv[rank - kSurvivorCap] = rec;  // the buffer is empty again
    }
  }
  nsurv = ns;
  return base;
}

// The leaf batches of one flush: the culling tree's primary walk defers its guard, every other
// walk takes it first (or, the reference walk, has none).  ns: the primary walk's waiting
// survivors; a shadow walk passes a counter that stays 0.
template <bool SHADOW, bool SPHERES, bool CULL, bool SKIP, bool CAMERA, bool WHOLE,
          bool HIGH = false>
__device__ __forceinline__ int leaf_batches(const RenderParams& P, WaveLeafLds& L, int n, int& ns,
                                            const LaneRay& r, float thr, Diag& dg) {
  if constexpr (CULL && !SHADOW)
    return batch_flush_deferred<SPHERES, SKIP, CAMERA, WHOLE>(P, L, n, ns, r, dg);
  else
    return batch_flush<SHADOW, SPHERES, CULL, SKIP, CAMERA, WHOLE, HIGH>(P, L, n, r, thr, dg);
}

// A mid-walk flush (n >= 64 pending): the whole batches only; the n & 63 left-over entries move
// to the front of the queue and stay pending.  The source range starts at full >= 64 > rem, so
// the ranges do not overlap; LDS accesses of one wave complete in order, so the next visit's
// pushes land after the move.  The same tests run as before, a batch later at most; a shadow
// lane whose occluding test is carried stays `alive` until the next flush.
// (The lane index is computed afresh, as in the shadow phase's light loop, so that no address
// derived from it is kept live across the walk: the kernel sits at its 72-VGPR budget.)
template <bool SHADOW, bool SPHERES, bool CULL, bool SKIP, bool CAMERA = false, bool HIGH = false>
__device__ __forceinline__ void leaf_flush_full(const RenderParams& P, WaveLeafLds& L, int& n,
                                                int& ns, const LaneRay& r, float thr, Diag& dg) {
  const int full =
      leaf_batches<SHADOW, SPHERES, CULL, SKIP, CAMERA, true, HIGH>(P, L, n, ns, r, thr, dg);
  const int rem = n - full;
  const int lane = fresh_lane();
  if (lane < rem) L.q[lane] = L.q[full + lane];
  DIAG(dg.ev[kPhFlushes]++; dg.ev[kPhFlushIters] += full / 64;
       dg.carry[0] += rem == 0; dg.carry[1] += rem >= 1 && rem <= 16; dg.carry[2] += rem >= 48);
  n = rem;
}

// Queues the leaf tests of a visited reference node's leaf children for the lanes of h0 / h1.
__device__ __forceinline__ void queue_binary_leaves(WaveLeafLds& L, int& pending, const DevNode& N,
                                                    bool h0, bool h1, uint64_t alive, Diag& dg) {
  if (N.child[0] < 0) {
    const uint64_t b = ballot(h0) & alive;
    batch_push(L, pending, ~N.child[0], b);
    DIAG(dg.leaves++; dg.leaf_lanes += __builtin_popcountll(b));
  }
  if (N.child[1] < 0) {
    const uint64_t b = ballot(h1) & alive;
    batch_push(L, pending, ~N.child[1], b);
    DIAG(dg.leaves++; dg.leaf_lanes += __builtin_popcountll(b));
  }
}

// ------------------------------------------------------------------ 8-wide culling nodes
// The whole 128-B node (DevNode8) in one round trip: two s_load_dwordx16 and one wait.
typedef int v16i __attribute__((ext_vector_type(16)));
// `ref` is the tagged node reference: (ref << 6) as 32 bits is the byte offset of its first slot
// (the tag bit falls off the top; the host keeps the node array below 2^26 slots), used as the
// loads' SGPR offset — one shift and one add per visit instead of a 64-bit address.
__device__ __forceinline__ void load_node8(const DevNode* __restrict__ nodes, int ref, v16i& a,
                                           v16i& b) {
  const unsigned off = (unsigned)ref << 6, off2 = off + 64u;
  asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx16 %1, %2, %4\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(b) : "s"(nodes), "s"(off), "s"(off2) : "memory");
}

// fp16 halves of a slot word: the compiler feeds them to v_fma_mix_f32 straight from the SGPR
__device__ __forceinline__ float half_lo(int w) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)((unsigned)w & 0xffffu));
}
__device__ __forceinline__ float half_hi(int w) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)((unsigned)w >> 16));
}

#define RT_NODE_WORD(k) ((k) < 16 ? a[(k)] : b[(k) - 16])

// One packet visit of an 8-wide culling node.  Every slot takes a plain slab test on its
// conservative box (plane t = fma(h, 2^k / d, (origin - o) / d), the entry plane moved earlier
// and the exit plane later by the ray's own margin 2^-18 |o| / |d| — DESIGN.md §4.2: with the
// host's margin the test never culls a treelet the reference would enter, so no decision band
// is needed); the slots lie sorted by kind, the inner ones from slot 0 upwards and the leafy ones
// from slot 7 downwards, and the visit runs along each kind until it ends (an invalid slot's NaN
// planes would fail the test anyway).  A leafy slot's leaves go to the leaf queue (the exact
// guard decision is taken there); of the entered inner slots the first becomes `node` and the
// others are pushed.  `alive`: lanes still searching.  Returns false when the walk is over.
// (Round 5: shadow rays used to enter the nearest slot by the first entering lane's entry
// distance, so occluders would turn up early; the readlane and compare per entered slot cost
// more than it saved — C3 frame kernel 0.397 -> 0.392 ms, four in flight 0.374 -> 0.369 ms,
// profiles/r05/ab_shadow_first.json.  Any-hit: the visiting order does not change the answer.)
// Plane order per lane: a slot word holds the lo plane in its low half and the hi plane in its
// high half; one v_alignbit by the ray's sh (16 where 1/d < 0) puts the lane's ENTRY plane low,
// so a slot costs 3 alignbit + 6 fma_mix + max3 + min3 + 2 compares instead of a min and a max
// per axis on top (same values: the entry plane moved down, the exit plane up by |m|).  A
// skipped axis (SKIP) gets S = 0 and planes -inf / +inf, once per visit.
// COHERENT (the frame kernel's octant sub-walks): the node belongs to the octant copy of every
// lane in `m` (octant_walks), whose words already hold the entry plane low — the same halves
// reach the same fma_mix operands with no v_alignbit and no use of sh.  Its plane distances are
// in the launch's scaled time t 2^-E (coherent_ray: the ray's reciprocal and margin share times
// 2^-E, every product and sum then scaling exactly), chosen so that every entry distance stays
// below 1 (visit_time_exp), and the zero of `tf >= max(tn, 0)` is the clamp bit of axis 0's entry
// fma_mix: a slot costs 6 fma_mix + max3 + min3 + one compare, 9 VALU.
template <bool SKIP, bool SHADOW, bool DEEP, bool SPHERES, bool COHERENT = false>
__device__ __forceinline__ bool visit_wide(const RenderParams& P, const DevNode* __restrict__ nodes,
                                           WaveLeafLds& L, int& pending, const LaneRay& r, int& node,
                                           uint64_t& m, uint64_t alive, WaveStack<DEEP>& st,
                                           Diag& dg) {
  v16i a, b;
  DIAG(const unsigned long long tl0 = clock_now());
  load_node8(nodes, node, a, b);
  DIAG(dg.cyc_load += clock_now() - tl0);
  const unsigned scale = (unsigned)a[3];
  const int inner_base = a[4], leaf_base = a[5], kinds = a[6];
  const unsigned offs = (unsigned)a[7];
  const unsigned inner = (unsigned)kinds & ~((unsigned)kinds >> 8) & 0xffu;
  DIAG(dg.nodes++; dg.wide++; dg.node_lanes += __builtin_popcountll(m));
  // (COHERENT: the reciprocal and the margin share in the launch's scaled time, coherent_ray)
  const float o[3] = {r.o.x, r.o.y, r.o.z};
  const float rc[3] = {COHERENT ? r.vr.x : r.r.x, COHERENT ? r.vr.y : r.r.y, COHERENT ? r.vr.z : r.r.z};
  const float mg[3] = {COHERENT ? r.vm.x : r.m.x, COHERENT ? r.vm.y : r.m.y, COHERENT ? r.vm.z : r.m.z};
  [[maybe_unused]] const int sh[3] = {r.sh0, r.sh1, r.sh2};
  float S[3], Alo[3], Ahi[3];
#pragma unroll
  for (int x = 0; x < 3; x++) {
    S[x] = __builtin_amdgcn_ldexpf(rc[x], (int)(signed char)(scale >> (8 * x)));
    // (fma: three VALU per axis, and one rounding fewer than a product and a sum — DESIGN.md §4.2)
    const float A = __int_as_float(a[x]) - o[x];
    Alo[x] = __builtin_fmaf(A, rc[x], -__builtin_fabsf(mg[x]));  // entry plane earlier
    Ahi[x] = __builtin_fmaf(A, rc[x], __builtin_fabsf(mg[x]));   // exit plane later
    if (SKIP) {  // a skipped axis: every plane at -inf / +inf (fma(h, 0, -+inf), h finite)
      const bool sk = x == 0 ? r.skip0 : (x == 1 ? r.skip1 : r.skip2);
      S[x] = sk ? 0.0f : S[x];
      Alo[x] = sk ? -RT_INF : Alo[x];
      Ahi[x] = sk ? RT_INF : Ahi[x];
    }
  }
  // The lane mask inside the slab test: a lane outside `m` gets the exit plane -inf and a finite
  // scale on axis 0, once per visit (after the skip selects), so every slot's compare is false
  // for it and the compare's own mask is the set of entering lanes of `m` — no s_andn2 with the
  // mask and no 64-bit zero test per slot.  The same set: a lane in `m` keeps its operands, and
  // the ordered >= equals !(unordered <); outside `m`, f3[0] = fma(h, 1, -inf) = -inf for the
  // finite fp16 h (the lane's own S[0] may be 1/0 = inf, and h * inf with h = 0 a NaN: hence the
  // scale), v_min3 ignores a NaN on the other axes, so tf = -inf, and max(tn, 0) >= 0 whatever
  // tn is (fmaxf drops a NaN tn): -inf >= it is false.  An invalid slot's NaN planes still fail
  // in every lane.
  // COHERENT, where the zero bound is axis 0's clamp (slot_lanes): outside `m` tf is -inf as
  // above, and tn is at least the clamped plane, 0 or more, or a NaN if the clamp lets a NaN
  // entry plane through and the other two are NaN too — -inf >= either is false.  An invalid
  // slot's exit planes are not clamped: tf = min3 of three NaN is NaN and fails every lane,
  // whether the clamp turned the NaN entry plane into 0 or left it.
  {
    const bool in = lane_in(m);
    S[0] = in ? S[0] : 1.0f;
    Ahi[0] = in ? Ahi[0] : -RT_INF;
  }
  int nxt = -1;
  uint64_t nm = 0;
  // One slot's slab test on its three plane words: the lanes of `m` that enter the slot.
  auto slot_lanes = [&](const int (&w3)[3]) -> uint64_t {
    float n3[3], f3[3];
#pragma unroll
    for (int x = 0; x < 3; x++) {
      // this lane's entry plane into the low half (COHERENT: the copy holds it there)
      int w = w3[x];
      if (!COHERENT)
        w = (int)__builtin_amdgcn_alignbit((unsigned)w, (unsigned)w, (unsigned)sh[x]);
      n3[x] = __builtin_fmaf(half_lo(w), S[x], Alo[x]);
      f3[x] = __builtin_fmaf(half_hi(w), S[x], Ahi[x]);
    }
    // COHERENT: tf >= max(tn, 0) with the zero as the clamp bit of axis 0's v_fma_mix — one
    // v_max3 where a v_max and a v_max3 stood.  max3(clamp01(n0), n1, n2) = max(n0, n1, n2, 0)
    // while n0 <= 1, which the launch's time scale sees to (visit_time_exp); a larger n0 enters
    // the compare as 1, that is earlier, so the slot can only be entered by more lanes, the side
    // the guard decides exactly.  In a lane of `m` on a valid slot n0 is no NaN
    // (finite h and S, A finite or, skipped, -inf: clamped to 0).
    if constexpr (COHERENT) {
      n3[0] = __builtin_amdgcn_fmed3f(n3[0], 0.0f, 1.0f);
      const float tn = __builtin_fmaxf(__builtin_fmaxf(n3[0], n3[1]), n3[2]);
      const float tf = __builtin_fminf(__builtin_fminf(f3[0], f3[1]), f3[2]);
      return lanes_ge(tf, tn);
    }
    const float tn = __builtin_fmaxf(__builtin_fmaxf(n3[0], n3[1]), n3[2]);
    const float tf = __builtin_fminf(__builtin_fminf(f3[0], f3[1]), f3[2]);
    // in: tf >= max(tn, 0) — one compare (in a lane of `m`, tn and tf are never NaN on a valid
    // slot: finite fp16 planes, finite scales, skipped axes at -inf / +inf; a lane outside `m`
    // fails it, see above)
    // (m holds no lane outside `alive` wherever a visit starts — occluded() folds it in after
    // every flush and pop_live at every pop — so the slots do not mask with it again)
    return lanes_ge(tf, __builtin_fmaxf(tn, 0.0f));
  };
  // The slots lie sorted by kind (check_accel): the inner slots at 0, 1, ..., the leafy ones at
  // 7, 6, ..., so the visit is two unrolled runs, each ending at the first slot that is not of
  // its kind, and a slot's body holds its own kind's code alone: no kind test per entered slot
  // (round 17: 2 x (s_bitcmp0 + s_cbranch) each) and no rank of the slot among the inner ones
  // for the child reference (5 SALU per inner hit): slot c's child is inner_base + 2c.
  const int child0 = inner_base | kWideTag;
#pragma unroll
  for (int c = 0; c < kWideSlots; c++) {
    if (!(inner & (1u << c))) break;
    DIAG(dg.ev[kPhSlotsTested]++);
    const int w3[3] = {RT_NODE_WORD(8 + 3 * c), RT_NODE_WORD(9 + 3 * c), RT_NODE_WORD(10 + 3 * c)};
    const uint64_t hm = slot_lanes(w3);
    if (hm) {
      DIAG(dg.ev[kPhSlotHits]++; dg.ev[kPhInnerHits]++);
      const int ch = child0 + 2 * c;
      if (nxt < 0) {
        nxt = ch;
        nm = hm;
      } else {
        st.push(ch, hm);
      }
    }
  }
#pragma unroll
  for (int c = kWideSlots - 1; c >= 0; c--) {
    if (!(kinds & (kSlotLeafy << c))) break;
    DIAG(dg.ev[kPhSlotsTested]++);
    const int w3[3] = {RT_NODE_WORD(8 + 3 * c), RT_NODE_WORD(9 + 3 * c), RT_NODE_WORD(10 + 3 * c)};
    const uint64_t hm = slot_lanes(w3);
    if (hm) {
      DIAG(dg.ev[kPhSlotHits]++; dg.ev[kPhLeafyHits]++);
      const int leaf = leaf_base + (int)((offs >> (4 * c)) & 15u);
      [[maybe_unused]] const bool pair = (kinds & (kSlotPair << c)) != 0;  // (RT_DIAG counts)
      DIAG(dg.ev[kPhPairHits] += pair);
      // (the shadow walk keeps the exec-mask pushes: in the separate shadow kernel junk writes
      // cost VGPR spills, and in the fused frame kernel they measured 1.4 % slower, round 17,
      // DESIGN.md §4.3)
      batch_push_n<!SHADOW>(L, pending, leaf, hm, ((unsigned)kinds >> (16 + c)) & 1u);
      DIAG(dg.leaves += 1 + pair; dg.leaf_lanes += (1 + pair) * __builtin_popcountll(hm));
    }
  }
  if (nxt >= 0) {
    node = nxt;
    m = nm;
    return true;
  }
  return st.pop_live(node, m, alive);
}
#undef RT_NODE_WORD

// Wave priority (s_setprio) by phase (round 6).  A node visit is the traversal's dependent chain
// — scalar node load -> slot tests -> lane masks -> next node — of short VALU -> SALU -> branch
// steps, each waiting on the one before; the leaf-batch flushes are long runs of independent
// VALU work on loaded records.  With the visits at the highest priority the arbiter issues a
// ready visit instruction first and the flushes (lowest) fill the slots the chains leave idle;
// setup and shading sit between.  Same box, three interleaved rounds
// (profiles/r06/ab_priority*.json): C3 frame kernel 0.390 -> 0.362 ms one frame at a time,
// six in flight 0.352 -> 0.333 ms per frame; the flushes above the visits, or at the visits'
// level, measured slower.  (A/B builds: -DRT_PRIO_V=.. -DRT_PRIO_F=.. -DRT_PRIO_REST=..)
#ifndef RT_PRIO_V
#define RT_PRIO_V 3
#endif
#ifndef RT_PRIO_F
#define RT_PRIO_F 0
#endif
#ifndef RT_PRIO_REST
#define RT_PRIO_REST 1
#endif
#define RT_PRIO_VISIT_BEGIN __builtin_amdgcn_s_setprio(RT_PRIO_V)
#define RT_PRIO_VISIT_END __builtin_amdgcn_s_setprio(RT_PRIO_REST)
#define RT_PRIO_FLUSH_BEGIN __builtin_amdgcn_s_setprio(RT_PRIO_F)
#define RT_PRIO_FLUSH_END __builtin_amdgcn_s_setprio(RT_PRIO_REST)
// ------------------------------------------------------------------ closest hit
// The reference's (t, leaf) for every active ray: leaf < 0 = miss.  FAST: the 8-wide culling
// tree over reference treelets (the launch takes it only when the scene has one); otherwise
// the reference tree itself.  CAMERA: all rays share one origin (batch_flush).
// OCT (FAST only; the frame kernel's octant_walks): one sub-walk of a packet — the active lanes
// share direction-sign octant k and the walk starts at that octant's copy of the culling nodes,
// accel_root + root_off (root_off = k * accel_stride), whose plane order is read as it lies
// (visit_wide COHERENT).  The caller presets every lane's L.key and reads the packet's result
// from it after the last sub-walk; best_t and best_leaf are not set.
template <bool SKIP, bool FAST, bool DEEP, bool SPHERES, bool CAMERA = false, bool OCT = false>
__device__ __forceinline__ void closest_hit(const RenderParams& P, const DevNode* __restrict__ nodes,
                                            int* spill, WaveLeafLds& L, const LaneRay& r,
                                            bool active, float& best_t, int& best_leaf, Diag& dg,
                                            int root_off = 0, const int* cut = nullptr) {
  static_assert(!OCT || FAST, "octant copies exist of the culling nodes only");
  if (!OCT) {
    best_t = RT_INF;
    best_leaf = -1;
  }
  // (a FAST launch has a node root, use_fast)
  if (!OCT && P.root_kind != kRootNode) {  // the root IS the primitive (BVH.h:13-14): its own rule
    float t;
    if (active && leaf_test<SPHERES>(P.prims, P.root_ref, r, t)) {
      best_t = t;
      best_leaf = P.root_ref;
    }
    return;
  }
  uint64_t m;
  {
    float tn, tf;
    bool acc, und;
    if (FAST) {  // the culling tree's root box (conservative, tested with the band)
      slab_span<SKIP>(P.accel_box, r, tn, tf);
      m = ballot(active && decide_cull(tn, tf));
    } else {
      slab_fast<SKIP>(P.root_box, r, tn, acc, und);
      m = ballot(active && (acc || (und && box_exact(P.root_box, r))));
    }
  }
  if (!m) return;
  const int lane = lane_id();
  WaveStack<DEEP> st;
  st.lds = spill;
  int pending = 0, waiting = 0;  // queued tests; survivors waiting for their guard (wave-uniform)
  if (!OCT) L.key[lane] = kNoHitKey;
  int node = FAST ? P.accel_root + root_off : P.root_ref;
  // The packet's entry cut (entry_record; the primary sub-walks): the walk starts at the cut's
  // first node and holds the others on the stack, all with the root box's mask — the host has shown
  // that no ray of the tile reaches a leaf outside them (entry_cuts.cpp).
  if constexpr (OCT) {
    if (cut) {
      node = cut[0] + root_off;
#pragma unroll
      for (int i = 1; i < kEntryCut; i++)
        if (cut[i] >= 0) st.push(cut[i] + root_off, m);
      // (the LDS stack's push writes under `lane 0`: folded into these wave-uniform conditions,
      // that branch made the compiler take the stack pointer for a per-lane value)
      if constexpr (DEEP) st.sp = uniform(st.sp);
    }
  }
  // (an octant sub-walk: the visits' priority is set once and after each flush, and lowered where
  // the walk leaves the loop — no s_setprio pair between two visits that no flush separates,
  // DESIGN.md §4.3 round 14; every other walk keeps the pair around each visit)
  constexpr bool kAtExit = OCT;
  if (kAtExit) RT_PRIO_VISIT_BEGIN;
  for (;;) {
    if (pending >= kBatchFlush) {  // between visits: only the ray and the stack are live
      DIAG(const unsigned long long tf0 = clock_now());
      RT_PRIO_FLUSH_BEGIN;
      leaf_flush_full<false, SPHERES, FAST, SKIP, CAMERA>(P, L, pending, waiting, r, 0.0f, dg);
      if (kAtExit)
        RT_PRIO_VISIT_BEGIN;
      else
        RT_PRIO_FLUSH_END;
      DIAG(dg.cyc_flush += clock_now() - tf0);
    }
    if constexpr (FAST) {
      DIAG(const unsigned long long tv0 = clock_now(); dg.ev[kPhVisits]++);
      if (!kAtExit) RT_PRIO_VISIT_BEGIN;
      const bool more =
          visit_wide<SKIP, false, DEEP, SPHERES, OCT>(P, nodes, L, pending, r, node, m, ~0ull, st, dg);
      if (!kAtExit) RT_PRIO_VISIT_END;
      DIAG(dg.cyc_visit += clock_now() - tv0);
      if (!more) break;
    } else {
      const DevNode N = nodes[node];
      bool h0, h1;
      float t0, t1;
      visit_node<SKIP>(N, r, lane_in(m), h0, h1, t0, t1);
      DIAG(dg.nodes++; dg.node_lanes += __builtin_popcountll(m));
      queue_binary_leaves(L, pending, N, h0, h1, ~0ull, dg);
      // leaves are queued; only inner children are entered
      const uint64_t m0 = N.child[0] >= 0 ? ballot(h0) : 0ull;
      const uint64_t m1 = N.child[1] >= 0 ? ballot(h1) : 0ull;
      if (!advance(st, N.child[0], N.child[1], m0, m1, t0, t1, node, m, ~0ull)) break;
    }
  }
  if (kAtExit) RT_PRIO_VISIT_END;
  if (pending | waiting) {  // the last tests, and the survivors still waiting for their guard
    DIAG(const unsigned long long tf0 = clock_now());
    RT_PRIO_FLUSH_BEGIN;
    leaf_batches<false, SPHERES, FAST, SKIP, CAMERA, false>(P, L, pending, waiting, r, 0.0f, dg);
    RT_PRIO_FLUSH_END;
    DIAG(dg.cyc_flush += clock_now() - tf0; dg.ev[kPhFlushes] += pending != 0;
         dg.ev[kPhFlushIters] += (pending + 63) / 64);
  }
  DIAG(dg.ev[kPhPushes] += st.pushes; dg.ev[kPhPops] += st.pops);
  if (!OCT) {
    const unsigned long long key = L.key[lane];
    best_t = __uint_as_float((unsigned)(key >> 32));
    best_leaf = (int)(unsigned)key;
  }
}

// ------------------------------------------------------------------ shadow (any hit)
// Occluded iff some leaf the ray may reach has 0 < t < thr — identical to the reference's
// closest-hit shadow test `0 < t_closest < dist - eps` (HW2/Scene.cpp:123-127), appendix A.7.
// OCT: one sub-walk of a packet, as in closest_hit — the caller clears every lane's L.key
// and reads it after the last sub-walk; the value returned then covers the lanes walked so far.
// KEEP (the frame kernel): the flag is the key's high word alone — cleared, tested and
// returned — and the low word, the lane's primary leaf, is left as it is.
template <bool SKIP, bool FAST, bool DEEP, bool SPHERES, bool OCT = false, bool KEEP = false>
__device__ __forceinline__ bool occluded(const RenderParams& P, const DevNode* __restrict__ nodes,
                                         int* spill, WaveLeafLds& L, const LaneRay& r, bool active,
                                         float thr, Diag& dg, int root_off = 0) {
  static_assert(!OCT || FAST, "octant copies exist of the culling nodes only");
  if (!OCT && P.root_kind != kRootNode) {
    float t;
    return active && leaf_test<SPHERES>(P.prims, P.root_ref, r, t) && t < thr && t > 0.0f;
  }
  uint64_t m;
  {
    float tn, tf;
    bool acc, und;
    // thr <= 0 (or NaN): nothing can satisfy 0 < t < thr
    if (FAST) {
      slab_span<SKIP>(P.accel_box, r, tn, tf);
      m = ballot(active && thr > 0.0f && decide_cull(tn, tf));
    } else {
      slab_fast<SKIP>(P.root_box, r, tn, acc, und);
      m = ballot(active && thr > 0.0f && (acc || (und && box_exact(P.root_box, r))));
    }
  }
  if (!m) return false;
  uint64_t alive = m;
  const int lane = lane_id();
  WaveStack<DEEP> st;
  st.lds = spill;
  // (waiting: the survivor count the shared flush helpers take by reference; a shadow walk has no
  // deferred guard, so it stays 0 — kept because the shipped listing changes without it)
  int pending = 0, waiting = 0;  // queued tests (wave-uniform)
  if (!OCT) {
    unsigned long long clear = 0ull;
    asm volatile("" : "+v"(clear));  // a fresh zero here, not one kept (and spilled) across the walk
    if (KEEP)
      key_words(L, lane)[1] = (unsigned)clear;
    else
      L.key[lane] = clear;
  }
  int node = FAST ? P.accel_root + root_off : P.root_ref;
  constexpr bool kAtExit = OCT;  // (as in closest_hit)
  if (kAtExit) RT_PRIO_VISIT_BEGIN;
  for (;;) {
    if (pending >= kShadowFlush) {  // between visits; a lane found occluded stops entering nodes
      DIAG(const unsigned long long tf0 = clock_now());
      RT_PRIO_FLUSH_BEGIN;
      leaf_flush_full<true, SPHERES, FAST, SKIP, false, KEEP>(P, L, pending, waiting, r, thr, dg);
      if (kAtExit)
        RT_PRIO_VISIT_BEGIN;
      else
        RT_PRIO_FLUSH_END;
      DIAG(dg.cyc_flush += clock_now() - tf0);
      alive &= ~ballot(KEEP ? key_words(L, lane)[1] != 0u : L.key[lane] != 0ull);
      m &= alive;
      if (!m && !st.pop_live(node, m, alive)) break;
    }
    if constexpr (FAST) {
      DIAG(const unsigned long long tv0 = clock_now(); dg.ev[kPhVisits]++);
      if (!kAtExit) RT_PRIO_VISIT_BEGIN;
      const bool more =
          visit_wide<SKIP, true, DEEP, SPHERES, OCT>(P, nodes, L, pending, r, node, m, alive, st, dg);
      if (!kAtExit) RT_PRIO_VISIT_END;
      DIAG(dg.cyc_visit += clock_now() - tv0);
      if (!more) break;
    } else {
      const DevNode N = nodes[node];
      bool h0, h1;
      float t0, t1;
      visit_node<SKIP>(N, r, lane_in(m), h0, h1, t0, t1);
      DIAG(dg.nodes++; dg.node_lanes += __builtin_popcountll(m));
      queue_binary_leaves(L, pending, N, h0, h1, alive, dg);  // the still-unoccluded lanes
      const uint64_t m0 = N.child[0] >= 0 ? ballot(h0) & alive : 0ull;
      const uint64_t m1 = N.child[1] >= 0 ? ballot(h1) & alive : 0ull;
      if (!advance(st, N.child[0], N.child[1], m0, m1, t0, t1, node, m, alive)) break;
    }
  }
  if (kAtExit) RT_PRIO_VISIT_END;
  if (pending | waiting) {
    DIAG(const unsigned long long tf0 = clock_now());
    RT_PRIO_FLUSH_BEGIN;
    leaf_batches<true, SPHERES, FAST, SKIP, false, false, KEEP>(P, L, pending, waiting, r, thr, dg);
    RT_PRIO_FLUSH_END;
    DIAG(dg.cyc_flush += clock_now() - tf0; dg.ev[kPhFlushes] += pending != 0;
         dg.ev[kPhFlushIters] += (pending + 63) / 64);
  }
  DIAG(dg.ev[kPhPushes] += st.pushes; dg.ev[kPhPops] += st.pops);
  return KEEP ? key_words(L, lane)[1] != 0u : L.key[lane] != 0ull;
}

// The kernel's RenderParams (its FIRST argument, so at offset 0 of the kernarg segment) read
// through a pointer the compiler cannot see through: loads from it are not hoisted above this
// point, so the packet code does not pull every field it uses into SGPRs for the whole kernel
// (they were spilled to VGPR lanes across the traversal and reloaded per visit).
typedef __attribute__((address_space(4))) const RenderParams KernargParams;
__device__ __forceinline__ const RenderParams& fresh_params(const RenderParams& P) {
  (void)P;
  KernargParams* p = (KernargParams*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const RenderParams*)p;
}

// The frame kernel's scaled-time exponent (PacketGeom::neg_t_exp of its LAST argument), read the
// same way where a packet forms a ray, so that it is not kept in an SGPR across the walks.
// FrameKernargs: trace_frame_kernel's parameters in order, for the offset alone.
struct FrameKernargs {
  RenderParams P;
  const DevNode* nodes;
  const DevLight* lights;
  PacketGeom G;
};
__device__ __forceinline__ int fresh_neg_t_exp() {
  typedef __attribute__((address_space(4))) const FrameKernargs Args;
  Args* p = (Args*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p->G.neg_t_exp;
}

// The entry cut of the wave's tile (RenderParams::entry_cuts): one scalar load of the tile's
// record, its address from the wave's tile in LDS and the kernel arguments read afresh, so that
// nothing of it is live across a walk.  Without a table, the root alone.
struct alignas(4 * kEntryCut) EntryRecord {
  int ref[kEntryCut];
};
__device__ __forceinline__ EntryRecord entry_record(const RenderParams& P, const WaveLeafLds& L) {
  const RenderParams& F = fresh_params(P);
  EntryRecord rec;
  rec.ref[0] = F.accel_root;
#pragma unroll
  for (int i = 1; i < kEntryCut; i++) rec.ref[i] = -1;
  if (F.entry_cuts) {
    const int tile = uniform(L.ty) * F.tiles_x + uniform(L.tx);
    // (constant address space: the table is read-only for the life of the scene — a scalar load)
    typedef __attribute__((address_space(4))) const EntryRecord Records;
    Records* q = (Records*)F.entry_cuts + tile;
#pragma unroll
    for (int i = 0; i < kEntryCut; i++) rec.ref[i] = q->ref[i];
  }
  // (wave-uniform by construction; said so, since the references feed scalar node loads)
#pragma unroll
  for (int i = 0; i < kEntryCut; i++) rec.ref[i] = uniform(rec.ref[i]);
  return rec;
}

// ------------------------------------------------------------------ render kernels
// Three phases per packet (trace_frame_kernel): the primary phase finds each pixel's closest
// hit and leaves its leaf and its point in the wave's LDS block; the shadow phase traces the
// point-light shadow rays from the hit point into occlusion bits; the shading phase runs the
// point-light loop.  Going through LDS keeps each phase's live state small (occupancy is what
// hides the dependent node loads).  (Until round 14 an 8-byte {t, leaf} record per pixel went
// through memory instead)
//
// A packet is normally one wave's 64 lanes = the tile's 8x8 pixels.  A heavy tile can instead
// be split over four waves (sub = 0..3: wave `sub` takes quadrant `sub` of the tile, 4x4 pixels
// in lanes 0..15): fewer rays per wave walk a smaller union of BVH paths, and the
// four quadrants run side by side (kSplitEntries workgroups of kTraceWaves waves).
struct PacketPixel {
  int lane;  // pixel lane: the pixel's index within the tile's 8x8 (its record's slot)
  int px, py;
  bool own;    // this wave lane holds a pixel of the packet (all lanes unless split)
  bool valid;  // ... inside the image
};

// Pixel lane of wave lane `lane` (-1: none, the lanes 16..63 of a quadrant wave).
__device__ __forceinline__ int pixel_lane(int lane, int sub) {
  if (sub < 0) return lane;
  return lane < 16 ? ((sub >> 1) * 4 + (lane >> 2)) * kTile + (sub & 1) * 4 + (lane & 3) : -1;
}

// The pixel of wave lane `lane` in the packet of tile (tx, ty).
__device__ __forceinline__ PacketPixel tile_pixel(const RenderParams& P, int tx, int ty, int sub,
                                                 int lane) {
  PacketPixel q;
  const int pl = pixel_lane(lane, sub);
  q.own = pl >= 0;
  q.lane = q.own ? pl : 0;
  q.px = tx * kTile + (q.lane & 7);
  const int lr = ty * kTile + (q.lane >> 3);  // logical row
  q.valid = q.own && q.px < P.width && lr < P.rows;
  q.py = P.row0 + lr * P.row_stride;
  return q;
}

// (the recursive kernel: a packet per selected tile, its tile divided out in place)
__device__ __forceinline__ PacketPixel packet_pixel(const RenderParams& P, int sel, int sub = -1,
                                                   int lane = lane_id()) {
  int tx, ty;
  if (P.block_deal) {  // selected block sel / 4, its tile sel % 4
    deal_block_tile(P.tiles_x, P.tile_begin + (sel >> 2) * P.tile_step, sel & 3, tx, ty);
  } else {
    const int tile = P.tile_begin + sel * P.tile_step;
    tx = tile % P.tiles_x;
    ty = tile / P.tiles_x;
  }
  return tile_pixel(P, tx, ty, sub, lane);
}

// This wave's quadrant (-1: the whole packet), kept in the wave's LDS block instead of a
// register across the traversals.
__device__ __forceinline__ int wave_sub(const WaveLeafLds& L) { return uniform(L.sub); }

// The frame kernel's packet: its tile was worked out once, when the wave took it, and waits in
// the wave's LDS block like the quadrant (every lane reads the same word: a broadcast).
__device__ __forceinline__ PacketPixel wave_pixel(const RenderParams& P, const WaveLeafLds& L,
                                                 int lane = lane_id()) {
  return tile_pixel(P, L.tx, L.ty, wave_sub(L), lane);
}

// ------------------------------------------------------------------ MSAA sample positions
// HW2/Scene.cpp:35-44: a std::default_random_engine (libstdc++ minstd_rand0, x <- 16807 x mod
// 2^31-1) per pixel, seeded here with splitmix64(seed, pixel) instead of the wall clock, and
// uniform_real_distribution<float>(0, 1) = generate_canonical<float, 24>: one draw u,
// float(u - 1) / 2^31, clamped below 1.  Sample s = x*n + y uses draws 2s+1 and 2s+2.
__device__ __forceinline__ unsigned long long msaa_pixel_seed(unsigned long long base,
                                                              unsigned long long pixel) {
  unsigned long long z = base + 0x9E3779B97F4A7C15ull * (pixel + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned minstd_state0(unsigned long long seed) {
  const unsigned x = (unsigned)(seed % kMinstdM);
  return x == 0 ? 1u : x;
}

__device__ __forceinline__ unsigned minstd_mulmod(unsigned a, unsigned b) {
  unsigned long long p = (unsigned long long)a * b;  // < 2^62; 2^31 = 1 (mod 2^31-1)
  p = (p & kMinstdM) + (p >> 31);
  p = (p & kMinstdM) + (p >> 31);
  return (unsigned)(p >= kMinstdM ? p - kMinstdM : p);
}

__device__ __forceinline__ float minstd_uniform01(unsigned u) {
  float r = (float)(u - 1u) / 2147483648.0f;  // exact: power-of-two divisor
  return r >= 1.0f ? __uint_as_float(0x3f7fffffu) : r;
}

// sample_x, sample_y of HW2/Scene.cpp:43-44 for sample index s of pixel (px, py)
__device__ __forceinline__ void msaa_offsets(const RenderParams& P, int px, int py, float& sx,
                                             float& sy) {
  const unsigned u0 = minstd_state0(
      msaa_pixel_seed(P.msaa_seed, (unsigned long long)py * (unsigned)P.width + (unsigned)px));
  const float n = (float)P.msaa_n;
  sx = ((float)(P.msaa_s / P.msaa_n) + minstd_uniform01(minstd_mulmod(u0, P.msaa_mul[0]))) / n;
  sy = ((float)(P.msaa_s % P.msaa_n) + minstd_uniform01(minstd_mulmod(u0, P.msaa_mul[1]))) / n;
}

// Camera::calculate_ray_at (HW2/Camera.h:30-35); x + 0.5 is exact in fp32 for x < 2^23.
// MSAA passes x = i + sample_x - 0.5 (a double narrowed to the float parameter) and the
// camera widens it again for x + 0.5 before the float multiply.
__device__ __forceinline__ V3 primary_dir(const RenderParams& P, int px, int py) {
  float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
  if (P.msaa_n) {
    float sx, sy;
    msaa_offsets(P, px, py, sx, sy);
    fx = (float)((double)(float)((double)((float)px + sx) - 0.5) + 0.5);
    fy = (float)((double)(float)((double)((float)py + sy) - 0.5) + 0.5);
  }
  const V3 s = (ld3(P.cam_tl) + ld3(P.cam_su) * fx) - ld3(P.cam_sv) * fy;
  return normalize(s - ld3(P.cam_e));
}

__device__ __forceinline__ unsigned long long* counter_row(const RenderParams& P, int sel) {
  return P.counters + kCounterWidth * (sel % kCounterSlots);
}

// What the shading phase reads back of the primary hit: x = the leaf (-1 miss, -2 outside the
// image), y = 0 since the point is parked (it was the bits of t).  (The shape the memory record
// had until round 14; shade_pixel keeps it because the shipped listing changes with a plain int.)
struct alignas(8) int2_t {
  int32_t x, y;
};
__device__ __forceinline__ int hit_leaf(int2_t rec) { return rec.x; }

// The frame kernel's walks over the octant copies of the culling nodes (kOctantCopies,
// rt_internal.h).  A lane's octant is the sign of its three reciprocals — per axis exactly the
// predicate behind LaneRay::sh, so +-0 and skipped axes fall where the per-lane order puts them
// (a skipped axis has S = 0 and planes at -+inf: either copy gives the same distances).
__device__ __forceinline__ int lane_octant(const LaneRay& r) {
  return (int)((__float_as_uint(r.r.x) >> 31) | ((__float_as_uint(r.r.y) >> 31) << 1) |
               ((__float_as_uint(r.r.z) >> 31) << 2));
}
// Calls walk(mine, k) once per octant k present among the `active` lanes, `mine` being this lane's
// membership: a wave-uniform loop — the first remaining lane's octant, the lanes that share it,
// their walk, and again without them.  A camera's or a light's rays change sign along a line
// through the image, so nearly every packet makes one walk.  Each lane takes part in exactly one
// walk, and the walks leave their results per lane in L.key, so their order does not matter.
// The octant is recomputed from the ray per walk, not kept in a register across one.
template <typename F>
__device__ __forceinline__ void octant_walks(const LaneRay& r, bool active, Diag& dg, F&& walk) {
  uint64_t rest = ballot(active);
  DIAG(dg.oct_packets += rest != 0);
  while (rest) {
    const int oct = lane_octant(r);
    const int k = __builtin_amdgcn_readlane(oct, (int)__builtin_ctzll(rest));
    const bool mine = lane_in(rest) && oct == k;
    rest &= ~ballot(mine);
    DIAG(dg.oct_walks++);
    walk(mine, k);
  }
}

// One wave = the 8x8 packet of selected tile `sel` (< num_sel_tiles): closest hit per pixel, its
// leaf into the lane's key and its point parked beside it.
template <bool FAST, bool DEEP, bool SPHERES>
__device__ __forceinline__ void primary_packet(const RenderParams& P,
                                               const DevNode* __restrict__ nodes, int sel,
                                               int* spill, WaveLeafLds& L) {
  DIAG(const unsigned long long s0 = clock_now());
  const PacketPixel q = wave_pixel(P, L);
  LaneRay ray = make_ray(ld3(P.cam_e), primary_dir(P, q.px, q.py), P.quot_ok);
  if constexpr (FAST) coherent_ray(ray, fresh_neg_t_exp());
  // The camera origin is wave-uniform; left to itself the compiler keeps it in 3 SGPRs and
  // copies it to VGPRs at every node visit (a VALU op takes one SGPR operand, the box
  // coordinate already is one).  Pin it to VGPRs once.
  asm volatile("" : "+v"(ray.o.x), "+v"(ray.o.y), "+v"(ray.o.z));
  const bool any_skip = q.valid && (ray.skip0 || ray.skip1 || ray.skip2);
  Diag dg;
  float t;
  int leaf;
  // (CAMERA = true: every lane's origin is cam_e, so the leaf batch fetches no owner origin)
  DIAG(const unsigned long long s1 = clock_now());
  if constexpr (FAST) {  // the culling tree: one sub-walk per octant present in the packet
    L.key[lane_id()] = kNoHitKey;
    octant_walks(ray, q.valid, dg, [&](bool mine, int k) {
      const int off = k * P.accel_stride;
      const EntryRecord cut = entry_record(P, L);  // (per sub-walk: not held across one)
      if (ballot(mine && any_skip))
        closest_hit<true, FAST, DEEP, SPHERES, true, true>(P, nodes, spill, L, ray, mine, t, leaf,
                                                           dg, off, cut.ref);
      else
        closest_hit<false, FAST, DEEP, SPHERES, true, true>(P, nodes, spill, L, ray, mine, t, leaf,
                                                            dg, off, cut.ref);
    });
    const unsigned long long key = L.key[lane_id()];
    t = __uint_as_float((unsigned)(key >> 32));
    leaf = (int)(unsigned)key;
  } else if (ballot(any_skip)) {  // the reference traversal
    closest_hit<true, FAST, DEEP, SPHERES, true>(P, nodes, spill, L, ray, q.valid, t, leaf, dg);
  } else {
    closest_hit<false, FAST, DEEP, SPHERES, true>(P, nodes, spill, L, ray, q.valid, t, leaf, dg);
  }
  DIAG(const unsigned long long s2 = clock_now());
  // the hit point e + d * t (Ray::point_at, HW2/Scene.cpp:101) while d and t are in registers; the
  // later phases read it back (a miss parks inf or NaN, which nobody reads)
  park_point(L, lane_id(), ray.o + ray.d * t);
  const RenderParams& Pw = fresh_params(P);  // post-traversal fields: not live across it
  const PacketPixel qw = wave_pixel(Pw, L);  // (recomputed, not kept)
  // The later phases read the leaf from the low word of this lane's key (-1 a miss).  Written by
  // every lane: a walk that found nothing to enter (or a root primitive) never set the key, and a
  // lane outside the image, or of a quadrant wave outside the packet, holds -2.
  key_words(L, lane_id())[0] = (unsigned)(qw.valid ? leaf : -2);
  const unsigned long long nvalid = __builtin_popcountll(ballot(qw.valid));  // (all lanes)
  const unsigned long long nhit = __builtin_popcountll(ballot(qw.valid && leaf >= 0));
  if (Pw.counters && lane_id() == 0) {  // spread over kCounterSlots rows: no hot address
    unsigned long long* c = counter_row(Pw, sel);
    atomicAdd(&c[kCntPrimary], nvalid);
    atomicAdd(&c[kCntHits], nhit);
#ifdef RT_DIAG
    const unsigned long long s3 = clock_now();  // (lane 0's, past the ray counters)
    atomicAdd(&g_phase[kPhCycPrimSetup], s1 - s0);
    atomicAdd(&g_phase[kPhCycPrimWalk], s2 - s1);
    atomicAdd(&g_phase[kPhCycPrimTail], s3 - s2);
    atomicAdd(&c[kCntPrimNodes], dg.nodes);
    atomicAdd(&c[kCntPrimNodeLanes], dg.node_lanes);
    atomicAdd(&c[kCntPrimLeaves], dg.leaves);
    atomicAdd(&c[kCntPrimLeafLanes], dg.leaf_lanes);
    atomicAdd(&c[kCntPrimWide], dg.wide);
    atomicAdd(&c[kCntGuardTests], dg.guard);
    for (int k = 0; k < kPhaseEvents; k++) atomicAdd(&g_phase[k], dg.ev[k]);
    atomicAdd(&g_phase[kPhCycPrimVisit], dg.cyc_visit);
    atomicAdd(&g_phase[kPhCycPrimLoad], dg.cyc_load);
    atomicAdd(&g_phase[kPhCycPrimFlush], dg.cyc_flush);
    for (int k = 0; k < 3; k++) atomicAdd(&g_phase[kPhCarryZero + k], dg.carry[k]);
    for (int k = 0; k < kDeferEvents; k++) atomicAdd(&g_phase[kPhDeferPrim + k], dg.defer[k]);
    atomicAdd(&g_phase[kPhOctPrimPackets], dg.oct_packets);
    atomicAdd(&g_phase[kPhOctPrimWalks], dg.oct_walks);
#endif
  }
}

// What the shadow phase leaves in registers for the shading phase (nothing of it is live across
// a walk that follows: `wi` and `bits` are each written after their walk).  (The last light's
// length(light - p) handed over as well measured inside the run-to-run range: DESIGN.md §4.3.)
struct ShadowHand {
  V3 wi = {0.0f, 0.0f, 0.0f};  // the last light's normalize(light - p)
  unsigned bits = 0;           // the last occlusion word (the only one when occ_words == 1)
};

// Shadow rays of HW2/Scene.cpp:113-127: one bit per point light, set when the light is
// occluded for this pixel's primary hit.
template <bool FAST, bool DEEP, bool SPHERES>
__device__ __forceinline__ void shadow_packet(const RenderParams& P0,
                                              const DevNode* __restrict__ nodes,
                                              const DevLight* __restrict__ lights, int sel,
                                              int* spill, WaveLeafLds& L, ShadowHand& hand) {
  Diag dg;
  for (int w = 0; w < P0.occ_words; w++) {
    unsigned bits = 0;
    const int lend = min(P0.num_lights, 32 * (w + 1));
    for (int li = 32 * w; li < lend; li++) {
      // per light: the pixel's leaf and its hit point are read back from the wave's LDS block
      // (park_point), so nothing but the occlusion bits is live across the traversal
      DIAG(const unsigned long long s0 = clock_now());
      const RenderParams& P = fresh_params(P0);
      const DevLight& lt = lights[li];
      // the packet's pixel indices recomputed here, not hoisted out of the light loop (where
      // they would be live across the traversal and spilled to scratch)
      int sel_l = sel;
      asm volatile("" : "+s"(sel_l));
      const int lane_l = fresh_lane();
      // the leaf in the lane's key: -1 a miss, -2 no pixel of the frame
      const bool hit = (int)key_words(L, lane_l)[0] >= 0;
      V3 pk = v3(0, 0, 0);
      if (hit) pk = parked_point(L, lane_l);
      if (li == 0 && P.counters) {  // the packet's shadow rays: every light's are these lanes'
        const unsigned long long nhit = __builtin_popcountll(ballot(hit));
        if (lane_l == 0)
          atomicAdd(&counter_row(P, sel_l)[kCntShadow], nhit * (unsigned long long)P.num_lights);
      }
      const V3 ld = ld3(lt.position) - pk;
      const V3 wi = normalize_shared(ld, !hit);  // (a lane without a hit traces no shadow ray)
      const float dist = length(ld);
      LaneRay sr = make_ray(pk + wi * P.eps, wi, P.quot_ok);  // p + eps * w_i
      if constexpr (FAST) coherent_ray(sr, fresh_neg_t_exp());
      const float thr = dist - P.eps;
      const bool any_skip = hit && (sr.skip0 || sr.skip1 || sr.skip2);
      bool occ;
      DIAG(const unsigned long long s1 = clock_now());
      if constexpr (FAST) {  // (KEEP: the walks use the key's flag word only)
        unsigned long long clear = 0ull;
        asm volatile("" : "+v"(clear));  // (a fresh zero, as in occluded)
        key_words(L, lane_l)[1] = (unsigned)clear;  // the leaf below it stays for the shading
        octant_walks(sr, hit, dg, [&](bool mine, int k) {
          const int off = k * P.accel_stride;
          if (ballot(mine && any_skip))
            occluded<true, FAST, DEEP, SPHERES, true, true>(P, nodes, spill, L, sr, mine, thr, dg,
                                                            off);
          else
            occluded<false, FAST, DEEP, SPHERES, true, true>(P, nodes, spill, L, sr, mine, thr, dg,
                                                             off);
        });
        occ = key_words(L, fresh_lane())[1] != 0u;
      } else {  // the reference traversal
        occ = ballot(any_skip) ? occluded<true, FAST, DEEP, SPHERES, false, true>(
                                     P, nodes, spill, L, sr, hit, thr, dg)
                               : occluded<false, FAST, DEEP, SPHERES, false, true>(
                                     P, nodes, spill, L, sr, hit, thr, dg);
      }
      DIAG(const unsigned long long s2 = clock_now());
      bits |= (occ ? 1u : 0u) << (li - 32 * w);
      hand.wi = sr.d;  // (the last light's is the one that stays)
      DIAG(dg.cyc_setup += s1 - s0);
      DIAG(dg.cyc_walk += s2 - s1);
    }
    DIAG(const unsigned long long s3 = clock_now());
    const RenderParams& Pw = fresh_params(P0);
    int sel_w = sel;
    asm volatile("" : "+s"(sel_w));
    const int pl = pixel_lane(fresh_lane(), wave_sub(L));
    // a lone occlusion word goes to the shading in a register; nothing else reads P.occ
    hand.bits = bits;
    if (pl >= 0 && Pw.occ_words != 1)
      Pw.occ[((size_t)sel_w * (kTile * kTile) + pl) * Pw.occ_words + w] = bits;
    DIAG(dg.cyc_tail += clock_now() - s3);
  }
#ifdef RT_DIAG
  const RenderParams& Pc = fresh_params(P0);
  if (Pc.counters) {
    if (lane_id() == 0) {
      unsigned long long* c = counter_row(Pc, sel);
      atomicAdd(&c[kCntShadNodes], dg.nodes);
      atomicAdd(&c[kCntShadNodeLanes], dg.node_lanes);
      atomicAdd(&c[kCntShadLeaves], dg.leaves);
      atomicAdd(&c[kCntShadLeafLanes], dg.leaf_lanes);
      atomicAdd(&c[kCntShadWide], dg.wide);
      atomicAdd(&c[kCntGuardTests], dg.guard);
      for (int k = 0; k < kPhaseEvents; k++) atomicAdd(&g_phase[kPhaseEvents + k], dg.ev[k]);
      atomicAdd(&g_phase[kPhCycShadVisit], dg.cyc_visit);
      atomicAdd(&g_phase[kPhCycShadLoad], dg.cyc_load);
      atomicAdd(&g_phase[kPhCycShadFlush], dg.cyc_flush);
      for (int k = 0; k < 3; k++) atomicAdd(&g_phase[kPhCarryZero + k], dg.carry[k]);
      for (int k = 0; k < kDeferEvents; k++) atomicAdd(&g_phase[kPhDeferShad + k], dg.defer[k]);
      atomicAdd(&g_phase[kPhOctShadPackets], dg.oct_packets);
      atomicAdd(&g_phase[kPhOctShadWalks], dg.oct_walks);
      atomicAdd(&g_phase[kPhCycShadSetup], dg.cyc_setup);
      atomicAdd(&g_phase[kPhCycShadWalk], dg.cyc_walk);
      atomicAdd(&g_phase[kPhCycShadTail], dg.cyc_tail);
    }
  }
#endif
}

// Local shading of HW2/Scene.cpp:101-138 given the occlusion bits, in the reference's
// accumulation order: ambient, then per light diffuse then specular.  No traversal here, so
// the fp64 pow (HW2 calls ::pow(double, double)) costs no occupancy in the traversal kernels.
// The leaf's normal and material come in one 16-B load (normals[4 * leaf + 3] holds the
// material index); the DevPrim record is read only in scenes with spheres (its kind).
// (float)pow((double)c, (double)p) of HW2/Scene.cpp:133-137.  p == 1 returns c itself: the exact
// result is the double c, and both glibc's pow (< 0.52 ulp) and ocml's (< 1 ulp) return an exact
// result when one exists, so the reference gets c too.  Any other exponent takes the fp64 pow.
// Out of line: inlined, ocml's fp64 pow needs ~60 VGPRs and set the register budget of every
// kernel that shades (the fused frame kernel spilled to scratch around it).
__device__ __attribute__((noinline)) float phong_pow_f64(float c, float p) {
  return (float)pow((double)c, (double)p);
}
__device__ __forceinline__ float phong_pow(float c, float p) {
  if (p == 1.0f) return c;
  return phong_pow_f64(c, p);
}

// The colour of a primary hit (leaf, t) of pixel (px, py): ambient, then per unoccluded light
// diffuse and specular, in the reference's order.  occluded(li): light li's shadow bit.
template <bool SPHERES, typename Occ>
__device__ __forceinline__ V3 shade_hit(const RenderParams& P, const DevPrim* __restrict__ prims,
                                        const float* __restrict__ normals,
                                        const DevMaterial* __restrict__ mats,
                                        const DevLight* __restrict__ lights, int leaf, V3 p,
                                        Occ occluded, int hand_li = -1,
                                        V3 hand_wi = {0.0f, 0.0f, 0.0f},
                                        unsigned long long* loads_done = nullptr) {
  (void)loads_done;  // (RT_DIAG: the time at which the normal and the material are back)
  V3 color = v3(0.0f, 0.0f, 0.0f);
  const V3 e = ld3(P.cam_e);
  const float4 nm = *reinterpret_cast<const float4*>(normals + 4 * leaf);
  const bool tri = !SPHERES || prims[leaf].kind == kPrimTriangle;
  const V3 n = tri ? v3(nm.x, nm.y, nm.z) : normalize_shared(p - ld3(prims[leaf].v0));
  const DevMaterial& m = mats[__float_as_int(nm.w)];
#ifdef RT_DIAG
  if (loads_done) {  // every material field now, so that the stamp closes the dependent loads
    float a = m.ambient[0], d = m.diffuse[0], sp = m.specular[0], ph = m.phong_exponent;
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(d), "+v"(sp), "+v"(ph) : : "memory");
    *loads_done = clock_now();
  }
#endif
  const V3 w0 = normalize_shared(e - p);  // (ray.o - intersection_point).normalize()
  color = color + ld3(m.ambient) * ld3(P.ambient);
  for (int li = 0; li < P.num_lights; li++) {
    if (occluded(li)) continue;
    const DevLight& Lt = lights[li];
    const V3 ld = ld3(Lt.position) - p;
    // hand_li (wave-uniform, the frame kernel's last light): the caller holds normalize(ld)
    const V3 wi = li == hand_li ? hand_wi : normalize_shared(ld);
    const float dist = length(ld);
    const V3 I = ld3(Lt.intensity);
    const float d2 = dist * dist;
    const float cos_d = dot(n, wi);
    const float cos_s = __builtin_fmaxf(dot(n, normalize_shared(w0 + wi)), 0.0f);
    const float pw = phong_pow(cos_s, m.phong_exponent);
    V3 diff, spec;  // added in the reference's order: diffuse, then specular
    light_quotients((ld3(m.diffuse) * I) * cos_d, (ld3(m.specular) * I) * pw, d2, diff, spec);
    color = (color + diff) + spec;
  }
  return color;
}

template <bool SPHERES>
__device__ __forceinline__ void shade_pixel(const RenderParams& P,
                                            const DevPrim* __restrict__ prims,
                                            const float* __restrict__ normals,
                                            const DevMaterial* __restrict__ mats,
                                            const DevLight* __restrict__ lights, int sel,
                                            const WaveLeafLds& L, const ShadowHand& hand,
                                            float* stage = nullptr) {
  const PacketPixel q = wave_pixel(P, L);  // (pair_rows: never a quadrant wave, L.sub is -1)
  const size_t pix = (size_t)sel * (kTile * kTile) + q.lane;
  DIAG(const unsigned long long s0 = clock_now());
  // the leaf waits in the lane's key (-1 a miss, -2 no pixel); t went into the parked point
  int2_t rec;
  rec.x = (int)key_words(L, lane_id())[0];
  rec.y = 0;
#ifdef RT_DIAG
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(rec.x), "+v"(rec.y) : : "memory");
  const unsigned long long s1 = clock_now();
  unsigned long long s2 = s1;
#endif
  const bool valid = q.own && hit_leaf(rec) != -2;
  const bool hit = q.own && hit_leaf(rec) >= 0;
  // a lone occlusion word is the shadow phase's register (0 without lights: no shadow phase)
  const bool occ_reg = P.occ_words == 1;
  if (P.records) {  // RT_TILE_RECORDS: the pixel record instead of its colour (rt_resolve_*)
    if (!q.own || (!P.tile_major && !valid)) return;
    unsigned r = kRecOutside;
    if (hit) {
      const unsigned bits = occ_reg ? hand.bits : P.occ[pix * P.occ_words];
      r = (unsigned)hit_leaf(rec) | ((bits & kRecLightMask) << kRecLightShift);
    } else if (valid) {
      r = kRecMiss;
    }
    unsigned* o = reinterpret_cast<unsigned*>(P.out);
    o[P.tile_major ? pix : (size_t)q.py * P.width + q.px] = r;  // tile-major, or row-major
    return;
  }
  V3 color = v3(0.0f, 0.0f, 0.0f);
  if (hit) {
    const unsigned* occ = P.occ + pix * P.occ_words;
    const V3 p = parked_point(L, lane_id());
    color = shade_hit<SPHERES>(
        P, prims, normals, mats, lights, hit_leaf(rec), p,
        [&](int li) {
          const unsigned word = occ_reg ? hand.bits : occ[li >> 5];
          return ((word >> (li & 31)) & 1u) != 0;
        },
        P.num_lights - 1, hand.wi
#ifdef RT_DIAG
        , &s2
#endif
    );
  } else if (valid) {
    color = ld3(P.background);  // primary miss: max_recursion_depth == depth
  }
  if (valid && stage) {  // pair_rows: the colour waits in LDS for the workgroup's row writes
    stage[3 * q.lane] = 0.0f + color.x;
    stage[3 * q.lane + 1] = 0.0f + color.y;
    stage[3 * q.lane + 2] = 0.0f + color.z;
  } else if (valid) {
    float* o;
    if (P.tile_major)
      o = P.out + 3 * pix;
    else
      o = P.out + 3 * ((size_t)q.py * P.width + q.px);
    o[0] = 0.0f + color.x;  // Pixel::add_color(color, 1) onto a zeroed pixel
    o[1] = 0.0f + color.y;
    o[2] = 0.0f + color.z;
  } else if (P.tile_major && q.own) {
    float* o = P.out + 3 * pix;
    o[0] = o[1] = o[2] = 0.0f;
  }
#ifdef RT_DIAG
  {  // the wave's latest material return closes its loads (a lane without a hit has none)
    unsigned long long s3 = clock_now();
    for (int o = 32; o; o >>= 1) {
      const unsigned long long other = __shfl_xor(s2, o, 64);
      s2 = other > s2 ? other : s2;
    }
    if (lane_id() == 0) {
      atomicAdd(&g_phase[kPhCycShadeRecord], s1 - s0);
      atomicAdd(&g_phase[kPhCycShadeLoads], s2 - s1);
      atomicAdd(&g_phase[kPhCycShadeMath], s3 - s2);
    }
  }
#endif
}

// pair_rows (rt_render into pinned host memory): the frame kernel's stores cross PCIe, where a
// wave's 8 rows of 96 B each end in a half-filled 64-B line.  The workgroup's two tiles (a 2x1
// unit, tx even) instead leave their colours in their waves' LDS; the second wave to arrive
// writes both tiles as 8 rows of 192 B — whole 64-B lines, 16-B stores.  (Same values, same
// pixels: only who stores them changes.)
// (launch_variant takes pair_rows only with two-wave workgroups; RT_TRACE_WAVES 1 and 4 still build)
static_assert(kTraceWaves != 2 || (kBlockW == 2 && kBlockH == 1),
              "pair_write: a workgroup is two tiles of one tile row");
__device__ __forceinline__ void pair_write(const RenderParams& P, WaveLeafLds* lds, int* arrived) {
  __threadfence_block();  // this wave's staged colours before its arrival
  int first = 0;
  if (lane_id() == 0) first = atomicAdd(arrived, 1) == 0;
  if (__builtin_amdgcn_readfirstlane(first)) return;  // the partner writes both tiles
  __threadfence_block();
  const int w = (int)threadIdx.x >> 6;
  const int tx0 = uniform(lds[w].tx) - w, ty = uniform(lds[w].ty);  // the unit's left tile
  for (int f = lane_id(); f < 96; f += 64) {  // 8 rows x 12 float4
    const int r = f / 12, k = f % 12;
    const int lr = ty * kTile + r;
    if (lr >= P.rows) continue;
    const float* src = reinterpret_cast<const float*>(lds[k / 6].q) + r * 24 + (k % 6) * 4;
    const size_t y = (size_t)(P.row0 + lr * P.row_stride);
    float4* dst = reinterpret_cast<float4*>(P.out + 3 * (y * P.width + (size_t)tx0 * kTile) + 4 * k);
    *dst = make_float4(src[0], src[1], src[2], src[3]);
  }
}

// ------------------------------------------------------------------ recursion (f1)
// HW2/Scene.cpp:88-196 with MaxRecursionDepth > 0: mirror rays (:141-146) and dielectrics
// (:149-194, refract_ray :72-86).  Each lane walks its ray tree in the reference's post order
// with an explicit stack of frames in HBM (layout [level][field][lane]); traversal calls stay
// wave-uniform packet calls over the lanes' current rays.  The parent's colour is combined
// with each child result in the source's order: color += km (x) child; and for a dielectric
// color += k (x) (r*refl + (1-r)*trans), with r*refl held in the frame until trans returns.
enum : int {
  kFrColor = 0, kFrStage = 3, kFrP = 4, kFrN = 7, kFrW0 = 10, kFrD = 13, kFrT = 16,
  kFrMat = 17, kFrDepth = 18, kFrMedium = 19, kFrK = 20, kFrR = 23, kFrA = 24, kFrFields = 28
};
enum : int {
  kStStart = 0, kStMirrorWait = 1, kStRefr = 2, kStTirWait = 3, kStReflWait = 4,
  kStTransWait = 5, kStDone = 6
};

struct FrameRef {
  float* base;
  size_t stride;  // floats between fields (= lanes in the launch)
  __device__ __forceinline__ float& f(int field) const { return base[(size_t)field * stride]; }
  __device__ __forceinline__ V3 v(int field) const { return v3(f(field), f(field + 1), f(field + 2)); }
  __device__ __forceinline__ void put(int field, V3 a) const {
    f(field) = a.x;
    f(field + 1) = a.y;
    f(field + 2) = a.z;
  }
  __device__ __forceinline__ int i(int field) const { return __float_as_int(f(field)); }
  __device__ __forceinline__ void put_i(int field, int x) const { f(field) = __int_as_float(x); }
};

// HW2/Scene.cpp:72-86
__device__ __forceinline__ bool refract_ray(V3 dir, V3 n, float idx, V3& out) {
  const float n_ratio = 1 / idx;
  const float cos_t = dot(v3(-dir.x, -dir.y, -dir.z), n);
  const float delta = 1 - (n_ratio) * (n_ratio) * (1 - (cos_t * cos_t));
  if (delta < 0.0f) return false;
  out = normalize((dir + n * cos_t) * n_ratio - n * __builtin_sqrtf(delta));
  return true;
}

// ------------------------------------------------------------------ instanced scenes
__device__ __forceinline__ bool query_ray_ok(V3 o, V3 d);  // (below, with the ray queries)
// A two-level walk.  The wave walks the TOP-LEVEL reference tree over the
// instances and the loose primitives with visit_node / advance and the exact box rule.  A loose
// primitive is tested in place.  An instance is wave-uniform: its record and its base mesh's
// descriptor come by scalar loads, the lanes that reached it test its world box (one more
// ancestor box) and take their ray through the inverse matrix — Matrix4x4::multiply's order, every
// product and sum rounded, the direction not normalised, so the local t is the world t — and the
// wave calls the ordinary closest_hit / occluded on a RenderParams view of the base mesh with only
// those lanes active.  The inner walk owns L.key and its own stack; the outer best
// (t, top-level position, mesh leaf) stays in registers.  A local ray that is no valid query ray
// misses the instance.
__device__ __forceinline__ V3 inst_point(const float* e, V3 p) {  // multiply(p, false), rows 0..2
  return v3(((e[3] + e[0] * p.x) + e[1] * p.y) + e[2] * p.z,
            ((e[7] + e[4] * p.x) + e[5] * p.y) + e[6] * p.z,
            ((e[11] + e[8] * p.x) + e[9] * p.y) + e[10] * p.z);
}
__device__ __forceinline__ V3 inst_vector(const float* e, V3 d) {  // multiply(d, true)
  return v3(((0.0f + e[0] * d.x) + e[1] * d.y) + e[2] * d.z,
            ((0.0f + e[4] * d.x) + e[5] * d.y) + e[6] * d.z,
            ((0.0f + e[8] * d.x) + e[9] * d.y) + e[10] * d.z);
}
// The normal matrix is the inverse's transpose: row i of it is column i of `e`.
__device__ __forceinline__ V3 inst_normal(const float* e, V3 n) {
  return v3(((0.0f + e[0] * n.x) + e[4] * n.y) + e[8] * n.z,
            ((0.0f + e[1] * n.x) + e[5] * n.y) + e[9] * n.z,
            ((0.0f + e[2] * n.x) + e[6] * n.y) + e[10] * n.z);
}

// The records of a reached instance and of its base mesh by scalar loads, as load_node8 takes a
// wide node: the kernel stores results, so the compiler would fetch them per lane.  (The first 16
// words of a DevInstance are its matrix rows and box[0..3]; the next 8 the rest.)
typedef int v8i __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void load_instance(const DevInstance* __restrict__ instances, int index,
                                              v16i& a, v8i& b) {
  const unsigned off = (unsigned)index * (unsigned)sizeof(DevInstance), off2 = off + 64u;
  asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx8 %1, %2, %4\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(b) : "s"(instances), "s"(off), "s"(off2) : "memory");
}
__device__ __forceinline__ DevNode load_top_node(const DevNode* __restrict__ nodes, int index) {
  const unsigned off = (unsigned)index << 6;
  v16i a;
  asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a) : "s"(nodes), "s"(off) : "memory");
  return __builtin_bit_cast(DevNode, a);
}
template <typename T>
__device__ __forceinline__ const T* word_pointer(int lo, int hi) {
  return reinterpret_cast<const T*>(((uint64_t)(unsigned)hi << 32) | (uint64_t)(unsigned)lo);
}

// The base mesh as the scene a walk sees: a, b the two halves of its DevMesh record.
__device__ __forceinline__ RenderParams mesh_view(const RenderParams& P, const v16i& a,
                                                  const v16i& b) {
  RenderParams V = P;
  V.nodes = word_pointer<DevNode>(a[0], a[1]);
  V.leaves = word_pointer<DevLeaf>(a[2], a[3]);
  V.prims = word_pointer<DevPrim>(a[4], a[5]);
  V.anc = word_pointer<DevAncestry>(a[6], a[7]);
  V.normals = word_pointer<float>(a[8], a[9]);
  V.root_kind = a[12];
  V.root_ref = a[13];
  V.accel_root = a[14];
  V.accel_stride = a[15];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    V.root_box[k] = __int_as_float(b[k]);
    V.accel_box[k] = __int_as_float(b[6 + k]);
  }
  V.quot_ok = b[12];
  return V;
}
static_assert(offsetof(DevMesh, root_kind) == 48 && offsetof(DevMesh, root_box) == 64 &&
              offsetof(DevMesh, quot_ok) == 112 && offsetof(DevInstance, box) == 48 &&
              offsetof(DevInstance, mesh) == 72, "the word indices above");

// OCC == false: the closest hit of every valid lane's ray w — bt, and btop / bleaf (the top-level
// position and, under an instance, the mesh leaf; -1: a miss).  OCC == true: returns whether some
// reachable primitive has 0 < t < thr; a lane found occluded leaves the walk.
// MOTION (the motion kernels only): the lane's ray has the time tau.  A moving
// instance (DevInstance::moving, wave-uniform) is entered through the lane's own inverse of
// T(tau v) * M and then exactly as a static one; a kPrimMovingSphere is tested on its local ray
// (Sphere.h:76-154; no box of its own, as there).  Mo->fast replaces FAST at run time.
template <bool FAST, bool SPHERES, bool OCC, bool MOTION = false>
__device__ __forceinline__ bool inst_walk(const RenderParams& P, const InstParams& T,
                                          WaveLeafLds& L, const LaneRay& w, bool valid, float thr,
                                          float& bt, int& btop, int& bleaf, Diag& dg,
                                          const MotionParams* Mo = nullptr, float tau = 0.0f) {
  bt = RT_INF;
  btop = -1;
  bleaf = -1;
  bool occ = false;
  if (OCC) valid = valid && thr > 0.0f;  // thr <= 0 (or NaN): nothing satisfies 0 < t < thr
  const bool lone = T.top_root_kind != kTopNode;  // the list is one object: its own rule
  uint64_t m, alive = ~0ull;
  int node = -1;
  if (lone) {
    m = ballot(valid);
  } else {
    float tn;
    bool acc, und;
    slab_fast<true>(T.top_box, w, tn, acc, und);
    m = ballot(valid && (acc || (und && box_exact(T.top_box, w))));
    node = 0;
  }
  if (!m) return false;
  WaveStack<false> st;
  for (;;) {
    int q0 = lone ? 0 : -1, q1 = -1;  // the top-level leaves the lanes of m test at this step
    int c0 = -1, c1 = -1;
    uint64_t m0 = 0ull, m1 = 0ull;
    float t0 = 0.0f, t1 = 0.0f;
    if (!lone) {
      const DevNode N = load_top_node(T.top_nodes, node);
      bool h0, h1;
      visit_node<true>(N, w, lane_in(m), h0, h1, t0, t1);
      c0 = N.child[0];
      c1 = N.child[1];
      // a leaf child has no box: every lane in the node tests it; inner children are entered
      if (c0 < 0) q0 = ~c0; else m0 = ballot(h0) & alive;
      if (c1 < 0) q1 = ~c1; else m1 = ballot(h1) & alive;
    }
#pragma nounroll
    for (int k = 0; k < 2; k++) {
      const int pos = k ? q1 : q0;
      if (pos < 0) continue;
      const bool in = lane_in(m & alive);
      const DevPrim* __restrict__ tp = T.top_prims + pos;
      const int kind = uniform(tp->kind);
      float t = RT_INF;
      int leaf = -1;
      bool hit;
      if (kind == kPrimInstance) {
        v16i ia, ma, mb;
        v8i ib;
        load_instance(T.instances, uniform(tp->material), ia, ib);
        load_node8(reinterpret_cast<const DevNode*>(T.meshes), 2 * ib[2], ma, mb);  // (128 B each)
        float inv[12];
#pragma unroll
        for (int e = 0; e < 12; e++) inv[e] = __int_as_float(ia[e]);
        if constexpr (MOTION) {
          if (ib[4]) {  // it moves: each lane its own inverse (NaNs where det == 0: a miss below)
            const DevMotionInstance& mi = Mo->instances[uniform(tp->material)];
            motion_inverse(mi.fwd, mi.vel, tau, inv);
          }
        }
        const float box[6] = {__int_as_float(ia[12]), __int_as_float(ia[13]),
                              __int_as_float(ia[14]), __int_as_float(ia[15]),
                              __int_as_float(ib[0]), __int_as_float(ib[1])};
        float tn;
        bool acc, und;
        slab_fast<true>(box, w, tn, acc, und);
        const bool boxed = in && (acc || (und && box_exact(box, w)));
        V3 lo = inst_point(inv, w.o), ld = inst_vector(inv, w.d);
        const bool go = boxed && query_ray_ok(lo, ld);
        if (!ballot(go)) continue;
        if (!go) {  // an idle lane still takes part in the wave-wide steps: a harmless ray
          lo = v3(0.0f, 0.0f, 0.0f);
          ld = v3(0.0f, 0.0f, 1.0f);
        }
        const RenderParams V = mesh_view(P, ma, mb);
        const LaneRay lr = make_ray(lo, ld, V.quot_ok);
        bool culled = FAST && V.accel_root >= 0;
        if constexpr (MOTION) culled = culled && Mo->fast;
        if (OCC) {
          bool o;
          if (culled)
            o = occluded<true, true, false, false>(V, V.nodes, nullptr, L, lr, go, thr, dg);
          else
            o = occluded<true, false, false, false>(V, V.nodes, nullptr, L, lr, go, thr, dg);
          occ |= go && o;
          hit = false;
        } else {
          if (culled)
            closest_hit<true, true, false, false>(V, V.nodes, nullptr, L, lr, go, t, leaf, dg);
          else
            closest_hit<true, false, false, false>(V, V.nodes, nullptr, L, lr, go, t, leaf, dg);
          // (0 < t by the leaf test; a one-face mesh's lone-root answer may still be t = inf,
          // which the top-level tree's leaf rule rejects)
          hit = go && leaf >= 0 && (lone || t < RT_INF);
        }
      } else {
        bool plain = true;
        if constexpr (MOTION) {
          if (kind == kPrimMovingSphere) {  // Sphere.h:76-154: sphere_test on the local ray
            plain = false;
            const DevMotionSphere& S = Mo->spheres[uniform(tp->material)];
            float inv[12];
#pragma unroll
            for (int e = 0; e < 12; e++) inv[e] = S.inv[e];
            if (S.moving) motion_inverse(S.fwd, S.vel, tau, inv);
            const V3 lo = inst_point(inv, w.o), ld = inst_vector(inv, w.d);
            const LaneRay lr = make_ray(lo, ld, 0);
            hit = in && query_ray_ok(lo, ld) && sphere_test(ld3(S.center), S.radius, lr, t);
          }
        }
        if (plain) hit = in && leaf_test<SPHERES>(T.top_prims, pos, w, t);
        // in the tree: the leaf rule 0 < t < inf; the lone object: its own answer as it is
        if (!lone) hit = hit && t > 0.0f && t < RT_INF;
        if (OCC) {
          occ |= hit && t > 0.0f && t < thr;
          hit = false;
        }
      }
      // HW2/HW3 BVH::intersect over the top level: the smaller t, at equal t the earlier leaf
      if (!OCC && hit && (t < bt || btop < 0 || (t == bt && pos < btop))) {
        bt = t;
        btop = pos;
        bleaf = leaf;
      }
    }
    if (lone) break;
    if (OCC) {
      alive &= ~ballot(occ);
      m0 &= alive;
      m1 &= alive;
    }
    if (!advance(st, c0, c1, m0, m1, t0, t1, node, m, alive)) break;
  }
  return occ;
}


// What the ray-tree code takes for an instanced scene: nothing in the flat instantiations (NoInst,
// the default: their code is that of a build without instances), the scene's InstParams in the
// INST ones, where every closest hit and every shadow ray goes through inst_walk and
// Hit_data::normal / the material come from the instance (Mesh.h:69) or the loose primitive.
struct NoInst {
  static constexpr bool on = false;
  static constexpr bool motion = false;
};
struct InstArg {
  static constexpr bool on = true;
  static constexpr bool motion = false;
  InstParams T;
};
// A scene with motion: the lane's time too, one constant for its whole ray tree
// (HW3/src/Scene.cpp:153, 196, 226, 258: every secondary ray inherits it).
struct MotionArg {
  static constexpr bool on = true;
  static constexpr bool motion = true;
  InstParams T;
  MotionParams M;
  float tau;
};
template <bool FAST, bool SPHERES>
__device__ __forceinline__ bool inst_occluded(const RenderParams& P, const MotionArg& inst,
                                              WaveLeafLds& L, const LaneRay& sr, bool active,
                                              float thr, Diag& dg, std::bool_constant<FAST>,
                                              std::bool_constant<SPHERES>) {
  float t;
  int top, leaf;
  return inst_walk<FAST, SPHERES, true, true>(P, inst.T, L, sr, active, thr, t, top, leaf, dg,
                                              &inst.M, inst.tau);
}

// What a motion kernel reports of the winner of inst_walk (top >= 0), computed after the walk for
// the winner only: a moving object's inverse is built again from tau rather than carried across
// the inner walk.  The normal is (A^-1)^T.multiply(n, true).normalize(): of the mesh's flat normal
// (Mesh.h:69, 87), or of the local (o' + t d' - center).normalize() (Sphere.h:91, 133).
struct MotionHit {
  V3 n;
  int material, object, leaf, instance;
};
__device__ __forceinline__ MotionHit motion_hit(const InstParams& T, const MotionParams& M,
                                                const LaneRay& ray, float tau, float t, int top,
                                                int mesh_leaf) {
  const DevPrim& pr = T.top_prims[top];
  MotionHit h;
  if (pr.kind == kPrimInstance) {
    const DevInstance& I = T.instances[pr.material];
    const DevMesh& Me = T.meshes[I.mesh];
    float inv[12];
#pragma unroll
    for (int e = 0; e < 12; e++) inv[e] = I.inv[e];
    const DevMotionInstance& mi = M.instances[pr.material];  // (read only when it moves)
    if (I.moving) motion_inverse(mi.fwd, mi.vel, tau, inv);
    h.n = normalize(inst_normal(inv, ld3(Me.normals + 4 * mesh_leaf)));
    h.material = I.material;
    h.object = Me.object_base + Me.leaf_object[mesh_leaf];
    h.leaf = Me.leaf_base + mesh_leaf;
    h.instance = pr.material;
    return h;
  }
  if (pr.kind == kPrimMovingSphere) {
    const DevMotionSphere& S = M.spheres[pr.material];
    float inv[12];
#pragma unroll
    for (int e = 0; e < 12; e++) inv[e] = S.inv[e];
    if (S.moving) motion_inverse(S.fwd, S.vel, tau, inv);
    const V3 lo = inst_point(inv, ray.o), ld = inst_vector(inv, ray.d);
    h.n = normalize(inst_normal(inv, normalize((lo + ld * t) - ld3(S.center))));
    h.material = S.material;
  } else {
    h.n = pr.kind == kPrimTriangle ? ld3(T.top_normals + 4 * top)
                                   : normalize((ray.o + ray.d * t) - ld3(pr.v0));
    h.material = pr.material;
  }
  h.object = T.top_info[2 * top];
  h.leaf = T.top_info[2 * top + 1];
  h.instance = -1;
  return h;
}
// A shadow ray of an instanced scene's local shading.
template <bool FAST, bool SPHERES>
__device__ __forceinline__ bool inst_occluded(const RenderParams& P, const InstArg& inst,
                                              WaveLeafLds& L, const LaneRay& sr, bool active,
                                              float thr, Diag& dg, std::bool_constant<FAST>,
                                              std::bool_constant<SPHERES>) {
  float t;
  int top, leaf;
  return inst_walk<FAST, SPHERES, true>(P, inst.T, L, sr, active, thr, t, top, leaf, dg);
}

// Local shading of one hit (ambient + point lights with shadow rays), Scene.cpp:107-139.
// Wave-uniform: every lane calls it; `shade` selects the lanes that shade (hit, !in_medium).
// LIT (rt_shade_rays_lit*): after the scene's lights, the lane's own `own_k`
// light records at `own` (rt_light_sample: three 16-B words each).  A record whose position is
// not finite is absent; a light no shading lane of the wave has is skipped wave-wide.  A record
// with a non-zero normal is a sample of an emitter: both terms carry dot(-w_i, normal)
// (HW3/src/Scene.cpp:207-218), chosen per lane behind a select.
// TEX: `kd` is the lane's diffuse colour in place of the material's.
template <bool FAST, bool DEEP, bool SPHERES, bool LIT = false, typename Inst = NoInst,
          bool TEX = false>
__device__ __forceinline__ V3 local_color(const RenderParams& P, const DevNode* __restrict__ nodes,
                                          const DevPrim* __restrict__ prims,
                                          const DevMaterial* __restrict__ mats,
                                          const DevLight* __restrict__ lights, int* spill, WaveLeafLds& L,
                                          bool shade, V3 o, V3 p, V3 n, int mat, Diag& dg,
                                          unsigned long long& shadow_rays, const f4* own = nullptr,
                                          int own_k = 0, const Inst& inst = Inst{},
                                          [[maybe_unused]] V3 kd = V3{}) {
  V3 color = v3(0.0f, 0.0f, 0.0f);
  const DevMaterial& m = mats[shade ? mat : 0];
  auto diffuse = [&]() {
    if constexpr (TEX)
      return kd;
    else
      return ld3(m.diffuse);
  };
  if (shade) color = color + ld3(m.ambient) * ld3(P.ambient);
  const V3 w0 = shade ? normalize(o - p) : v3(0, 0, 0);
  for (int li = 0; li < P.num_lights; li++) {
    const DevLight& lt = lights[li];
    const V3 ld = ld3(lt.position) - p;
    const V3 wi = normalize(ld);
    const float dist = length(ld);
    const LaneRay sr = make_ray(p + wi * P.eps, wi, P.quot_ok);
    const float thr = dist - P.eps;
    bool occ;
    if constexpr (Inst::on) {
      occ = inst_occluded(P, inst, L, sr, shade, thr, dg, std::bool_constant<FAST>{},
                          std::bool_constant<SPHERES>{});
    } else {
      const bool sskip = ballot(shade && (sr.skip0 || sr.skip1 || sr.skip2)) != 0;
      occ = sskip ? occluded<true, FAST, DEEP, SPHERES>(P, nodes, spill, L, sr, shade, thr, dg)
                  : occluded<false, FAST, DEEP, SPHERES>(P, nodes, spill, L, sr, shade, thr, dg);
    }
    shadow_rays += __builtin_popcountll(ballot(shade));
    if (shade && !occ) {
      const V3 I = ld3(lt.intensity);
      const float d2 = dist * dist;
      color = color + ((diffuse() * I) * dot(n, wi)) / d2;
      const float cos_s = __builtin_fmaxf(dot(n, normalize(w0 + wi)), 0.0f);
      const float pw = (float)pow((double)cos_s, (double)m.phong_exponent);
      color = color + ((ld3(m.specular) * I) * pw) / d2;
    }
  }
  if constexpr (LIT) {
    for (int j = 0; j < own_k; j++) {
      f4 a = {0.0f, 0.0f, 0.0f, 0.0f}, b = a, c = a;
      if (shade) {
        a = own[3 * j];
        b = own[3 * j + 1];
        c = own[3 * j + 2];
      }
      const V3 lp = v3(a.x, a.y, a.z);
      const bool lit = shade && finite3(lp);
      if (!ballot(lit)) continue;
      const V3 ld = lit ? lp - p : v3(0.0f, 0.0f, 1.0f);  // (an idle lane: a harmless ray)
      const V3 wi = normalize(ld);
      const float dist = length(ld);
      const LaneRay sr = make_ray(p + wi * P.eps, wi, P.quot_ok);
      const float thr = dist - P.eps;
      bool occ;
      if constexpr (Inst::on) {
        occ = inst_occluded(P, inst, L, sr, lit, thr, dg, std::bool_constant<FAST>{},
                            std::bool_constant<SPHERES>{});
      } else {
        const bool sskip = ballot(lit && (sr.skip0 || sr.skip1 || sr.skip2)) != 0;
        occ = sskip ? occluded<true, FAST, DEEP, SPHERES>(P, nodes, spill, L, sr, lit, thr, dg)
                    : occluded<false, FAST, DEEP, SPHERES>(P, nodes, spill, L, sr, lit, thr, dg);
      }
      shadow_rays += __builtin_popcountll(ballot(lit));
      if (lit && !occ) {
        const V3 I = v3(b.x, b.y, b.z), en = v3(c.x, c.y, c.z);
        const bool point = (en.x == 0.0f) & (en.y == 0.0f) & (en.z == 0.0f);
        const float ic = dot(v3(-wi.x, -wi.y, -wi.z), en);
        const float d2 = dist * dist;
        const V3 kd = diffuse() * I, ks = ld3(m.specular) * I;
        color = color + ((point ? kd : kd * ic) * dot(n, wi)) / d2;
        const float cos_s = __builtin_fmaxf(dot(n, normalize(w0 + wi)), 0.0f);
        // the same (float)pow((double), (double)), out of line: a second inlined copy costs the
        // lean variants their fourth wave per SIMD
        const float pw = phong_pow_f64(cos_s, m.phong_exponent);
        color = color + ((point ? ks : ks * ic) * pw) / d2;
      }
    }
  }
  return color;
}

// Ray counts of one wave's ray trees (trace_tree): hits and shadow are wave totals, secondary is
// this lane's own.
struct TreeCounts {
  unsigned long long hits = 0, shadow = 0, secondary = 0;
};

// Scene::trace_ray(Ray(ro, rd, medium), depth) of every `active` lane: the lane's ray tree in the
// reference's post order.  Both callers run it: recursive_packet for a camera's pixel rays and
// query_radiance_kernel for the caller's own.  The lane's frames are
// frames[(level * kFrFields + field) * stride], `frames` already pointing at the lane's slot.
// t_first: Hit_data::t of the lane's first ray, +inf on a miss or an inactive lane.
// RECURSE = false (depth 0, or a scene without mirror or glass: no material can spawn a ray):
// closest hit, local shading or the miss rule, and no frame is read or written.
// LIT: the lane's own light records join every local shading of its tree (local_color).
// SMOOTH: the scene has a smooth mesh; a hit on one of its faces takes the interpolated vertex
// normal (triangle_normal) wherever Hit_data::normal is read.
// TEX: the scene has textures (SPHERES and SMOOTH are then both set, the leaf's flags deciding);
// a hit on a textured leaf takes HW4's texture step (textured_hit).
template <bool FAST, bool DEEP, bool SPHERES, bool RECURSE = true, bool LIT = false,
          bool SMOOTH = false, typename Inst = NoInst, bool TEX = false>
__device__ __forceinline__ V3 trace_tree(const RenderParams& P, const DevNode* __restrict__ nodes,
                                         const DevPrim* __restrict__ prims,
                                         const float* __restrict__ normals,
                                         const DevMaterial* __restrict__ mats,
                                         const DevLight* __restrict__ lights, int* spill,
                                         WaveLeafLds& L, float* frames, size_t stride, V3 ro, V3 rd,
                                         bool medium, int depth, bool active, float& t_first,
                                         TreeCounts& cnt, const SurfArg<SMOOTH>& surf,
                                         const f4* own = nullptr, int own_k = 0,
                                         const Inst& inst = Inst{},
                                         [[maybe_unused]] const TexArg<TEX>& tex = TexArg<TEX>{}) {
  static_assert(!TEX || (SPHERES && SMOOTH && !Inst::on), "TEX: flat scenes, SPHERES and SMOOTH set");
  auto frame = [&](int level) {
    return FrameRef{frames + (size_t)level * kFrFields * stride, stride};
  };
  int sp = 0;  // frames on this lane's stack
  V3 res = v3(0, 0, 0), out = v3(0, 0, 0);
  Diag dg;
  unsigned long long n_hits = 0, n_shadow = 0, n_secondary = 0;
  bool first = true;
  t_first = RT_INF;
  while (ballot(active)) {
    const LaneRay ray = make_ray(ro, rd, P.quot_ok);
    const bool skip = !Inst::on && ballot(active && (ray.skip0 || ray.skip1 || ray.skip2)) != 0;
    float t;
    int leaf;
    [[maybe_unused]] int mesh_leaf = -1;  // INST: `leaf` is the top-level position
    if constexpr (Inst::motion)
      inst_walk<FAST, SPHERES, false, true>(P, inst.T, L, ray, active, 0.0f, t, leaf, mesh_leaf, dg,
                                            &inst.M, inst.tau);
    else if constexpr (Inst::on)
      inst_walk<FAST, SPHERES, false>(P, inst.T, L, ray, active, 0.0f, t, leaf, mesh_leaf, dg);
    else if (skip)
      closest_hit<true, FAST, DEEP, SPHERES>(P, nodes, spill, L, ray, active, t, leaf, dg);
    else
      closest_hit<false, FAST, DEEP, SPHERES>(P, nodes, spill, L, ray, active, t, leaf, dg);
    const bool hit = active && leaf >= 0;
    if (first) {
      n_hits = __builtin_popcountll(ballot(hit));
      if (hit) t_first = t;
    }
    first = false;
    V3 p = v3(0, 0, 0), n = v3(0, 0, 0);
    int mat = 0;
    [[maybe_unused]] V3 kd = v3(0, 0, 0);   // TEX: the hit's diffuse colour, or its REPLACE_ALL texel
    [[maybe_unused]] bool replace_all = false;
    if (hit) {
      p = ray.o + ray.d * t;
      if constexpr (TEX) {
        const DevPrim& pr = prims[leaf];
        textured_hit(surf, tex, pr, leaf, ray, p, ld3(normals + 4 * leaf), mats, n, kd, replace_all);
        mat = replace_all ? tex.blank_material : pr.material;
      } else if constexpr (Inst::motion) {
        const MotionHit h = motion_hit(inst.T, inst.M, ray, inst.tau, t, leaf, mesh_leaf);
        n = h.n;
        mat = h.material;
      } else if constexpr (Inst::on) {
        const DevPrim& pr = inst.T.top_prims[leaf];
        if (pr.kind == kPrimInstance) {  // Mesh.h:69: the instance's normal matrix and material
          const DevInstance& I = inst.T.instances[pr.material];
          n = normalize(inst_normal(I.inv, ld3(inst.T.meshes[I.mesh].normals + 4 * mesh_leaf)));
          mat = I.material;
        } else {
          n = pr.kind == kPrimTriangle ? ld3(inst.T.top_normals + 4 * leaf)
                                       : normalize(p - ld3(pr.v0));
          mat = pr.material;
        }
      } else {
        const DevPrim& pr = prims[leaf];
        n = pr.kind == kPrimTriangle
                ? triangle_normal<SMOOTH>(surf, pr, leaf, ray, ld3(normals + 4 * leaf))
                : normalize(p - ld3(pr.v0));
        mat = pr.material;
      }
    }
    V3 local;
    if constexpr (TEX) {  // a REPLACE_ALL hit is its texel and nothing else (Scene.cpp:156-159)
      local = local_color<FAST, DEEP, SPHERES, LIT, Inst, true>(
          P, nodes, prims, mats, lights, spill, L, hit && !medium && !replace_all, ray.o, p, n, mat,
          dg, n_shadow, own, own_k, inst, kd);
      if (replace_all) local = kd;
    } else {
      local = local_color<FAST, DEEP, SPHERES, LIT, Inst>(
          P, nodes, prims, mats, lights, spill, L, hit && !medium, ray.o, p, n, mat, dg, n_shadow,
          own, own_k, inst);
    }
    if constexpr (!RECURSE) {  // the one ray of the tree (a miss: Scene.cpp:96-99)
      if (hit)
        out = local;
      else if (active && depth == P.max_depth)
        out = ld3(P.background);
      break;
    }
    if (active) {
      bool spawned = false;
      if (hit) {  // open a frame for this hit
        const FrameRef F = frame(sp++);
        F.put(kFrColor, local);
        F.put_i(kFrStage, kStStart);
        F.put(kFrP, p);
        F.put(kFrN, n);
        F.put(kFrW0, normalize(ray.o - p));
        F.put(kFrD, ray.d);
        F.f(kFrT) = t;
        F.put_i(kFrMat, mat);
        F.put_i(kFrDepth, depth);
        F.put_i(kFrMedium, medium ? 1 : 0);
      } else {  // a miss returns background only at the primary depth (Scene.cpp:96-99)
        res = depth == P.max_depth ? ld3(P.background) : v3(0.0f, 0.0f, 0.0f);
      }
      // run the post-order state machine until a new ray is spawned or the tree is done
      while (sp > 0 && !spawned) {
        const FrameRef F = frame(sp - 1);
        const int stage = F.i(kFrStage);
        const DevMaterial& m = mats[F.i(kFrMat)];
        const int fdepth = F.i(kFrDepth);
        V3 color = F.v(kFrColor);
        const V3 fn = F.v(kFrN), fp = F.v(kFrP), fw0 = F.v(kFrW0);
        const V3 wr = normalize(fn * (2 * dot(fn, fw0)) - fw0);  // (2 n.w0) n - w0
        int next = stage;
        if (stage == kStStart) {
          const bool mirror = m.mirror[0] != 0.0f || m.mirror[1] != 0.0f || m.mirror[2] != 0.0f;
          if (mirror && fdepth > 0) {
            ro = fp + wr * P.eps;
            rd = wr;
            medium = false;
            spawned = true;
            next = kStMirrorWait;
          } else {
            next = kStRefr;
          }
        } else if (stage == kStMirrorWait) {
          color = color + ld3(m.mirror) * res;
          next = kStRefr;
        } else if (stage == kStRefr) {
          const bool glass = m.transparency[0] != 0.0f || m.transparency[1] != 0.0f ||
                             m.transparency[2] != 0.0f;
          if (glass && fdepth > 0) {
            V3 td = v3(0.0f, 0.0f, 0.0f), k = v3(0.0f, 0.0f, 0.0f);
            float cos_t = 0.0f;
            const V3 dn = normalize(F.v(kFrD));
            const float idx = m.refraction_index;
            bool tir = false, entering;
            if (dot(dn, fn) < 0.0f) {
              refract_ray(dn, fn, idx, td);
              cos_t = dot(v3(-dn.x, -dn.y, -dn.z), fn);
              k = v3(1.0f, 1.0f, 1.0f);
              entering = true;
            } else {
              const double tt = (double)F.f(kFrT);
              k.x = (float)exp(-log((double)m.transparency[0]) * tt);
              k.y = (float)exp(-log((double)m.transparency[1]) * tt);
              k.z = (float)exp(-log((double)m.transparency[2]) * tt);
              entering = false;
              if (refract_ray(dn, v3(-fn.x, -fn.y, -fn.z), 1.0f / idx, td))
                cos_t = dot(td, fn);
              else
                tir = true;
            }
            F.put(kFrK, k);
            ro = fp + wr * P.eps;
            rd = wr;
            spawned = true;
            if (tir) {
              medium = true;
              next = kStTirWait;
            } else {
              const float r0 = (idx - 1) * (idx - 1) / ((idx + 1) * (idx + 1));
              const float r =
                  (float)((double)r0 + (double)(1 - r0) * pow((double)(1 - cos_t), 5.0));
              F.f(kFrR) = r;
              F.put(kFrA, td);  // transmission direction until the reflection returns
              medium = !entering;
              F.put_i(kFrMedium, entering ? 1 : 0);  // medium flag of the transmission ray
              next = kStReflWait;
            }
          } else {
            next = kStDone;
          }
        } else if (stage == kStTirWait) {
          color = color + F.v(kFrK) * res;
          next = kStDone;
        } else if (stage == kStReflWait) {
          const V3 td = F.v(kFrA);
          F.put(kFrA, res * F.f(kFrR));  // r * trace(reflection)
          ro = fp + td * P.eps;
          rd = td;
          medium = F.i(kFrMedium) != 0;
          spawned = true;
          next = kStTransWait;
        } else if (stage == kStTransWait) {
          color = color + F.v(kFrK) * (F.v(kFrA) + res * (1 - F.f(kFrR)));
          next = kStDone;
        }
        if (next == kStDone) {
          res = color;
          sp--;
          continue;
        }
        F.put(kFrColor, color);
        F.put_i(kFrStage, next);
        if (spawned) {
          depth = fdepth - 1;
          n_secondary++;
        }
      }
      if (!spawned) {  // the whole tree of this lane is done
        out = res;
        active = false;
      }
    }
  }
  cnt.hits = n_hits;
  cnt.shadow = n_shadow;
  cnt.secondary = n_secondary;
  return out;
}

template <bool FAST, bool DEEP, bool SPHERES, bool SMOOTH, typename Inst = NoInst, bool TEX = false>
__device__ __forceinline__ void recursive_packet(const RenderParams& P,
                                                 const DevNode* __restrict__ nodes,
                                                 const DevPrim* __restrict__ prims,
                                                 const float* __restrict__ normals,
                                                 const DevMaterial* __restrict__ mats,
                                                 const DevLight* __restrict__ lights, int sel,
                                                 int* spill, WaveLeafLds& L,
                                                 const SurfArg<SMOOTH>& surf,
                                                 const Inst& inst = Inst{},
                                                 const TexArg<TEX>& tex = TexArg<TEX>{}) {
  const PacketPixel q = packet_pixel(P, sel);
  const size_t lanes_total = (size_t)P.num_sel_tiles * (kTile * kTile);
  const size_t g = (size_t)sel * (kTile * kTile) + q.lane;
  const unsigned long long n_primary = __builtin_popcountll(ballot(q.valid));
  float t_first;
  TreeCounts cnt;
  // the camera's pixel ray at the scene's maximum depth
  const V3 out = trace_tree<FAST, DEEP, SPHERES, true, false, SMOOTH, Inst, TEX>(
      P, nodes, prims, normals, mats, lights, spill, L, P.frames + g, lanes_total, ld3(P.cam_e),
      primary_dir(P, q.px, q.py), false, P.max_depth, q.valid, t_first, cnt, surf, nullptr, 0, inst,
      tex);
  const unsigned long long n_hits = cnt.hits, n_shadow = cnt.shadow, n_secondary = cnt.secondary;
  if (q.valid) {
    float* o;
    if (P.tile_major)
      o = P.out + 3 * g;
    else
      o = P.out + 3 * ((size_t)q.py * P.width + q.px);
    o[0] = 0.0f + out.x;  // Pixel::add_color(color, 1) onto a zeroed pixel
    o[1] = 0.0f + out.y;
    o[2] = 0.0f + out.z;
  } else if (P.tile_major) {
    float* o = P.out + 3 * g;
    o[0] = o[1] = o[2] = 0.0f;
  }
  if (P.counters) {
    // n_secondary is per lane: reduce over the wave with atomics from every lane that spawned
    unsigned long long* c = counter_row(P, sel);
    if (n_secondary) atomicAdd(&c[kCntSecondary], n_secondary);
    if (q.lane == 0) {
      atomicAdd(&c[kCntPrimary], n_primary);
      atomicAdd(&c[kCntHits], n_hits);
      atomicAdd(&c[kCntShadow], n_shadow);
    }
  }
}

// The frame kernel hides its dependent node loads with occupancy: 7 waves/SIMD (<= 72 VGPRs),
// where the wide node's 32 SGPRs and the fp32 traversal state fit without scratch (at 8 the
// traversal spills).  (Macro: A/B builds, `make exp EXTRA=-D...`.)
#ifndef RT_FRAME_MIN_WAVES
#define RT_FRAME_MIN_WAVES 7
#endif
#define RT_FRAME_OCCUPANCY __attribute__((amdgpu_waves_per_eu(RT_FRAME_MIN_WAVES, 8)))

// XCD-aware block order: blocks b and b+8 share an XCD (round-robin dispatch), so hand each
// XCD a contiguous run of blocks — neighbouring packets share BVH nodes through its L2.
template <int W>
__device__ __forceinline__ int packet_index() {
  const int nb = (int)gridDim.x, b = (int)blockIdx.x;
  const int q = nb / 8, rem = nb % 8, x = b % 8;
  const int logical = (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + b / 8;
  return uniform(logical * W + ((int)threadIdx.x >> 6));
}

// Traversal workgroups: kTraceWaves packets, which the hardware keeps on ONE CU, so they share
// its scalar cache.  With P.tile_block the workgroup's packets form a kBlockW x kBlockH block
// of tiles (blocks row-major over the frame) instead of a run along a tile row: neighbouring
// rays walk the same nodes, and the cache serves them once.
// (kBlockW, kBlockH, and the packet index arithmetic — packet_sel, unit_sel, order_slot,
// sel_tile — are rt_internal.h's: the host works out their divisions, the PacketGeom argument.)

// ------------------------------------------------------------------ dispatch order
// Traversal kernels are LPT-scheduled: a packet's cost varies ~5x over a C3 frame (rays that
// graze the height field walk far more nodes), and a kernel's tail is set by the heavy packets
// that start last.  The hardware dispatcher hands out workgroups in block order as slots free
// up, so launching the units (one workgroup's kTraceWaves packets) heaviest first is a
// longest-processing-time schedule.  Orders never change results: every tile is written by
// exactly one wave.
//
// Selected tile of this wave in a traversal launch, and its quadrant (sub, -1: the whole
// packet): ordered (block b of the grid takes entry b / regions of region b mod regions' list,
// heaviest first: a unit, -1 = none, or -2 - (p kSplitEntries + j) = quadrants j kTraceWaves ..
// of logical packet p's tile, wave k taking quadrant j kTraceWaves + k), else the XCD-remapped
// block order.
__device__ __forceinline__ int dispatch_sel(const RenderParams& Q, const PacketGeom& G, int& sub) {
  const int w = (int)threadIdx.x >> 6;
  sub = -1;
  if (Q.use_order) {
    const int e = uniform(Q.unit_order[order_slot(Q, G, (int)blockIdx.x)]);
    if (e >= 0) return uniform(unit_sel(Q, G, e, w));
    if (e == -1) return -1;
    sub = ((-2 - e) % kSplitEntries) * kTraceWaves + w;
    const int p = (-2 - e) / kSplitEntries;  // the split tile's logical packet
    return uniform(unit_sel(Q, G, p / kTraceWaves, p % kTraceWaves));
  }
  const int p = packet_index<kTraceWaves>();
  const int sel = p < G.packets ? packet_sel(Q, G, p) : -1;
  return sel < Q.num_sel_tiles ? sel : -1;
}

// Units of region x: chunks c = x, x + regions, ... of order_chunk consecutive units.
__device__ __forceinline__ int region_units(const RenderParams& P, int x) {
  const int full = P.order_units / P.order_chunk, rem = P.order_units % P.order_chunk;
  int n = x < full ? ((full - 1 - x) / P.order_regions + 1) * P.order_chunk : 0;
  if (rem && full % P.order_regions == x) n += rem;
  return n;
}
__device__ __forceinline__ int region_unit(const RenderParams& P, int x, int i) {
  return (x + (i / P.order_chunk) * P.order_regions) * P.order_chunk + i % P.order_chunk;
}

constexpr int kOrderBuckets = 256;
__device__ __forceinline__ int cost_bucket(unsigned c) {  // 8 steps per octave
  c = c ? c : 1u;
  const int msb = 31 - __builtin_clz(c);
  const int frac = msb >= 3 ? (int)((c >> (msb - 3)) & 7u) : (int)((c << (3 - msb)) & 7u);
  return min(kOrderBuckets - 1, msb * 8 + frac);
}

// A unit holds its workgroup slot until its slowest packet ends, so it is ranked by its
// most expensive tile (ranking by the sum measured 14 % worse in a replay of measured
// per-tile times).
__device__ __forceinline__ unsigned unit_cost(const RenderParams& P, const PacketGeom& G, int u) {
  unsigned c = 0;
  for (int w = 0; w < kTraceWaves; w++) {
    const int sel = unit_sel(P, G, u, w);
    if (sel >= 0) c = max(c, P.tile_cost[sel]);
  }
  return c;
}

// One workgroup per region: a bucket sort of the region's units by cost, heaviest first (order
// inside a bucket is free), into unit_order[x * stride ..]; -1 pads the list to `stride`.
// 256 threads: with frames in flight the GPU is full of traversal waves, and a bigger workgroup
// waits for a CU with that many free wave slots (rocprof: 1024-thread order launches averaged
// 79 us, up to 373, beside other frames' traversal; the sort itself takes 8 us).
//
// Split: the heaviest units — at most order_split per region, each costing at
// least kSplitBuckets buckets (2^(kSplitBuckets/8)) above the region's median — are listed as
// kSplitEntries entries per tile, so each of their tiles gets kSplitEntries workgroups whose
// waves take one quadrant each.  Those tiles' costs are zeroed here: the next frame's quadrant waves
// add their times into them (the tile's cost = the sum of its quadrants).
constexpr int kOrderThreads = 256;
// Split tuning (A/B builds): threshold in buckets above the median (8 per octave: 11 = 2.6 x),
// tiles split per region at most (1 / RT_SPLIT_DIV of the region's tiles, at most kMaxSplit), and
// only in launches whose regions hold at most RT_SPLIT_MAX_TILES tiles (the shares of a frame
// split over GPUs: a whole frame's tail is already hidden by the frames in flight, and splitting
// adds work).  Counted in tiles, so the split covers the same share whatever the workgroup size.
#ifndef RT_SPLIT_BUCKETS
#define RT_SPLIT_BUCKETS 11
#endif
#ifndef RT_SPLIT_DIV
#define RT_SPLIT_DIV 16
#endif
#ifndef RT_SPLIT_MAX_TILES
#define RT_SPLIT_MAX_TILES 768
#endif
constexpr int kSplitBuckets = RT_SPLIT_BUCKETS;
constexpr int kMaxSplit = 128;  // tiles split per region at most
__global__ __launch_bounds__(kOrderThreads) void order_kernel(RenderParams P, PacketGeom G) {
  __shared__ int hist[kOrderBuckets];
  __shared__ int split_info[2];  // [0] = split threshold bucket, [1] = units split
  const int tid = (int)threadIdx.x, x = (int)blockIdx.x;
  const int n = region_units(P, x);
  int* out = P.unit_order + (size_t)x * P.order_stride;
  for (int i = tid; i < kOrderBuckets; i += kOrderThreads) hist[i] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += kOrderThreads)
    atomicAdd(&hist[cost_bucket(unit_cost(P, G, region_unit(P, x, i)))], 1);
  __syncthreads();
  if (tid < 64) {  // exclusive offsets, heaviest bucket first: one wave scans the 256 buckets
    const int lane = tid;
    int v[kOrderBuckets / 64], run = 0;
#pragma unroll
    for (int k = 0; k < kOrderBuckets / 64; k++) {
      v[k] = hist[kOrderBuckets - 1 - (lane * (kOrderBuckets / 64) + k)];
      run += v[k];
    }
    int x2 = run;  // inclusive scan of the lane totals
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x2, o, 64);
      if (lane >= o) x2 += y;
    }
    int base = x2 - run;
    // the median unit's bucket (heaviest first: where the running count passes n / 2), and
    // how many units lie kSplitBuckets or more above it
    int med = -1;
#pragma unroll
    for (int k = 0; k < kOrderBuckets / 64; k++) {
      const int bucket = kOrderBuckets - 1 - (lane * (kOrderBuckets / 64) + k);
      if (base <= n / 2 && n / 2 < base + v[k]) med = bucket;
      hist[bucket] = base;
      base += v[k];
    }
    const uint64_t has = ballot(med >= 0);
    if (has) {
      const int mb = __builtin_amdgcn_readlane(med, (int)__builtin_ctzll(has));
      const int thr = mb + kSplitBuckets;
      if (lane == 0) {
        // hist[] now holds each bucket's first rank: units in buckets >= thr have ranks
        // below hist[thr - 1]'s ... i.e. the first rank of the next lighter bucket
        const int heavy = thr > kOrderBuckets - 1 ? 0 : hist[thr - 1];
        split_info[0] = thr;
        split_info[1] = min(P.order_split, heavy);
      }
    } else if (lane == 0) {
      split_info[0] = kOrderBuckets;
      split_info[1] = 0;
    }
  }
  __syncthreads();
  const int nsplit = split_info[1];
  unsigned* snap = P.tile_cost + sched_snap_offset((unsigned long long)P.num_sel_tiles);
  for (int i = tid; i < n; i += kOrderThreads) {
    const int u = region_unit(P, x, i);
    for (int w = 0; w < kTraceWaves; w++) {  // this frame's costs, kept for rt_tile_costs
      const int sel = unit_sel(P, G, u, w);
      if (sel >= 0) snap[sel] = P.tile_cost[sel];
    }
    const int r = atomicAdd(&hist[cost_bucket(unit_cost(P, G, u))], 1);
    if (r < nsplit) {  // kSplitEntries entries per tile, -1 for a padding tile of an edge block
      for (int w = 0; w < kTraceWaves; w++) {
        const int sel = unit_sel(P, G, u, w);
        for (int j = 0; j < kSplitEntries; j++)
          out[kQuadrants * r + kSplitEntries * w + j] =
              sel >= 0 ? -2 - ((kTraceWaves * u + w) * kSplitEntries + j) : -1;
        if (sel >= 0) P.tile_cost[sel] = 0u;
      }
    } else {
      out[r + (kQuadrants - 1) * nsplit] = u;
    }
  }
  for (int i = n + (kQuadrants - 1) * nsplit + tid; i < P.order_stride; i += kOrderThreads)
    out[i] = -1;
}

// RT_TIMELINE (experiment builds only): every traversal wave records its start and end on the
// 100 MHz clock and its own tile, so tools/timeline.py can draw the occupancy curve of a launch.
#ifdef RT_TIMELINE
constexpr int kTimelineWaves = 1 << 18;
__device__ unsigned long long g_timeline[2][kTimelineWaves][3];
#define TL_BEGIN                                                   \
  int tl_sel = -1;                                                  \
  const unsigned long long tl0 = __builtin_amdgcn_s_memrealtime()
#define TL_SEL(x) tl_sel = (x)
#define TL_END(k)                                                                         \
  do {                                                                                    \
    const unsigned long long tl1 = __builtin_amdgcn_s_memrealtime();                      \
    const int wid = (int)blockIdx.x * (int)(blockDim.x >> 6) + ((int)threadIdx.x >> 6);   \
    if (lane_id() == 0 && wid < kTimelineWaves) {                                         \
      g_timeline[k][wid][0] = tl0;                                                        \
      g_timeline[k][wid][1] = tl1;                                                        \
      g_timeline[k][wid][2] = (unsigned)tl_sel;                                           \
    }                                                                                     \
  } while (0)
#else
#define TL_BEGIN
#define TL_SEL(x)
#define TL_END(k)
#endif

// One launch per frame: each wave runs its packet's primary traversal, its shadow rays and its
// shading back to back, so a frame is one kernel with one tail (round 4 chained primary ->
// order -> shadow -> shade kernels, each with its own tail: a 1/8 share of a C3 frame then took
// 0.16 ms one at a time).  The occlusion bits of a scene with more than 32 lights
// still go through the stream's scratch (the same lane writes, then reads them: program order),
// which keeps the register state of the three phases apart; the hit's leaf and point wait in the
// wave's LDS block (a lane is the same pixel's in every phase, in a quadrant wave too), and the
// last light's direction and a lone occlusion word stay in registers from the last shadow walk on
// (ShadowHand).  tile_cost: the whole packet's time.
template <bool FAST, bool DEEP, bool SPHERES>
__global__ __launch_bounds__(kTraceWaves * 64) RT_FRAME_OCCUPANCY void trace_frame_kernel(
    RenderParams P, const DevNode* __restrict__ nodes, const DevLight* __restrict__ lights,
    PacketGeom G) {
  extern __shared__ __attribute__((aligned(16))) int deep_stack[];
  __shared__ WaveLeafLds leaf_lds[kTraceWaves];
  int* spill = DEEP ? deep_stack + ((int)threadIdx.x >> 6) * kDeepWords * kDeepStack : nullptr;
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  __shared__ int pair_arrived;
  if (P.pair_rows) {
    if (threadIdx.x == 0) pair_arrived = 0;
    __syncthreads();
  }
  TL_BEGIN;
  DIAG(const unsigned long long cp = clock_now());
  const RenderParams& Q = fresh_params(P);
  int sub;
  const int sel = dispatch_sel(Q, G, sub);
  TL_SEL(sel);
  if (sel >= 0) {
    L.sub = sub;
    {  // the packet's tile, once: every later phase reads it back (wave_pixel)
      int tx, ty;
      sel_tile(Q, G, sel, tx, ty);
      L.tx = tx;
      L.ty = ty;
    }
    // the packet's start time waits in the wave's LDS block (kept in SGPRs across the
    // traversals it spilled; in an array of its own, the slot's address was a VGPR held, and
    // with the carried leaf queue spilled to scratch, across them): its low word, which gives
    // the elapsed ticks modulo 2^32 (43 s at 100 MHz)
    L.start = (unsigned)__builtin_amdgcn_s_memrealtime();
    DIAG(const unsigned long long c0 = clock_now());
    primary_packet<FAST, DEEP, SPHERES>(Q, nodes, sel, spill, L);
    DIAG(const unsigned long long c1 = clock_now());
    ShadowHand hand;
    if (fresh_params(P).num_lights > 0)
      shadow_packet<FAST, DEEP, SPHERES>(fresh_params(P), nodes, lights, sel, spill, L, hand);
    DIAG(const unsigned long long c2 = clock_now());
    const RenderParams& Ps = fresh_params(P);
    if (Ps.pair_rows) {
      shade_pixel<SPHERES>(Ps, Ps.prims, Ps.normals, Ps.materials, lights, sel, L, hand,
                           reinterpret_cast<float*>(L.q));
      pair_write(fresh_params(P), leaf_lds, &pair_arrived);
    } else {
      shade_pixel<SPHERES>(Ps, Ps.prims, Ps.normals, Ps.materials, lights, sel, L, hand);
    }
#ifdef RT_DIAG
    const unsigned long long c3 = clock_now();
    if (lane_id() == 0) {
      atomicAdd(&g_phase[kPhCycPrimTotal], c1 - c0);
      atomicAdd(&g_phase[kPhCycShadTotal], c2 - c1);
      atomicAdd(&g_phase[kPhCycShade], c3 - c2);
      atomicAdd(&g_phase[kPhCycFrame], c3 - c0);
      atomicAdd(&g_phase[kPhCycPrologue], c0 - cp);
      atomicAdd(&g_phase[kPhWaves], 1ull);
    }
#endif
    const RenderParams& Pw = fresh_params(P);
    if (Pw.tile_cost && lane_id() == 0) {  // the next frame's dispatch order
      const unsigned c = (unsigned)__builtin_amdgcn_s_memrealtime() - L.start;
      if (wave_sub(L) < 0)
        Pw.tile_cost[sel] = c;
      else  // a quadrant: the tile's cost is the sum of its quadrants' (zeroed by order_kernel)
        atomicAdd(&Pw.tile_cost[sel], c);
    }
  }
  TL_END(0);
}

template <bool FAST, bool DEEP, bool SPHERES, bool SMOOTH, bool TEX, typename... Surf>
__global__ __launch_bounds__(kWavesPerBlock * 64) void recursive_kernel(
    RenderParams P, const DevNode* __restrict__ nodes, const DevPrim* __restrict__ prims,
    const float* __restrict__ normals, const DevMaterial* __restrict__ mats,
    const DevLight* __restrict__ lights, Surf... surf) {
  static_assert(sizeof...(Surf) == (TEX ? 2 : SMOOTH ? 1 : 0),
                "SMOOTH kernels take one SurfArg<true>, TEX kernels a TexArg<true> after it");
  extern __shared__ __attribute__((aligned(16))) int deep_stack[];
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  const int sel = packet_index<kWavesPerBlock>();
  if (sel >= P.num_sel_tiles) return;
  int* spill = DEEP ? deep_stack + ((int)threadIdx.x >> 6) * kDeepWords * kDeepStack : nullptr;
  recursive_packet<FAST, DEEP, SPHERES, SMOOTH, NoInst, TEX>(
      P, nodes, prims, normals, mats, lights, sel, spill, leaf_lds[threadIdx.x >> 6],
      surf_of(surf...), NoInst{}, tex_of(surf...));
}

// recursive_kernel for an instanced scene: the same packets and ray trees, every
// walk through inst_walk.  (No DEEP variant: instanced scenes' trees fit the wave stack.)
template <bool FAST, bool SPHERES>
__global__ __launch_bounds__(kWavesPerBlock * 64) void inst_recursive_kernel(
    RenderParams P, const DevMaterial* __restrict__ mats, const DevLight* __restrict__ lights,
    InstArg inst) {
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  const int sel = packet_index<kWavesPerBlock>();
  if (sel >= P.num_sel_tiles) return;
  recursive_packet<FAST, false, SPHERES, false, InstArg>(P, nullptr, nullptr, nullptr, mats, lights,
                                                        sel, nullptr, leaf_lds[threadIdx.x >> 6],
                                                        surf_of(), inst);
}

// ... and for a scene with motion: frames render at time 0 (inst.tau, set by the
// host), so a moving object stands where its matrix puts it, through the moving branch's code.
__global__ __launch_bounds__(kWavesPerBlock * 64) void motion_recursive_kernel(
    RenderParams P, const DevMaterial* __restrict__ mats, const DevLight* __restrict__ lights,
    MotionArg inst) {
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  const int sel = packet_index<kWavesPerBlock>();
  if (sel >= P.num_sel_tiles) return;
  recursive_packet<true, false, true, false, MotionArg>(P, nullptr, nullptr, nullptr, mats, lights,
                                                        sel, nullptr, leaf_lds[threadIdx.x >> 6],
                                                        surf_of(), inst);
}

// marks (nullable): 4 events recorded before the frame kernel (or the recursive kernel), after
// it, after the order kernel and at the end (rt_set_kernel_timing).
static inline void mark(const hipEvent_t* marks, int k, hipStream_t stream) {
  if (marks) (void)hipEventRecord(marks[k], stream);
}

// Calls f(FAST, DEEP, SPHERES) with the three flags as std::bool_constants: the kernel variant
// of a frame, query or radiance launch.  (The branches' order is the variants' order in the code
// object: FAST ones first, and among them plain before DEEP before SPHERES.)
template <typename F>
static void dispatch_variant(bool fast, bool deep, bool spheres, F&& f) {
  auto pick = [](bool b, auto&& g) {
    if (!b)
      g(std::false_type{});
    else
      g(std::true_type{});
  };
  pick(!fast, [&](auto slow) {
    pick(deep, [&](auto de) {
      pick(spheres, [&](auto sp) { f(std::bool_constant<!decltype(slow)::value>{}, de, sp); });
    });
  });
}

// FAST walks the culling tree: only when the scene has one (a root primitive or a tree of one
// treelet has none, accel_build.cpp).
static bool use_fast(const RenderParams& P, bool fast) {
  return fast && P.accel_root >= 0 && P.root_kind == kRootNode && P.leaves != nullptr;
}

// Dynamic LDS of a workgroup of `waves` waves: the DEEP variants' per-wave stacks.
template <bool DEEP>
constexpr size_t deep_lds_bytes(int waves) {
  return DEEP ? sizeof(int) * kDeepWords * kDeepStack * waves : 0;
}

// Dispatch-order geometry of a traversal launch: units of one traversal
// workgroup, `regions` regions of `chunk`-unit chunks (tile_block: half a row of 2x1 blocks), LPT
// within each region.  Sets T's tile_block and order_* fields, the launch's unit count (tblocks)
// and the units per region; false: the launch runs in block order (no order kernel).
#ifndef RT_ORDER_MIN_TILES  // launches selecting fewer tiles run in block order (no order kernel)
#define RT_ORDER_MIN_TILES 0
#endif
static bool order_geometry(RenderParams& T, PacketGeom& G, int& tblocks, int& per_region) {
  // 2-D blocks of tiles for a selection of whole tile rows: the whole frame, or a row band
  // (dist_tiles.BandPlan: tiles tile_begin .. tile_begin + num_sel_tiles - 1)
  T.tile_block = whole_tile_rows(T);
  G = packet_geom(T);  // (order_regions is the caller's: nothing below changes a divisor)
  tblocks = (G.packets + kTraceWaves - 1) / kTraceWaves;
  per_region = 0;
  T.use_order = 0;
  if (!(T.tile_cost != nullptr && T.unit_order != nullptr && T.order_regions > 0 &&
        T.num_sel_tiles >= RT_ORDER_MIN_TILES))
    return false;
  T.order_units = tblocks;
  const int nbx = (T.tiles_x + kBlockW - 1) / kBlockW;
  if (T.order_chunk > 0)  // host-set: that many chunks per region
    T.order_chunk = max(1, (tblocks + T.order_regions * T.order_chunk - 1) / (T.order_regions * T.order_chunk));
  else
    T.order_chunk = T.tile_block ? max(1, (nbx + 1) / 2) : 64;
  const int chunks = (T.order_units + T.order_chunk - 1) / T.order_chunk;
  per_region = ((chunks + T.order_regions - 1) / T.order_regions) * T.order_chunk;
  // room for order_split units per region listed quadrant group by quadrant group
  const int region_tiles = per_region * kTraceWaves;
  T.order_split = region_tiles <= RT_SPLIT_MAX_TILES
                      ? max(1, min(kMaxSplit, region_tiles / RT_SPLIT_DIV) / kTraceWaves) : 0;
  T.order_stride = per_region + (kQuadrants - 1) * T.order_split;
  // the order lists end below the cost snapshot (sched layout: rt_internal.h sched_words_for)
  return (unsigned long long)(T.unit_order - reinterpret_cast<int*>(T.tile_cost)) +
             (unsigned long long)T.order_regions * T.order_stride <=
         sched_snap_offset((unsigned long long)T.num_sel_tiles);
}

// The cold order of a camera's whole frame (rt_api.hip seed_cold_orders): P's tile_cost holds
// the estimated tile costs; the order kernel lists the units heaviest first into P's
// unit_order, without split entries.  Returns 1 if the launch is ordered (a list was made).
int launch_cold_order(RenderParams P, hipStream_t stream) {
  int tblocks = 0, per_region = 0;
  PacketGeom G;
  if (P.num_sel_tiles <= 0 || !order_geometry(P, G, tblocks, per_region)) return 0;
  P.order_split = 0;
  P.order_stride = per_region;
  hipLaunchKernelGGL(order_kernel, dim3(P.order_regions), dim3(kOrderThreads), 0, stream, P, G);
  return hipGetLastError() == hipSuccess ? 1 : 0;
}

// The surface argument of a launch: f(std::true_type, the scene's surface data) for a scene with
// a smooth mesh (surf non-null), else f(std::false_type) — the flat kernels take none.
template <typename F>
static void with_surface(const SurfParams* surf, F&& f) {
  if (surf) {
    SurfArg<true> arg;
    static_cast<SurfParams&>(arg) = *surf;
    f(std::true_type{}, arg);
  } else {
    f(std::false_type{});
  }
}
// The two trailing arguments of a TEX launch (a textured scene always has surface data).
struct TexLaunch {
  SurfArg<true> surf;
  TexArg<true> tex;
  TexLaunch(const SurfParams& s, const TexParams& t) {
    static_cast<SurfParams&>(surf) = s;
    static_cast<TexParams&>(tex) = t;
  }
};

// Tests only (rt_test_visit_time_exp): when on, every frame launch takes 2^E = the largest power
// of two not above 2^rel times the root box's diagonal, instead of visit_time_exp's — far too
// small an E makes the slot test's upper clamp bind, which may only cost culling.
static std::atomic<int> g_test_t_exp_on{0}, g_test_t_exp_rel{0};
void set_test_visit_time_exp(int on, int rel) {
  g_test_t_exp_rel.store(rel);
  g_test_t_exp_on.store(on);
}
static int test_visit_time_exp(const RenderParams& P, int e) {
  if (!g_test_t_exp_on.load() || P.accel_root < 0) return e;
  double diag2 = 0.0;
  for (int x = 0; x < 3; x++) {
    const double w = (double)P.accel_box[x + 3] - (double)P.accel_box[x];
    diag2 += w * w;
  }
  if (!(diag2 > 0.0 && diag2 < 1e300)) return e;
  int fl = 0;
  (void)std::frexp(std::sqrt(diag2), &fl);  // diag = f 2^fl, f in [1/2, 1)
  return std::max(-kVisitTimeExpMax, std::min(kVisitTimeExpMax, fl - 1 + g_test_t_exp_rel.load()));
}

template <bool FAST, bool DEEP, bool SPHERES>
static void launch_variant(const RenderParams& P, int blocks, const hipEvent_t* marks,
                           const SurfParams* surf, const TexParams* tex, hipStream_t stream) {
  const DevNode* nodes = P.nodes;
  const DevLight* lights = P.lights;
  if (P.frames) {  // recursive scenes: one kernel walks each pixel's ray tree
    const size_t lds = deep_lds_bytes<DEEP>(kWavesPerBlock);
    mark(marks, 0, stream);
    if (tex) {  // a textured scene: the TEX kernels, SPHERES and SMOOTH set whatever it holds
      const TexLaunch a(*surf, *tex);
      hipLaunchKernelGGL((recursive_kernel<FAST, DEEP, true, true, true>), dim3(blocks),
                         dim3(kWavesPerBlock * 64), lds, stream, P, nodes, P.prims, P.normals,
                         P.materials, lights, a.surf, a.tex);
    } else {
      with_surface(surf, [&](auto sm, auto... arg) {
        hipLaunchKernelGGL((recursive_kernel<FAST, DEEP, SPHERES, decltype(sm)::value, false>),
                           dim3(blocks), dim3(kWavesPerBlock * 64), lds, stream, P, nodes, P.prims,
                           P.normals, P.materials, lights, arg...);
      });
    }
    mark(marks, 1, stream);
    mark(marks, 2, stream);
    mark(marks, 3, stream);
    return;
  }
  RenderParams T = P;
  int tblocks = 0, per_region = 0;
  PacketGeom G;
  bool ordered = order_geometry(T, G, tblocks, per_region);
  G.neg_t_exp = -test_visit_time_exp(T, -G.neg_t_exp);
  const size_t tlds = deep_lds_bytes<DEEP>(kTraceWaves);
  int oblocks = ordered ? T.order_regions * T.order_stride : tblocks;
  const RenderParams S = T;
  // one kernel per frame, dispatched by the previous frame's heavy-first order when there is one
  // (warm order: same selection, same stream), else — a camera's whole frame — by the order
  // seeded at scene creation (cold order, no split); the order kernel then sorts this frame's
  // packet costs for the next frame
  mark(marks, 0, stream);
  if (!ordered) T.tile_cost = nullptr;
  T.use_order = ordered && P.primary_order ? 1 : 0;
  if (ordered && !T.use_order && P.cold_order && P.num_sel_tiles == P.cold_tiles) {
    T.order_split = 0;
    T.order_stride = per_region;
    T.unit_order = const_cast<int*>(P.cold_order);
    T.use_order = 1;
    oblocks = T.order_regions * T.order_stride;
  }
  // every workgroup holds two tiles of one tile row (tiles_x even, whole 16-pixel rows)
  T.pair_rows = P.pair_rows && kTraceWaves == 2 && kBlockW == 2 && T.tile_block && !T.use_order &&
                !T.tile_major && !T.records && T.tiles_x % 2 == 0 && T.width % 16 == 0 &&
                (reinterpret_cast<uintptr_t>(T.out) & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL((trace_frame_kernel<FAST, DEEP, SPHERES>), dim3(T.use_order ? oblocks : tblocks),
                     dim3(kTraceWaves * 64), tlds, stream, T, nodes, lights, G);
  mark(marks, 1, stream);
  if (ordered) hipLaunchKernelGGL(order_kernel, dim3(S.order_regions), dim3(kOrderThreads), 0, stream, S, G);
  mark(marks, 2, stream);
  mark(marks, 3, stream);
}

// Gaussian splat of HW2/Scene.cpp:46-62 turned inside out: one thread per destination pixel
// gathers every contribution the reference adds to it, in the order a single-threaded
// render_image adds them (source rows, source columns, samples x-major), so the fp32 sums of
// Pixel::add_color are reproduced exactly; then Pixel::get_color's color / weight.
// (gaussian_filter: rt_internal.h, shared with the films of film_kernels.hip.)
__global__ __launch_bounds__(256) void msaa_resolve_kernel(MsaaResolveParams M) {
  const int ai = (int)(blockIdx.x * 16 + (threadIdx.x & 15));
  const int aj = M.row_lo + (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (ai >= M.width || aj >= M.row_hi) return;
  const int n = M.n, S = n * n;
  const size_t frame = (size_t)M.width * M.height * 3;
  float cr = 0.0f, cg = 0.0f, cb = 0.0f, wsum = 0.0f;
  for (int j = aj - 1; j < aj + 2; j++) {
    if (j < 0 || j >= M.height) continue;
    for (int i = ai - 1; i < ai + 2; i++) {
      if (i < 0 || i >= M.width) continue;
      unsigned u = minstd_state0(
          msaa_pixel_seed(M.seed, (unsigned long long)j * (unsigned)M.width + (unsigned)i));
      const float* src = M.samples + 3 * ((size_t)j * M.width + i);
      for (int k = 0; k < S; k++) {
        u = minstd_mulmod(u, kMinstdA);
        const float ex = minstd_uniform01(u);
        u = minstd_mulmod(u, kMinstdA);
        const float ey = minstd_uniform01(u);
        const float sample_x = ((float)(k / n) + ex) / (float)n;
        const float sample_y = ((float)(k % n) + ey) / (float)n;
        const float s_x = ((float)i + sample_x) - ((float)ai + 0.5f);
        const float s_y = ((float)j + sample_y) - ((float)aj + 0.5f);
        const float w = gaussian_filter(s_x, s_y, 1.0f / 3.0f);
        const float* c = src + (size_t)k * frame;
        cr = cr + c[0] * w;
        cg = cg + c[1] * w;
        cb = cb + c[2] * w;
        wsum = wsum + w;
      }
    }
  }
  float* o = M.out + 3 * ((size_t)aj * M.width + ai);
  o[0] = cr / wsum;
  o[1] = cg / wsum;
  o[2] = cb / wsum;
}

hipError_t launch_msaa_resolve(const MsaaResolveParams& M, hipStream_t stream) {
  if (M.row_hi <= M.row_lo) return hipSuccess;
  const dim3 grid((M.width + 15) / 16, (M.row_hi - M.row_lo + 15) / 16);
  hipLaunchKernelGGL(msaa_resolve_kernel, grid, dim3(256), 0, stream, M);
  return hipGetLastError();
}

// The gathered tiles of a multi-device frame back into rows (UntileParams).  Each 8-pixel row
// of a tile is 96 contiguous bytes in both layouts: six 16-B chunks, one per thread (a wave
// covers 10 tile rows); a tile row on the frame's right edge, or a frame whose rows are not
// 16-B aligned (width % 4 != 0), is copied by pixel instead.
// Gathered tile of frame tile t: rank r's slot tile k (false: a unit of rank 0 under skip_root).
__device__ __forceinline__ bool untile_slot(const UntileParams& U, int t, int tx, int ty, int& r,
                                            int& k) {
  int w = 0;
  const int u = U.blocks ? deal_block_index(U.tiles_x, tx, ty, w) : t;  // deal unit
  r = (u + U.tile_offset) % U.devices;
  if (U.skip_root && r == 0) return false;
  const int b = ((r - U.tile_offset) % U.devices + U.devices) % U.devices;  // rank r's first unit
  k = U.blocks ? 4 * ((u - b) / U.devices) + w : (u - b) / U.devices;  // slot tile
  return true;
}

// (nullptr: a unit of rank 0 under skip_root)
__device__ __forceinline__ const float* untile_src(const UntileParams& U, int t, int tx, int ty) {
  int r, k;
  if (!untile_slot(U, t, tx, ty, r, k)) return nullptr;
  return U.recv + (size_t)(r * U.slot + k) * (kTile * kTile * 3);
}

constexpr int kUntileChunks = 6;  // 16-B chunks per 8-pixel tile row
__global__ __launch_bounds__(256) void untile_kernel(UntileParams U) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long trow = i / kUntileChunks;  // tile row: tile * 8 + row in tile
  const int c = (int)(i - trow * kUntileChunks);
  if (trow >= (long long)U.tiles_total * kTile) return;
  const int t = (int)(trow >> 3), y = (int)(trow & 7);
  const int tx = t % U.tiles_x, ty = t / U.tiles_x;
  const int lr = ty * kTile + y, px0 = tx * kTile;
  if (lr >= U.rows) return;
  const float* src0 = untile_src(U, t, tx, ty);
  if (!src0) return;
  const float* src = src0 + y * (kTile * 3);
  float* dst = U.out + ((size_t)(U.row0 + lr * U.row_stride) * U.width + px0) * 3;
  if (px0 + kTile <= U.width && U.vec) {
    reinterpret_cast<float4*>(dst)[c] = reinterpret_cast<const float4*>(src)[c];
    return;
  }
  // edge tile row / unaligned frame: this thread's four floats, those inside the frame
  const int lim = (U.width - px0) * 3;
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int f = 4 * c + e;
    if (f < lim) dst[f] = src[f];
  }
}

hipError_t launch_untile(const UntileParams& U, hipStream_t stream) {
  if (U.tiles_total <= 0) return hipSuccess;
  const long long threads = (long long)U.tiles_total * kTile * kUntileChunks;
  hipLaunchKernelGGL(untile_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, U);
  return hipGetLastError();
}

// rt_resolve_device: the gathered pixel records of RT_TILE_RECORDS shares (rt_internal.h) into
// colours of the row-major frame — the shading the frame kernel would have done on the rank that
// traced them, done on the gathering rank.  One thread per pixel, 64 per tile, 4 tiles per
// workgroup.  The hit's t is re-derived by the intersection test the traversal ran (the same ray
// from the same camera arithmetic, the same primitive record, the same operations: the same
// bits), the hit point is o + t * d as trace_ray computes it, and shade_hit is the frame kernel's.
// The colour of pixel (px, py) from its record (not kRecOutside).
template <bool SPHERES>
__device__ __forceinline__ V3 resolve_pixel(const RenderParams& P, unsigned rec, int px, int py) {
  if (rec & kRecMiss) return ld3(P.background);
  const int leaf = (int)(rec & kRecLeafMask);
  const V3 e = ld3(P.cam_e), d = primary_dir(P, px, py);
  const LaneRay ray = make_ray(e, d, P.quot_ok);
  float th = 0.0f;
  (void)leaf_test<SPHERES>(P.prims, leaf, ray, th);
  const unsigned occ = (rec >> kRecLightShift) & kRecLightMask;
  return shade_hit<SPHERES>(P, P.prims, P.normals, P.materials, P.lights, leaf, e + d * th,
                            [&](int li) { return ((occ >> li) & 1u) != 0; });
}

// rt_resolve_rows: row-major pixel records (a row band's, received whole) into the row-major
// frame, rows [row_begin, row_end) of the camera's own frame; one thread per pixel, a patch of
// pixels per workgroup (256 consecutive pixels of a row measured slower).
#ifndef RT_RESOLVE_PW  // patch width (A/B builds); height 256 / width
#define RT_RESOLVE_PW 32
#endif
constexpr int kResolvePW = RT_RESOLVE_PW, kResolvePH = 256 / RT_RESOLVE_PW;
template <bool SPHERES>
__global__ __launch_bounds__(256) void resolve_rows_kernel(RenderParams P, const unsigned* rec,
                                                           int row_begin, int row_end) {
  // a 32 x 8 patch of pixels per workgroup: neighbouring rows' hits share primitives
  const int px = (int)blockIdx.x * kResolvePW + (int)(threadIdx.x % kResolvePW);
  const long long py = row_begin + (long long)blockIdx.y * kResolvePH + (threadIdx.x / kResolvePW);
  if (px >= P.width || py >= row_end) return;
  const size_t pix = (size_t)py * P.width + px;
  const V3 color = resolve_pixel<SPHERES>(P, rec[pix], px, (int)py);
  float* o = P.out + 3 * pix;
  o[0] = 0.0f + color.x;
  o[1] = 0.0f + color.y;
  o[2] = 0.0f + color.z;
}

hipError_t launch_resolve_rows(const RenderParams& P, const unsigned* rec, int row_begin,
                               int row_end, bool spheres, hipStream_t stream) {
  const long long n = (long long)(row_end - row_begin) * P.width;
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((P.width + kResolvePW - 1) / kResolvePW),
                  (unsigned)((row_end - row_begin + kResolvePH - 1) / kResolvePH));
  if (spheres)
    hipLaunchKernelGGL(resolve_rows_kernel<true>, grid, dim3(256), 0, stream, P, rec, row_begin, row_end);
  else
    hipLaunchKernelGGL(resolve_rows_kernel<false>, grid, dim3(256), 0, stream, P, rec, row_begin, row_end);
  return hipGetLastError();
}

template <bool SPHERES>
__global__ __launch_bounds__(256) void resolve_kernel(RenderParams P, UntileParams U) {
  const int t = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (t >= U.tiles_total) return;
  const int lane = (int)(threadIdx.x & 63);
  const int tx = t % U.tiles_x, ty = t / U.tiles_x;
  const int px = tx * kTile + (lane & 7), lr = ty * kTile + (lane >> 3);
  if (px >= U.width || lr >= U.rows) return;
  int r, k;
  if (!untile_slot(U, t, tx, ty, r, k)) return;
  const unsigned rec = reinterpret_cast<const unsigned*>(U.recv)[(size_t)(r * U.slot + k) * (kTile * kTile) + lane];
  if (rec & kRecOutside) return;
  const int py = U.row0 + lr * U.row_stride;
  const V3 color = resolve_pixel<SPHERES>(P, rec, px, py);
  float* o = U.out + 3 * ((size_t)py * U.width + px);
  o[0] = 0.0f + color.x;
  o[1] = 0.0f + color.y;
  o[2] = 0.0f + color.z;
}

hipError_t launch_resolve(const RenderParams& P, const UntileParams& U, bool spheres,
                          hipStream_t stream) {
  if (U.tiles_total <= 0) return hipSuccess;
  const dim3 grid((unsigned)((U.tiles_total + 3) / 4));
  if (spheres)
    hipLaunchKernelGGL(resolve_kernel<true>, grid, dim3(256), 0, stream, P, U);
  else
    hipLaunchKernelGGL(resolve_kernel<false>, grid, dim3(256), 0, stream, P, U);
  return hipGetLastError();
}

int max_supported_depth() { return kDeepStack; }

// ------------------------------------------------------------------ ray queries
// Caller-supplied rays (rt_trace_rays_device / rt_occluded_device): one lane per
// ray, 64 consecutive rays of the order in use per wave, through the same closest_hit / occluded
// as the frame kernels.  A ray with a non-finite component, or with every |d_i| < 1e-6 (the
// reference's rule would skip all three axes and test every leaf), is INVALID: its lane stays
// inactive and reports a miss / not occluded.
struct QueryRay {
  V3 o, d;
  float tmax;
  float time;  // rt_ray::pad as it lies: read by the motion kernels alone (load_motion_ray)
  bool in;     // i < n: the lane has a result slot
  bool valid;  // ... and a ray to trace
};

__device__ __forceinline__ bool query_ray_ok(V3 o, V3 d) {
  const bool tiny = (__builtin_fabsf(d.x) < kEps) & (__builtin_fabsf(d.y) < kEps) &
                    (__builtin_fabsf(d.z) < kEps);
  return finite3(o) && finite3(d) && !tiny;
}

// Ray index of this lane, and its result slot (perm[i], or i).
__device__ __forceinline__ long long query_index() {
  return (long long)blockIdx.x * (kWavesPerBlock * 64) + threadIdx.x;
}
__device__ __forceinline__ long long query_slot(const QueryParams& Q, long long i) {
  return Q.perm ? (long long)Q.perm[i] : i;
}

__device__ __forceinline__ QueryRay load_query_ray(const QueryParams& Q, long long i) {
  QueryRay q;
  q.in = i < Q.n;
  f4 a = {0.0f, 0.0f, 0.0f, 0.0f}, b = {0.0f, 0.0f, 1.0f, 0.0f};
  if (q.in) {
    const f4* p = reinterpret_cast<const f4*>(Q.rays) + 2 * query_slot(Q, i);
    a = p[0];
    b = p[1];
  }
  q.o = v3(a.x, a.y, a.z);
  q.d = v3(b.x, b.y, b.z);
  q.tmax = a.w;
  q.time = b.w;
  q.valid = q.in && query_ray_ok(q.o, q.d);
  if (!q.valid) {  // an idle lane still takes part in the wave-wide steps: a harmless ray
    q.o = v3(0.0f, 0.0f, 0.0f);
    q.d = v3(0.0f, 0.0f, 1.0f);
  }
  return q;
}

template <bool FAST, bool DEEP, bool SPHERES, bool SMOOTH, typename... Surf>
__global__ __launch_bounds__(kWavesPerBlock * 64) void query_closest_kernel(
    RenderParams P, QueryParams Q, const DevNode* __restrict__ nodes, Surf... surf) {
  static_assert(sizeof...(Surf) == (SMOOTH ? 1 : 0), "SMOOTH kernels take one SurfArg<true>");
  extern __shared__ __attribute__((aligned(16))) int deep_stack[];
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  if ((query_index() & ~63ll) >= Q.n) return;  // the whole wave is past the batch
  int* spill = DEEP ? deep_stack + ((int)threadIdx.x >> 6) * kDeepWords * kDeepStack : nullptr;
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_query_ray(Q, query_index());
  const LaneRay ray = make_ray(q.o, q.d, P.quot_ok);
  const bool any_skip = q.valid && (ray.skip0 || ray.skip1 || ray.skip2);
  Diag dg;
  float t;
  int leaf;
  if (ballot(any_skip))
    closest_hit<true, FAST, DEEP, SPHERES>(P, nodes, spill, L, ray, q.valid, t, leaf, dg);
  else
    closest_hit<false, FAST, DEEP, SPHERES>(P, nodes, spill, L, ray, q.valid, t, leaf, dg);
  f4 h0 = {RT_INF, __int_as_float(-1), __int_as_float(-1), __int_as_float(-1)};
  f4 h1 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q.valid && leaf >= 0) {
    const DevPrim& pr = P.prims[leaf];
    // Hit_data::normal: the flat normal (Triangle.cpp:14; a smooth mesh's face: the interpolated
    // vertex normal), or Sphere.h:42,50's (ray.point_at(t) - center).normalize()
    V3 n = !SPHERES || pr.kind == kPrimTriangle
               ? ld3(P.normals + 4 * leaf)
               : normalize((ray.o + ray.d * t) - ld3(pr.v0));
    if constexpr (SMOOTH) {
      if (!SPHERES || pr.kind == kPrimTriangle)
        n = triangle_normal<true>(surf_of(surf...), pr, leaf, ray, n);
    }
    h0 = (f4){t, __int_as_float(Q.leaf_object[leaf]), __int_as_float(pr.material),
              __int_as_float(leaf)};
    h1 = (f4){n.x, n.y, n.z, 0.0f};
  }
  const long long i = query_index();
  if (i < Q.n) {
    f4* out = reinterpret_cast<f4*>(Q.out) + 2 * query_slot(Q, i);
    out[0] = h0;
    out[1] = h1;
  }
}

template <bool FAST, bool DEEP, bool SPHERES>
__global__ __launch_bounds__(kWavesPerBlock * 64) void query_occluded_kernel(
    RenderParams P, QueryParams Q, const DevNode* __restrict__ nodes) {
  extern __shared__ __attribute__((aligned(16))) int deep_stack[];
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  if ((query_index() & ~63ll) >= Q.n) return;
  int* spill = DEEP ? deep_stack + ((int)threadIdx.x >> 6) * kDeepWords * kDeepStack : nullptr;
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_query_ray(Q, query_index());
  const LaneRay ray = make_ray(q.o, q.d, P.quot_ok);
  const bool any_skip = q.valid && (ray.skip0 || ray.skip1 || ray.skip2);
  Diag dg;
  // 0 < t < tmax; tmax <= 0 or NaN: never (occluded's own `thr > 0` test)
  const bool occ =
      ballot(any_skip)
          ? occluded<true, FAST, DEEP, SPHERES>(P, nodes, spill, L, ray, q.valid, q.tmax, dg)
          : occluded<false, FAST, DEEP, SPHERES>(P, nodes, spill, L, ray, q.valid, q.tmax, dg);
  const long long i = query_index();
  if (i < Q.n)
    reinterpret_cast<unsigned char*>(Q.out)[query_slot(Q, i)] = (q.valid && occ) ? 1 : 0;
}

// ------------------------------------------------------------------ instanced scenes: the query kernels
// (inst_walk and InstArg: before local_color)
template <bool FAST, bool SPHERES>
__global__ __launch_bounds__(kWavesPerBlock * 64) void inst_closest_kernel(RenderParams P,
                                                                           QueryParams Q,
                                                                           InstParams T) {
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  if ((query_index() & ~63ll) >= Q.n) return;  // the whole wave is past the batch
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_query_ray(Q, query_index());
  const LaneRay ray = make_ray(q.o, q.d, T.top_quot_ok);
  Diag dg;
  float t;
  int top, leaf;
  inst_walk<FAST, SPHERES, false>(P, T, L, ray, q.valid, 0.0f, t, top, leaf, dg);
  f4 h0 = {RT_INF, __int_as_float(-1), __int_as_float(-1), __int_as_float(-1)};
  f4 h1 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q.valid && top >= 0) {
    const DevPrim& pr = T.top_prims[top];
    if (pr.kind == kPrimInstance) {
      // Mesh.h:69: normalT.multiply(flat normal, true).normalize(); the instance's material
      const DevInstance& I = T.instances[pr.material];
      const DevMesh& M = T.meshes[I.mesh];
      const V3 n = normalize(inst_normal(I.inv, ld3(M.normals + 4 * leaf)));
      h0 = (f4){t, __int_as_float(M.object_base + M.leaf_object[leaf]),
                __int_as_float(I.material), __int_as_float(M.leaf_base + leaf)};
      h1 = (f4){n.x, n.y, n.z, __int_as_float(pr.material)};
    } else {
      const V3 n = !SPHERES || pr.kind == kPrimTriangle
                       ? ld3(T.top_normals + 4 * top)
                       : normalize((ray.o + ray.d * t) - ld3(pr.v0));
      h0 = (f4){t, __int_as_float(T.top_info[2 * top]), __int_as_float(pr.material),
                __int_as_float(T.top_info[2 * top + 1])};
      h1 = (f4){n.x, n.y, n.z, __int_as_float(-1)};
    }
  }
  const long long i = query_index();
  if (i < Q.n) {
    f4* out = reinterpret_cast<f4*>(Q.out) + 2 * query_slot(Q, i);
    out[0] = h0;
    out[1] = h1;
  }
}

template <bool FAST, bool SPHERES>
__global__ __launch_bounds__(kWavesPerBlock * 64) void inst_occluded_kernel(RenderParams P,
                                                                            QueryParams Q,
                                                                            InstParams T) {
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  if ((query_index() & ~63ll) >= Q.n) return;
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_query_ray(Q, query_index());
  const LaneRay ray = make_ray(q.o, q.d, T.top_quot_ok);
  Diag dg;
  float t;
  int top, leaf;
  const bool occ = inst_walk<FAST, SPHERES, true>(P, T, L, ray, q.valid, q.tmax, t, top, leaf, dg);
  const long long i = query_index();
  if (i < Q.n)
    reinterpret_cast<unsigned char*>(Q.out)[query_slot(Q, i)] = (q.valid && occ) ? 1 : 0;
}

// ------------------------------------------------------------------ scenes with motion: query kernels
//   The INST kernels with a time per lane: rt_ray::pad with RT_QUERY_RAY_TIME
// (M.ray_time), else 0.  A ray whose time is not finite is INVALID, as one with a non-finite
// component.  One instantiation each: loose spheres compiled in, the traversal mode a run-time
// choice (M.fast).
__device__ __forceinline__ QueryRay load_motion_ray(const QueryParams& Q, const MotionParams& M,
                                                    long long i) {
  QueryRay q = load_query_ray(Q, i);
  if (!M.ray_time) q.time = 0.0f;
  if (!(__builtin_fabsf(q.time) < RT_INF)) q.valid = false;
  if (!q.valid) {
    q.o = v3(0.0f, 0.0f, 0.0f);
    q.d = v3(0.0f, 0.0f, 1.0f);
    q.time = 0.0f;
  }
  return q;
}

__global__ __launch_bounds__(kWavesPerBlock * 64) void motion_closest_kernel(RenderParams P,
                                                                             QueryParams Q,
                                                                             InstParams T,
                                                                             MotionParams M) {
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  if ((query_index() & ~63ll) >= Q.n) return;  // the whole wave is past the batch
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_motion_ray(Q, M, query_index());
  const LaneRay ray = make_ray(q.o, q.d, T.top_quot_ok);
  Diag dg;
  float t;
  int top, leaf;
  inst_walk<true, true, false, true>(P, T, L, ray, q.valid, 0.0f, t, top, leaf, dg, &M, q.time);
  f4 h0 = {RT_INF, __int_as_float(-1), __int_as_float(-1), __int_as_float(-1)};
  f4 h1 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q.valid && top >= 0) {
    const MotionHit h = motion_hit(T, M, ray, q.time, t, top, leaf);
    h0 = (f4){t, __int_as_float(h.object), __int_as_float(h.material), __int_as_float(h.leaf)};
    h1 = (f4){h.n.x, h.n.y, h.n.z, __int_as_float(h.instance)};
  }
  const long long i = query_index();
  if (i < Q.n) {
    f4* out = reinterpret_cast<f4*>(Q.out) + 2 * query_slot(Q, i);
    out[0] = h0;
    out[1] = h1;
  }
}

__global__ __launch_bounds__(kWavesPerBlock * 64) void motion_occluded_kernel(RenderParams P,
                                                                              QueryParams Q,
                                                                              InstParams T,
                                                                              MotionParams M) {
  __shared__ WaveLeafLds leaf_lds[kWavesPerBlock];
  if ((query_index() & ~63ll) >= Q.n) return;
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_motion_ray(Q, M, query_index());
  const LaneRay ray = make_ray(q.o, q.d, T.top_quot_ok);
  Diag dg;
  float t;
  int top, leaf;
  const bool occ = inst_walk<true, true, true, true>(P, T, L, ray, q.valid, q.tmax, t, top, leaf,
                                                     dg, &M, q.time);
  const long long i = query_index();
  if (i < Q.n)
    reinterpret_cast<unsigned char*>(Q.out)[query_slot(Q, i)] = (q.valid && occ) ? 1 : 0;
}

// rt_debug_motion_inverse: the walk's own motion_inverse of one moving object's record at n times.
__global__ void motion_inverse_kernel(const float* __restrict__ fwd, const float* __restrict__ vel,
                                      const float* __restrict__ times, long long n,
                                      float* __restrict__ out12) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float inv[12];
  motion_inverse(fwd, vel, times[i], inv);
#pragma unroll
  for (int e = 0; e < 12; e++) out12[12 * i + e] = inv[e];
}

// Radiance of caller-supplied rays (rt_shade_rays_device): the layout of
// query_closest_kernel, and between the lane's two 16-B loads and its one 16-B store the ray tree
// of trace_tree from (o, d, R.in_medium, R.depth).  One launch covers the rays
// [R.first, Q.n) of the order in use (a chunk: R.first is a multiple of 64, so waves stay whole);
// a lane's frames sit at its slot within the chunk.  RECURSE = false touches no frame.
static_assert(kFrFields == kRadianceFrameFloats, "frame size the host sizes the scratch by");
#ifndef RT_RADIANCE_WAVES  // (A/B builds: waves per workgroup; measured in DESIGN.md §4.12)
#define RT_RADIANCE_WAVES kWavesPerBlock
#endif
#ifndef RT_RADIANCE_MIN_WAVES  // (A/B builds: an occupancy request, as RT_FRAME_MIN_WAVES; 0 = none)
#define RT_RADIANCE_MIN_WAVES 0
#endif
#if RT_RADIANCE_MIN_WAVES
#define RT_RADIANCE_OCCUPANCY __attribute__((amdgpu_waves_per_eu(RT_RADIANCE_MIN_WAVES, 8)))
#else
#define RT_RADIANCE_OCCUPANCY
#endif
constexpr int kRadianceWaves = RT_RADIANCE_WAVES;
// LIT (rt_shade_rays_lit_device): the ray's own light records, found by the
// ray's index in the caller's batch (its result slot), not by its place in the chunk or in the
// reordered order; shared records sit at index 0 for every ray.  LitArg<false> is empty.
template <bool FAST, bool DEEP, bool SPHERES, bool RECURSE, bool LIT, bool SMOOTH, bool TEX,
          typename... Surf>
__global__ __launch_bounds__(kRadianceWaves * 64) RT_RADIANCE_OCCUPANCY void query_radiance_kernel(
    RenderParams P, QueryParams Q, RadianceParams R, const DevNode* __restrict__ nodes,
    const DevPrim* __restrict__ prims, const float* __restrict__ normals,
    const DevMaterial* __restrict__ mats, const DevLight* __restrict__ lights, LitArg<LIT> lit,
    Surf... surf) {
  static_assert(sizeof...(Surf) == (TEX ? 2 : SMOOTH ? 1 : 0),
                "SMOOTH kernels take one SurfArg<true>, TEX kernels a TexArg<true> after it");
  extern __shared__ __attribute__((aligned(16))) int deep_stack[];
  __shared__ WaveLeafLds leaf_lds[kRadianceWaves];
  const long long slot = (long long)blockIdx.x * (kRadianceWaves * 64) + threadIdx.x;  // in the chunk
  const long long i = R.first + slot;
  if ((i & ~63ll) >= Q.n) return;  // the whole wave is past the batch
  int* spill = DEEP ? deep_stack + ((int)threadIdx.x >> 6) * kDeepWords * kDeepStack : nullptr;
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_query_ray(Q, i);
  const unsigned long long n_primary = __builtin_popcountll(ballot(q.valid));
  float t;
  TreeCounts cnt;
  const f4* own = nullptr;
  int own_k = 0;
  if constexpr (LIT) {
    const long long ray = q.in && !lit.shared ? query_slot(Q, i) : 0;
    own = reinterpret_cast<const f4*>(lit.lights) + 3 * (size_t)ray * (size_t)lit.k;
    own_k = lit.k;
  }
  const V3 c = trace_tree<FAST, DEEP, SPHERES, RECURSE, LIT, SMOOTH, NoInst, TEX>(
      P, nodes, prims, normals, mats, lights, spill, L, RECURSE ? R.frames + slot : nullptr,
      (size_t)R.lanes, q.o, q.d, R.in_medium != 0, R.depth, q.valid, t, cnt, surf_of(surf...), own,
      own_k, NoInst{}, tex_of(surf...));
  if (i < Q.n) {
    // Pixel::add_color(color, 1) onto a zeroed pixel; an invalid ray: (0, 0, 0, +inf)
    const f4 out = {0.0f + c.x, 0.0f + c.y, 0.0f + c.z, t};
    reinterpret_cast<f4*>(Q.out)[query_slot(Q, i)] = out;
  }
  if (P.counters) {
    unsigned long long* row = counter_row(P, (int)((i >> 6) % kCounterSlots));
    if (cnt.secondary) atomicAdd(&row[kCntSecondary], cnt.secondary);
    if (lane_id() == 0) {
      atomicAdd(&row[kCntPrimary], n_primary);
      atomicAdd(&row[kCntHits], cnt.hits);
      atomicAdd(&row[kCntShadow], cnt.shadow);
    }
  }
}

// query_radiance_kernel for an instanced scene.
template <bool FAST, bool SPHERES, bool RECURSE, bool LIT>
__global__ __launch_bounds__(kRadianceWaves * 64) void inst_radiance_kernel(
    RenderParams P, QueryParams Q, RadianceParams R, const DevMaterial* __restrict__ mats,
    const DevLight* __restrict__ lights, LitArg<LIT> lit, InstArg inst) {
  __shared__ WaveLeafLds leaf_lds[kRadianceWaves];
  const long long slot = (long long)blockIdx.x * (kRadianceWaves * 64) + threadIdx.x;
  const long long i = R.first + slot;
  if ((i & ~63ll) >= Q.n) return;  // the whole wave is past the batch
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_query_ray(Q, i);
  const unsigned long long n_primary = __builtin_popcountll(ballot(q.valid));
  float t;
  TreeCounts cnt;
  const f4* own = nullptr;
  int own_k = 0;
  if constexpr (LIT) {
    const long long ray = q.in && !lit.shared ? query_slot(Q, i) : 0;
    own = reinterpret_cast<const f4*>(lit.lights) + 3 * (size_t)ray * (size_t)lit.k;
    own_k = lit.k;
  }
  const V3 c = trace_tree<FAST, false, SPHERES, RECURSE, LIT, false, InstArg>(
      P, nullptr, nullptr, nullptr, mats, lights, nullptr, L, RECURSE ? R.frames + slot : nullptr,
      (size_t)R.lanes, q.o, q.d, R.in_medium != 0, R.depth, q.valid, t, cnt, surf_of(), own, own_k,
      inst);
  if (i < Q.n) {
    const f4 out = {0.0f + c.x, 0.0f + c.y, 0.0f + c.z, t};
    reinterpret_cast<f4*>(Q.out)[query_slot(Q, i)] = out;
  }
  if (P.counters) {
    unsigned long long* row = counter_row(P, (int)((i >> 6) % kCounterSlots));
    if (cnt.secondary) atomicAdd(&row[kCntSecondary], cnt.secondary);
    if (lane_id() == 0) {
      atomicAdd(&row[kCntPrimary], n_primary);
      atomicAdd(&row[kCntHits], cnt.hits);
      atomicAdd(&row[kCntShadow], cnt.shadow);
    }
  }
}

// inst_radiance_kernel for a scene with motion: the lane's time goes with the
// scene's tables into every walk of its ray tree.
template <bool RECURSE, bool LIT>
__global__ __launch_bounds__(kRadianceWaves * 64) void motion_radiance_kernel(
    RenderParams P, QueryParams Q, RadianceParams R, const DevMaterial* __restrict__ mats,
    const DevLight* __restrict__ lights, LitArg<LIT> lit, InstParams T, MotionParams M) {
  __shared__ WaveLeafLds leaf_lds[kRadianceWaves];
  const long long slot = (long long)blockIdx.x * (kRadianceWaves * 64) + threadIdx.x;
  const long long i = R.first + slot;
  if ((i & ~63ll) >= Q.n) return;  // the whole wave is past the batch
  WaveLeafLds& L = leaf_lds[threadIdx.x >> 6];
  const QueryRay q = load_motion_ray(Q, M, i);
  const unsigned long long n_primary = __builtin_popcountll(ballot(q.valid));
  float t;
  TreeCounts cnt;
  const f4* own = nullptr;
  int own_k = 0;
  if constexpr (LIT) {
    const long long ray = q.in && !lit.shared ? query_slot(Q, i) : 0;
    own = reinterpret_cast<const f4*>(lit.lights) + 3 * (size_t)ray * (size_t)lit.k;
    own_k = lit.k;
  }
  const MotionArg inst{T, M, q.time};
  const V3 c = trace_tree<true, false, true, RECURSE, LIT, false, MotionArg>(
      P, nullptr, nullptr, nullptr, mats, lights, nullptr, L, RECURSE ? R.frames + slot : nullptr,
      (size_t)R.lanes, q.o, q.d, R.in_medium != 0, R.depth, q.valid, t, cnt, surf_of(), own, own_k,
      inst);
  if (i < Q.n) {
    const f4 out = {0.0f + c.x, 0.0f + c.y, 0.0f + c.z, t};
    reinterpret_cast<f4*>(Q.out)[query_slot(Q, i)] = out;
  }
  if (P.counters) {
    unsigned long long* row = counter_row(P, (int)((i >> 6) % kCounterSlots));
    if (cnt.secondary) atomicAdd(&row[kCntSecondary], cnt.secondary);
    if (lane_id() == 0) {
      atomicAdd(&row[kCntPrimary], n_primary);
      atomicAdd(&row[kCntHits], cnt.hits);
      atomicAdd(&row[kCntShadow], cnt.shadow);
    }
  }
}

// RT_QUERY_REORDER: a permutation that brings similar rays into the same wave (64 unrelated rays
// walk the union of 64 paths).  Key, most significant first: the dominant axis and sign of d (6
// cube faces), the origin's cell in a 2x2x2 grid over the clamped scene box, and the direction's
// position on its cube face, 128 x 128 cells in Morton order (kQueryOriginBits / kQueryDirBits
// bits per axis, rt_internal.h; measured against 4x4x4 and 64 x 64 in DESIGN.md §4.11); small
// batches drop the low bits
// (Q.shift).  Invalid rays share the last bin (face 7, which no direction has).  One counting
// sort: histogram by atomics, exclusive scan (per chunk of kQueryScanChunk bins, then over the
// chunk totals), scatter through the bins' counters as atomic cursors.  Not stable: results do
// not depend on the order.
__device__ __forceinline__ unsigned spread8(unsigned x) {  // bits 0..7 -> the even bits 0..14
  x = (x | (x << 4)) & 0x0f0fu;
  x = (x | (x << 2)) & 0x3333u;
  x = (x | (x << 1)) & 0x5555u;
  return x;
}

__device__ __forceinline__ int cell_of(float x, float cells) {  // clamped, NaN -> 0
  return (int)__builtin_fminf(__builtin_fmaxf(x, 0.0f), cells - 1.0f);
}

__device__ __forceinline__ unsigned query_key(const QueryParams& Q, long long i) {
  const f4* p = reinterpret_cast<const f4*>(Q.rays) + 2 * i;
  const f4 a = p[0], b = p[1];
  const V3 o = v3(a.x, a.y, a.z), d = v3(b.x, b.y, b.z);
  if (!query_ray_ok(o, d)) return (unsigned)Q.bins - 1u;
  const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
  int axis = 0;
  float dm = d.x, du = d.y, dv = d.z;
  if (ay > ax && ay >= az) {
    axis = 1;
    dm = d.y, du = d.z, dv = d.x;
  } else if (az > ax && az > ay) {
    axis = 2;
    dm = d.z, du = d.x, dv = d.y;
  }
  const unsigned face = 2u * (unsigned)axis + (dm < 0.0f ? 1u : 0u);
  constexpr float kDirCells = (float)(1 << kQueryDirBits), kCells = (float)(1 << kQueryOriginBits);
  const float inv = 0.5f * kDirCells / __builtin_fabsf(dm);  // |du|, |dv| <= |dm|
  const unsigned u = (unsigned)cell_of(du * inv + 0.5f * kDirCells, kDirCells);
  const unsigned v = (unsigned)cell_of(dv * inv + 0.5f * kDirCells, kDirCells);
  const unsigned cx = (unsigned)cell_of((o.x - Q.box_lo[0]) * Q.box_scale[0] * kCells, kCells);
  const unsigned cy = (unsigned)cell_of((o.y - Q.box_lo[1]) * Q.box_scale[1] * kCells, kCells);
  const unsigned cz = (unsigned)cell_of((o.z - Q.box_lo[2]) * Q.box_scale[2] * kCells, kCells);
  const unsigned cell = (cz << (2 * kQueryOriginBits)) | (cy << kQueryOriginBits) | cx;
  const unsigned key = (face << (kQueryKeyBits - 3)) | (cell << (2 * kQueryDirBits)) |
                       (spread8(v) << 1) | spread8(u);
  return key >> Q.shift;
}

constexpr int kQueryThreads = 256;

// counter[key] += 1 for every active lane; returns what the lane's own atomicAdd(&counter[key], 1)
// would have (POS; its position in the bin when the counters are cursors).  Neighbouring rays
// of an ordered batch share a bin, and 64 atomics on one address serialise (first measurement:
// sorting an ordered C3 batch took twice as long as a shuffled one), so the lanes holding one of
// the wave's first kQueryAggregate distinct keys go through one atomic per key, ranked in lane
// order; the others (a shuffled batch: 64 different bins) add for themselves.  Every lane of
// the wave takes part.
constexpr int kQueryAggregate = 4;
template <bool POS>
__device__ __forceinline__ unsigned wave_count(unsigned* counter, unsigned key, bool active) {
  const int lane = lane_id();
  uint64_t todo = ballot(active);
  int head = lane;          // the lane whose atomic covers this one (itself: on its own)
  unsigned rank = 0, count = 1;
  for (int it = 0; it < kQueryAggregate && todo; it++) {
    const int leader = __builtin_ctzll(todo);
    const unsigned k = (unsigned)__builtin_amdgcn_readlane((int)key, leader);
    const uint64_t same = ballot(active && key == k) & todo;
    if ((same >> lane) & 1) {
      head = leader;
      rank = __builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32),
                                       __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));
      count = (unsigned)__builtin_popcountll(same);
    }
    todo &= ~same;
  }
  // one atomic per lane at most, all in flight together
  unsigned base = 0;
  if (active && head == lane) {
    if (POS)
      base = atomicAdd(&counter[key], count);
    else
      atomicAdd(&counter[key], count);
  }
  if (!POS) return 0;
  return (unsigned)__builtin_amdgcn_ds_bpermute(head << 2, (int)base) + rank;
}

__global__ __launch_bounds__(kQueryThreads) void query_hist_kernel(QueryParams Q) {
  const long long i = (long long)blockIdx.x * kQueryThreads + threadIdx.x;
  const bool active = i < Q.n;
  wave_count<false>(Q.hist, active ? query_key(Q, i) : 0u, active);
}

// Exclusive scan of v over the workgroup's T threads (T a power of two); total = the sum.
template <int T>
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* lds, unsigned& total) {
  const int tid = (int)threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const unsigned x = tid >= off ? lds[tid - off] : 0u;
    __syncthreads();
    lds[tid] += x;
    __syncthreads();
  }
  total = lds[T - 1];
  return lds[tid] - v;
}

// Each workgroup turns its chunk of kQueryScanChunk counters into exclusive prefix sums within
// the chunk and writes the chunk's total.
__global__ __launch_bounds__(kQueryThreads) void query_scan_chunks_kernel(QueryParams Q) {
  constexpr int kPer = kQueryScanChunk / kQueryThreads;
  __shared__ unsigned lds[kQueryThreads];
  unsigned* h = Q.hist + (size_t)blockIdx.x * kQueryScanChunk + threadIdx.x * kPer;
  unsigned c[kPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    c[k] = h[k];
    sum += c[k];
  }
  unsigned total;
  unsigned run = block_scan<kQueryThreads>(sum, lds, total);
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    h[k] = run;
    run += c[k];
  }
  if (threadIdx.x == 0) Q.totals[blockIdx.x] = total;
}

// The chunk totals (at most 2^(kQueryKeyBits - kQueryMinBinBits) <= 1024) into exclusive sums.
constexpr int kQueryMaxChunks = 1 << (kQueryKeyBits - kQueryMinBinBits);
__global__ __launch_bounds__(kQueryMaxChunks) void query_scan_totals_kernel(QueryParams Q) {
  __shared__ unsigned lds[kQueryMaxChunks];
  const int chunks = Q.bins / kQueryScanChunk;
  const unsigned v = (int)threadIdx.x < chunks ? Q.totals[threadIdx.x] : 0u;
  unsigned total;
  const unsigned e = block_scan<kQueryMaxChunks>(v, lds, total);
  if ((int)threadIdx.x < chunks) Q.totals[threadIdx.x] = e;
}

__global__ __launch_bounds__(kQueryThreads) void query_scatter_kernel(QueryParams Q) {
  const long long i = (long long)blockIdx.x * kQueryThreads + threadIdx.x;
  const bool active = i < Q.n;
  const unsigned key = active ? query_key(Q, i) : 0u;
  // the bin's counter holds its start within the chunk and serves as its cursor; the counts sum
  // to n, so every position is below n
  const unsigned at = wave_count<true>(Q.hist, key, active);
  if (active) Q.perm_out[at + Q.totals[key >> kQueryMinBinBits]] = (int)i;
}

hipError_t launch_query_sort(QueryParams Q, hipStream_t stream);

// One query launch over Q.n rays (0 < n <= kQueryMaxLaunch); reorder: Q's hist / totals /
// perm_out point at query_scratch_words(n) words of scratch.  The variant is picked as
// launch_render picks the frame kernels'.
hipError_t launch_query(const RenderParams& P, QueryParams Q, const DevNode* nodes, bool occlusion,
                        bool reorder, bool fast, bool deep, bool spheres, const SurfParams* surf,
                        hipStream_t stream) {
  if (Q.n <= 0) return hipSuccess;
  Q.perm = nullptr;
  if (reorder) {
    const hipError_t e = launch_query_sort(Q, stream);
    if (e != hipSuccess) return e;
    Q.perm = Q.perm_out;
  }
  const dim3 grid((unsigned)((Q.n + kWavesPerBlock * 64 - 1) / (kWavesPerBlock * 64)));
  dispatch_variant(use_fast(P, fast), deep, spheres, [&](auto fa, auto de, auto sp) {
    constexpr bool F = decltype(fa)::value, D = decltype(de)::value, S = decltype(sp)::value;
    const size_t lds = deep_lds_bytes<D>(kWavesPerBlock);
    if (occlusion)
      hipLaunchKernelGGL((query_occluded_kernel<F, D, S>), grid, dim3(kWavesPerBlock * 64), lds,
                         stream, P, Q, nodes);
    else
      with_surface(surf, [&](auto sm, auto... arg) {
        hipLaunchKernelGGL((query_closest_kernel<F, D, S, decltype(sm)::value>), grid,
                           dim3(kWavesPerBlock * 64), lds, stream, P, Q, nodes, arg...);
      });
  });
  return hipGetLastError();
}

// launch_query for an instanced scene.  fast: the base meshes that have a
// culling tree are walked through it; spheres: the top level holds a loose sphere.
hipError_t launch_inst_query(const RenderParams& P, QueryParams Q, const InstParams& T,
                             bool occlusion, bool reorder, bool fast, bool spheres,
                             const MotionParams* motion, hipStream_t stream) {
  if (Q.n <= 0) return hipSuccess;
  Q.perm = nullptr;
  if (reorder) {
    const hipError_t e = launch_query_sort(Q, stream);
    if (e != hipSuccess) return e;
    Q.perm = Q.perm_out;
  }
  const dim3 grid((unsigned)((Q.n + kWavesPerBlock * 64 - 1) / (kWavesPerBlock * 64)));
  if (motion) {  // a scene with motion: its own kernels (motion->fast: the traversal mode)
    if (occlusion)
      hipLaunchKernelGGL(motion_occluded_kernel, grid, dim3(kWavesPerBlock * 64), 0, stream, P, Q,
                         T, *motion);
    else
      hipLaunchKernelGGL(motion_closest_kernel, grid, dim3(kWavesPerBlock * 64), 0, stream, P, Q,
                         T, *motion);
    return hipGetLastError();
  }
  dispatch_variant(fast, false, spheres, [&](auto fa, auto, auto sp) {
    constexpr bool F = decltype(fa)::value, S = decltype(sp)::value;
    if (occlusion)
      hipLaunchKernelGGL((inst_occluded_kernel<F, S>), grid, dim3(kWavesPerBlock * 64), 0, stream,
                         P, Q, T);
    else
      hipLaunchKernelGGL((inst_closest_kernel<F, S>), grid, dim3(kWavesPerBlock * 64), 0, stream,
                         P, Q, T);
  });
  return hipGetLastError();
}

// The permutation of Q's rays [0, Q.n) into Q.perm_out (RT_QUERY_REORDER), for launches that
// trace the batch in chunks afterwards (launch_radiance).
hipError_t launch_query_sort(QueryParams Q, hipStream_t stream) {
  if (Q.n <= 0) return hipSuccess;
  const int bits = query_bin_bits(Q.n);
  Q.shift = kQueryKeyBits - bits;
  Q.bins = 1 << bits;
  const hipError_t e = hipMemsetAsync(Q.hist, 0, sizeof(unsigned) * (size_t)Q.bins, stream);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((Q.n + kQueryThreads - 1) / kQueryThreads));
  hipLaunchKernelGGL(query_hist_kernel, grid, dim3(kQueryThreads), 0, stream, Q);
  hipLaunchKernelGGL(query_scan_chunks_kernel, dim3(Q.bins / kQueryScanChunk),
                     dim3(kQueryThreads), 0, stream, Q);
  hipLaunchKernelGGL(query_scan_totals_kernel, dim3(1), dim3(kQueryMaxChunks), 0, stream, Q);
  hipLaunchKernelGGL(query_scatter_kernel, grid, dim3(kQueryThreads), 0, stream, Q);
  return hipGetLastError();
}

// One chunk of a radiance query: the rays [R.first, Q.n) of Q's order (Q.perm: the whole batch's
// permutation, or null), at most R.lanes of them.  R.frames == nullptr picks the variant that
// cannot recurse.
hipError_t launch_radiance(const RenderParams& P, const QueryParams& Q, const RadianceParams& R,
                           const LitParams* lit, const DevNode* nodes, bool fast, bool deep,
                           bool spheres, const SurfParams* surf, const InstParams* inst,
                           const MotionParams* motion, const TexParams* tex, hipStream_t stream) {
  if (Q.n <= R.first) return hipSuccess;
  const dim3 grid((unsigned)((Q.n - R.first + kRadianceWaves * 64 - 1) / (kRadianceWaves * 64)));
  if (inst && motion) {  // a scene with motion: its own kernels
    auto launch = [&](auto re, auto li, auto arg) {
      hipLaunchKernelGGL((motion_radiance_kernel<decltype(re)::value, decltype(li)::value>), grid,
                         dim3(kRadianceWaves * 64), 0, stream, P, Q, R, P.materials, P.lights, arg,
                         *inst, *motion);
    };
    using T = std::true_type;
    using N = std::false_type;
    if (lit) {
      LitArg<true> arg;
      static_cast<LitParams&>(arg) = *lit;
      if (R.frames == nullptr)
        launch(N{}, T{}, arg);
      else
        launch(T{}, T{}, arg);
    } else if (R.frames == nullptr) {
      launch(N{}, N{}, LitArg<false>{});
    } else {
      launch(T{}, N{}, LitArg<false>{});
    }
    return hipGetLastError();
  }
  if (inst) {  // an instanced scene: the INST kernels (fast: the base meshes' culling trees)
    const InstArg ia{*inst};
    dispatch_variant(fast, false, spheres, [&](auto fa, auto, auto sp) {
      constexpr bool F = decltype(fa)::value, S = decltype(sp)::value;
      auto launch = [&](auto re, auto li, auto arg) {
        hipLaunchKernelGGL((inst_radiance_kernel<F, S, decltype(re)::value, decltype(li)::value>),
                           grid, dim3(kRadianceWaves * 64), 0, stream, P, Q, R, P.materials,
                           P.lights, arg, ia);
      };
      using T = std::true_type;
      using N = std::false_type;
      if (lit) {
        LitArg<true> arg;
        static_cast<LitParams&>(arg) = *lit;
        if (R.frames == nullptr)
          launch(N{}, T{}, arg);
        else
          launch(T{}, T{}, arg);
      } else if (R.frames == nullptr) {
        launch(N{}, N{}, LitArg<false>{});
      } else {
        launch(T{}, N{}, LitArg<false>{});
      }
    });
    return hipGetLastError();
  }
  dispatch_variant(use_fast(P, fast), deep, spheres, [&](auto fa, auto de, auto sp) {
    constexpr bool F = decltype(fa)::value, D = decltype(de)::value, S = decltype(sp)::value;
    const size_t lds = deep_lds_bytes<D>(kRadianceWaves);
    auto launch = [&](auto re, auto li, auto arg) {
      constexpr bool RE = decltype(re)::value, LI = decltype(li)::value;
      if (tex) {  // a textured scene: the TEX kernels, SPHERES and SMOOTH set whatever it holds
        const TexLaunch a(*surf, *tex);
        hipLaunchKernelGGL((query_radiance_kernel<F, D, true, RE, LI, true, true>), grid,
                           dim3(kRadianceWaves * 64), lds, stream, P, Q, R, nodes, P.prims,
                           P.normals, P.materials, P.lights, arg, a.surf, a.tex);
      } else {
        with_surface(surf, [&](auto sm, auto... sarg) {
          hipLaunchKernelGGL((query_radiance_kernel<F, D, S, RE, LI, decltype(sm)::value, false>),
                             grid, dim3(kRadianceWaves * 64), lds, stream, P, Q, R, nodes, P.prims,
                             P.normals, P.materials, P.lights, arg, sarg...);
        });
      }
    };
    using T = std::true_type;
    using N = std::false_type;
    if (lit) {  // (caller light records: rt_shade_rays_lit*)
      LitArg<true> arg;
      static_cast<LitParams&>(arg) = *lit;
      if (R.frames == nullptr)  // (no RECURSE)
        launch(N{}, T{}, arg);
      else
        launch(T{}, T{}, arg);
    } else if (R.frames == nullptr) {
      launch(N{}, N{}, LitArg<false>{});
    } else {
      launch(T{}, N{}, LitArg<false>{});
    }
  });
  return hipGetLastError();
}

// rt_hit_attributes* (DESIGN.md §4.15): a lane per ray; two 16-B loads of the ray, one of the hit
// record's first half (t and the leaf), three 16-B stores.  Record i comes from ray i and
// hits[i].leaf alone: a triangle's beta and gamma as the walk computed them (tri_barycentrics), a
// sphere's normal from hits[i].t as query_closest_kernel computes it.  A leaf outside
// [0, S.num_leaves) or an invalid ray (query_ray_ok) gives the all-zero record, and no load
// depends on anything else the caller wrote.  S.tri / S.normals / S.uv may each be null.
constexpr int kAttrHit = 1, kAttrTriangle = 2, kAttrSmooth = 4;  // RT_ATTR_*
__global__ __launch_bounds__(256) void hit_attr_kernel(RenderParams P, SurfParams S, AttrParams A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const f4* rp = reinterpret_cast<const f4*>(A.rays) + 2 * i;
  const f4 ra = rp[0], rb = rp[1];
  const f4 h0 = reinterpret_cast<const f4*>(A.hits)[2 * i];
  const V3 o = v3(ra.x, ra.y, ra.z), d = v3(rb.x, rb.y, rb.z);
  const int leaf = __float_as_int(h0.w);
  f4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0, a2 = a0;
  if (leaf >= 0 && leaf < S.num_leaves && query_ray_ok(o, d)) {
    const DevPrim& pr = P.prims[leaf];
    if (pr.kind == kPrimTriangle) {
      const LaneRay ray = make_ray(o, d, P.quot_ok);
      float beta, gamma;
      tri_barycentrics(pr, ray, beta, gamma);
      const V3 flat = ld3(P.normals + 4 * leaf);
      V3 sn = flat;
      int flags = kAttrHit | kAttrTriangle;
      float u = 0.0f, v = 0.0f;
      if (S.tri) {
        const i4 tr = reinterpret_cast<const i4*>(S.tri)[leaf];
        if (S.uv) {
          const float w = (1.0f - beta) - gamma;
          const float* t0 = S.uv + 2 * (size_t)tr.x;
          const float* t1 = S.uv + 2 * (size_t)tr.y;
          const float* t2 = S.uv + 2 * (size_t)tr.z;
          u = bary_mix(t0[0], t1[0], t2[0], w, beta, gamma);
          v = bary_mix(t0[1], t1[1], t2[1], w, beta, gamma);
        }
        if (S.normals && (tr.w & kSurfSmooth)) {
          sn = smooth_normal(S, tr, beta, gamma);
          flags |= kAttrSmooth;
        }
      }
      a0 = (f4){beta, gamma, u, v};
      a1 = (f4){sn.x, sn.y, sn.z, __int_as_float(flags)};
      a2 = (f4){flat.x, flat.y, flat.z, 0.0f};
    } else {  // Sphere.h:42,50: (ray.point_at(t) - center).normalize()
      const V3 n = normalize((o + d * h0.x) - ld3(pr.v0));
      a1 = (f4){n.x, n.y, n.z, __int_as_float(kAttrHit)};
      a2 = (f4){n.x, n.y, n.z, 0.0f};
    }
  }
  f4* out = reinterpret_cast<f4*>(A.attr) + 3 * i;
  out[0] = a0;
  out[1] = a1;
  out[2] = a2;
}

hipError_t launch_hit_attributes(const RenderParams& P, const SurfParams& S, const AttrParams& A,
                                 hipStream_t stream) {
  if (A.n <= 0) return hipSuccess;
  for (long long done = 0; done < A.n; done += kQueryMaxLaunch) {  // (32-bit grids)
    AttrParams C;
    C.rays = static_cast<const char*>(A.rays) + (size_t)done * 32;
    C.hits = static_cast<const char*>(A.hits) + (size_t)done * 32;
    C.attr = static_cast<char*>(A.attr) + (size_t)done * 48;
    C.n = A.n - done < kQueryMaxLaunch ? A.n - done : kQueryMaxLaunch;
    hipLaunchKernelGGL(hit_attr_kernel, dim3((unsigned)((C.n + 255) / 256)), dim3(256), 0, stream,
                       P, S, C);
  }
  return hipGetLastError();
}

// rt_texture_lookup* (DESIGN.md §4.18): a lane per query, one 16-B load, tex_get_color as the ray
// trees run it, three stores.  A texture id outside [0, X.num_textures) gives 0 0 0 and reads
// nothing.
__global__ __launch_bounds__(256) void tex_lookup_kernel(TexParams X, TexLookupParams A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const f4 q = reinterpret_cast<const f4*>(A.q)[i];
  const int id = __float_as_int(q.x);
  float rgb[3] = {0.0f, 0.0f, 0.0f};
  if (id >= 0 && id < X.num_textures) tex_get_color(X.table[id], X.texels, q.y, q.z, rgb);
  float* o = A.rgb + 3 * i;
  o[0] = rgb[0];
  o[1] = rgb[1];
  o[2] = rgb[2];
}

hipError_t launch_texture_lookup(const TexParams& X, const TexLookupParams& A, hipStream_t stream) {
  if (A.n <= 0) return hipSuccess;
  for (long long done = 0; done < A.n; done += kQueryMaxLaunch) {  // (32-bit grids)
    TexLookupParams C;
    C.q = static_cast<const char*>(A.q) + (size_t)done * 16;
    C.rgb = A.rgb + 3 * (size_t)done;
    C.n = A.n - done < kQueryMaxLaunch ? A.n - done : kQueryMaxLaunch;
    hipLaunchKernelGGL(tex_lookup_kernel, dim3((unsigned)((C.n + 255) / 256)), dim3(256), 0, stream,
                       X, C);
  }
  return hipGetLastError();
}

// Self-check of tri_quotients against `/` on random operands spanning the whole fast range:
// |det| in [2^-40, 2^40] (a quarter with all-ones mantissas, where a reciprocal is hardest),
// numerators 0 or in [2^-49, 2^49], a quarter of them chosen so the quotient sits next to a
// rounding midpoint.  counts[0] += mismatches, counts[1] += cases.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void quot_check_kernel(unsigned long long seed, long long count,
                                                         unsigned long long* counts) {
  unsigned long long bad = 0, n = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const unsigned long long a = mix64(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1));
    const unsigned long long b = mix64(a ^ 0xD1B54A32D192ED03ull);
    const int ed = (int)(a % 81) - 40, en = (int)((a >> 8) % 99) - 49;
    unsigned md = (unsigned)(a >> 16) & 0x7fffffu;
    if (((a >> 40) & 3) == 0) md = 0x7fffffu - (unsigned)((a >> 42) & 3);
    float det = __uint_as_float(((unsigned)(ed + 127) << 23) | md);
    if ((a >> 44) & 1) det = -det;
    float num = __uint_as_float(((unsigned)(en + 127) << 23) | ((unsigned)b & 0x7fffffu));
    if ((b >> 23) & 1) num = -num;
    if (((b >> 24) & 3) == 0) {  // num = det * (a quotient just off a midpoint)
      const double q = ldexp(1.0 + (((b >> 26) & 0x7fffff) + 0.5) / 8388608.0, en - ed);
      const float m = (float)(q * (double)det);
      if (quot_coord(m) && __builtin_fabsf(m) >= 0x1p-49f && __builtin_fabsf(m) <= 0x1p49f) num = m;
    }
    if (((b >> 50) & 15) == 0) num = 0.0f;
    const V3 got = tri_quotients(v3(num, -num, num), det, true);
    const float want = num / det, wneg = (-num) / det;
    bad += (unsigned)(__float_as_uint(got.x) != __float_as_uint(want)) |
           (unsigned)(__float_as_uint(got.y) != __float_as_uint(wneg));
    n++;
  }
  atomicAdd(&counts[0], bad);
  atomicAdd(&counts[1], n);
}

// Mode 1: normalize_shared and light_quotients against `/` on random vectors.  A case is a vector
// a, six numerators and a divisor d2.  Exponents: a scale drawn from [-60, 60] (so lengths and
// divisors fall outside [2^-40, 2^40] as well as inside) minus 0..7 per component; one component
// in eight is zero, one in eight lies below 2^-49, a quarter of the mantissas are all ones (less
// 0..3).  counts[0] += cases with a quotient that differs from `/` in any bit, counts[1] += cases,
// counts[2] += helper calls that took the shared reciprocal, counts[3] += calls that took `/`.
__device__ __forceinline__ float quot_check_operand(unsigned long long h, int scale) {
  int e = scale - (int)(h & 7);
  if (((h >> 3) & 7) == 0) e = -50 - (int)((h >> 6) % 70);  // below 2^-49, down to 2^-119
  unsigned m = (unsigned)(h >> 16) & 0x7fffffu;
  if (((h >> 40) & 3) == 0) m = 0x7fffffu - (unsigned)((h >> 42) & 3);
  float x = __uint_as_float(((unsigned)(e + 127) << 23) | m);
  if (((h >> 44) & 7) == 0) x = 0.0f;
  return (h >> 47) & 1 ? -x : x;
}
__device__ __forceinline__ bool same_bits(V3 a, V3 b) {
  return __float_as_uint(a.x) == __float_as_uint(b.x) &&
         __float_as_uint(a.y) == __float_as_uint(b.y) &&
         __float_as_uint(a.z) == __float_as_uint(b.z);
}
__global__ __launch_bounds__(256) void quot_check_vec_kernel(unsigned long long seed,
                                                             long long count,
                                                             unsigned long long* counts) {
  unsigned long long bad = 0, n = 0, shared = 0, plain = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    unsigned long long h = mix64(seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1));
    const int sa = (int)(h % 121) - 60, sn = (int)((h >> 8) % 121) - 60,
              sd = (int)((h >> 16) % 121) - 60;
    float v[9];
    for (int k = 0; k < 9; k++) {
      h = mix64(h ^ 0xD1B54A32D192ED03ull);
      v[k] = quot_check_operand(h, k < 3 ? sa : sn);
    }
    h = mix64(h ^ 0xD1B54A32D192ED03ull);
    unsigned md = (unsigned)(h >> 16) & 0x7fffffu;
    if (((h >> 40) & 3) == 0) md = 0x7fffffu - (unsigned)((h >> 42) & 3);
    const float d2 = __uint_as_float(((unsigned)(sd + 127) << 23) | md);
    const V3 a = v3(v[0], v[1], v[2]), b = v3(v[3], v[4], v[5]), c = v3(v[6], v[7], v[8]);
    const float len = length(a);
    const bool ra = normalize_in_range(a, len), rl = light_terms_in_range(b, c, d2);
    V3 qb, qc;
    light_quotients(b, c, d2, qb, qc);
    const bool oa = same_bits(normalize_shared(a), a / len), ob = same_bits(qb, b / d2),
               oc = same_bits(qc, c / d2);
    bad += !(oa & ob & oc);
    shared += (unsigned)ra + (unsigned)rl;
    plain += (unsigned)!ra + (unsigned)!rl;
    n++;
  }
  atomicAdd(&counts[0], bad);
  atomicAdd(&counts[1], n);
  atomicAdd(&counts[2], shared);
  atomicAdd(&counts[3], plain);
}

hipError_t launch_quot_check(int mode, unsigned long long seed, long long count,
                             unsigned long long* counts, hipStream_t stream) {
  if (mode == 0)
    hipLaunchKernelGGL(quot_check_kernel, dim3(2048), dim3(256), 0, stream, seed, count, counts);
  else
    hipLaunchKernelGGL(quot_check_vec_kernel, dim3(2048), dim3(256), 0, stream, seed, count,
                       counts);
  return hipGetLastError();
}

hipError_t launch_motion_inverse(const float* fwd, const float* vel, const float* times,
                                 long long n, float* out12, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(motion_inverse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     fwd, vel, times, n, out12);
  return hipGetLastError();
}

hipError_t launch_render(const RenderParams& P, bool fast, bool deep, bool spheres,
                         const hipEvent_t* marks, const SurfParams* surf, const InstParams* inst,
                         const MotionParams* motion, const TexParams* tex, hipStream_t stream) {
  if (P.num_sel_tiles <= 0) return hipSuccess;
  if (tex && (!surf || !P.frames || inst)) return hipErrorInvalidValue;
  const int blocks = (P.num_sel_tiles + kWavesPerBlock - 1) / kWavesPerBlock;
  if (inst && motion) {  // a scene with motion: every ray of the frame at time 0
    if (!P.frames) return hipErrorInvalidValue;
    const MotionArg ma{*inst, *motion, 0.0f};
    mark(marks, 0, stream);
    hipLaunchKernelGGL(motion_recursive_kernel, dim3(blocks), dim3(kWavesPerBlock * 64), 0, stream,
                       P, P.materials, P.lights, ma);
    mark(marks, 1, stream);
    mark(marks, 2, stream);
    mark(marks, 3, stream);
    return hipGetLastError();
  }
  if (inst) {  // an instanced scene renders on the ray-tree path (P.frames: the host sees to it)
    if (!P.frames) return hipErrorInvalidValue;
    const InstArg ia{*inst};
    mark(marks, 0, stream);
    dispatch_variant(fast, false, spheres, [&](auto fa, auto, auto sp) {
      hipLaunchKernelGGL((inst_recursive_kernel<decltype(fa)::value, decltype(sp)::value>),
                         dim3(blocks), dim3(kWavesPerBlock * 64), 0, stream, P, P.materials,
                         P.lights, ia);
    });
    mark(marks, 1, stream);
    mark(marks, 2, stream);
    mark(marks, 3, stream);
    return hipGetLastError();
  }
  dispatch_variant(use_fast(P, fast), deep, spheres, [&](auto fa, auto de, auto sp) {
    launch_variant<decltype(fa)::value, decltype(de)::value, decltype(sp)::value>(
        P, blocks, marks, surf, tex, stream);
  });
  return hipGetLastError();
}

unsigned long long read_reset_exact_fallbacks() {
#ifdef RT_DIAG
  unsigned long long v = 0, z = 0;
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_exact_fallbacks), sizeof v);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_exact_fallbacks), &z, sizeof z);
  return v;
#else
  return 0;
#endif
}

// Copies (and clears) the RT_TIMELINE wave records: out[2][kTimelineWaves][3] start/end
// ticks of the 100 MHz clock and (estimated cost << 32 | tile sel, -1 for none).  Returns the number of values
// written, 0 in other builds.
long long read_reset_timeline(unsigned long long* out, long long max_values) {
#ifdef RT_TIMELINE
  const long long n = 2ll * kTimelineWaves * 3;
  if (max_values < n) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), n * sizeof *out) != hipSuccess) return -1;
  std::vector<unsigned long long> z((size_t)n, 0ull);
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), z.data(), n * sizeof *out) != hipSuccess) return -1;
  return n;
#else
  (void)out;
  (void)max_values;
  return 0;
#endif
}

// Copies (and clears) the RT_DIAG phase counters (kPhaseSlots values); 0 in other builds.
long long read_reset_phases(unsigned long long* out, long long max_values) {
#ifdef RT_DIAG
  if (max_values < kPhaseSlots) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), kPhaseSlots * sizeof *out) != hipSuccess) return -1;
  unsigned long long z[kPhaseSlots] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof z) != hipSuccess) return -1;
  return kPhaseSlots;
#else
  (void)out;
  (void)max_values;
  return 0;
#endif
}

// The runtime's occupancy query for the frame kernel's instantiation of a culling-tree scene
// without spheres or a deep tree (C3), on the current device: out4 = workgroups per CU, waves per
// CU, static LDS bytes per workgroup, VGPRs per lane.
hipError_t frame_kernel_occupancy(int* out4) {
  const auto kernel = trace_frame_kernel<true, false, false>;
  int blocks = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, kTraceWaves * 64, 0);
  if (e != hipSuccess) return e;
  hipFuncAttributes attr;
  e = hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kernel));
  if (e != hipSuccess) return e;
  out4[0] = blocks;
  out4[1] = blocks * kTraceWaves;
  out4[2] = (int)attr.sharedSizeBytes;
  out4[3] = attr.numRegs;
  return hipSuccess;
}

bool diag_build() {
#ifdef RT_DIAG
  return true;
#else
  return false;
#endif
}

}  // namespace rt
