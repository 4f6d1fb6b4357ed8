// MI355X (gfx950) film kernels: filtered accumulation of caller-supplied samples (rt_film_*,
// DESIGN.md §4.13) — the second half of Scene::render_image's MSAA branch (HW2/Scene.cpp:51-63,
// Pixel::add_color / get_color) for samples the caller chose.
//
// The contract is an order: after a call the film holds what one thread would leave that took the
// call's valid samples sorted by (source row, source column, index in the batch) and ran the
// reference's 3x3 splat for each.  fp32 addition does not commute with that order, so no float
// atomics: the call sorts the samples by source pixel (count, scan, scatter, order each list by
// index) and then GATHERS — one lane per destination pixel adds the samples of its
// neighbourhood's nine lists, row-major, in list order.
//
// Numerics: -ffp-contract=off and this file's pragma; '/' is the correctly rounded fp32 division;
// the Gaussian weight is rt_internal.h's gaussian_filter (fp64 ocml exp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ceng795_rt.h"
#include "rt_internal.h"

#pragma clang fp contract(off)

namespace rt {

namespace {

constexpr int kFilmThreads = 256;
constexpr int kFilmSortLds = 4096;   // list entries the workgroup sort keeps in LDS
constexpr int kFilmSortBlocks = 1024;  // workgroups that share the long lists
constexpr unsigned kFilmNoPixel = 0xffffffffu;

struct alignas(8) f2 {
  float x, y;
};
struct alignas(16) f4 {
  float x, y, z, w;
};

__device__ __forceinline__ int film_lane() {
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
__device__ __forceinline__ unsigned film_rank(uint64_t m) {  // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ bool film_finite(float a) {  // (a NaN fails the compare)
  return __builtin_fabsf(a) < __builtin_huge_valf();
}

// The source pixel of sample i, or kFilmNoPixel: the position outside [0, w) x [0, h) as fp32
// compares (-0.0f is inside and truncates to pixel 0; NaN fails every compare), or — the fused
// entry — an invalid ray (rt_kernels.hip query_ray_ok: a non-finite component, or every
// |d_i| < 1e-6).
__device__ __forceinline__ unsigned film_source(const FilmParams& F, long long i) {
  const f2 p = reinterpret_cast<const f2*>(F.xy)[i];
  bool ok = p.x >= 0.0f && p.x < (float)F.width && p.y >= 0.0f && p.y < (float)F.height;
  if (F.rays) {
    const f4* r = reinterpret_cast<const f4*>(F.rays) + 2 * i;
    const f4 a = r[0], b = r[1];
    constexpr float kEps = 0.000001f;  // HW2/Vector3.h:7 kEpsilon
    const bool tiny = (__builtin_fabsf(b.x) < kEps) & (__builtin_fabsf(b.y) < kEps) &
                      (__builtin_fabsf(b.z) < kEps);
    ok = ok && film_finite(a.x) && film_finite(a.y) && film_finite(a.z) && film_finite(b.x) &&
         film_finite(b.y) && film_finite(b.z) && !tiny;
  }
  return ok ? (unsigned)((int)p.y * F.width + (int)p.x) : kFilmNoPixel;
}

// counter[key] += 1 for every active lane; returns the value before this lane's own increment.
// Samples usually arrive grouped by pixel: when the wave's active lanes share one key its first
// lane adds their number and the lanes take consecutive values in lane order.
__device__ __forceinline__ unsigned film_cursor(unsigned* counter, unsigned key, bool active) {
  const uint64_t m = __ballot(active);
  if (!m) return 0;
  const int leader = __builtin_ctzll(m);
  const unsigned k0 = (unsigned)__shfl((int)key, leader);
  if (__ballot(active && key != k0) == 0) {
    unsigned base = 0;
    if (film_lane() == leader) base = atomicAdd(&counter[k0], (unsigned)__builtin_popcountll(m));
    return (unsigned)__shfl((int)base, leader) + film_rank(m);
  }
  return active ? atomicAdd(&counter[key], 1u) : 0u;
}

__global__ __launch_bounds__(kFilmThreads) void film_bin_kernel(FilmParams F) {
  const long long i = (long long)blockIdx.x * kFilmThreads + threadIdx.x;
  const bool in = i < F.n;
  const unsigned p = in ? film_source(F, i) : kFilmNoPixel;
  const bool valid = p != kFilmNoPixel;
  film_cursor(F.offs, p, valid);
  // the two sample counters: summed per workgroup first (every wave of the call adding to the
  // same two words cost more than the binning itself)
  __shared__ unsigned tally[2];
  if (threadIdx.x < 2) tally[threadIdx.x] = 0u;
  __syncthreads();
  const uint64_t added = __ballot(valid), dropped = __ballot(in && !valid);
  if (film_lane() == 0) {
    if (added) atomicAdd(&tally[0], (unsigned)__builtin_popcountll(added));
    if (dropped) atomicAdd(&tally[1], (unsigned)__builtin_popcountll(dropped));
  }
  __syncthreads();
  if (threadIdx.x < 2 && tally[threadIdx.x])
    atomicAdd(&F.counts[threadIdx.x], (unsigned long long)tally[threadIdx.x]);
}

// Exclusive scan of v over the workgroup's kFilmThreads threads; total = the sum.
__device__ __forceinline__ unsigned film_block_scan(unsigned v, unsigned* lds, unsigned& total) {
  const int tid = (int)threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int off = 1; off < kFilmThreads; off <<= 1) {
    const unsigned x = tid >= off ? lds[tid - off] : 0u;
    __syncthreads();
    lds[tid] += x;
    __syncthreads();
  }
  total = lds[kFilmThreads - 1];
  return lds[tid] - v;
}

// Each workgroup turns its chunk of kFilmScanChunk values of data[0, n) into exclusive prefix
// sums within the chunk and writes the chunk's total.
__global__ __launch_bounds__(kFilmThreads) void film_scan_kernel(unsigned* data, unsigned n,
                                                                 unsigned* totals) {
  constexpr int kPer = kFilmScanChunk / kFilmThreads;
  __shared__ unsigned lds[kFilmThreads];
  const unsigned base = blockIdx.x * (unsigned)kFilmScanChunk + threadIdx.x * (unsigned)kPer;
  unsigned c[kPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    c[k] = base + k < n ? data[base + k] : 0u;
    sum += c[k];
  }
  unsigned total;
  unsigned run = film_block_scan(sum, lds, total);
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    if (base + k < n) data[base + k] = run;
    run += c[k];
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// data[i] += the (scanned) total of the chunks before i's.
__global__ __launch_bounds__(kFilmThreads) void film_scan_add_kernel(unsigned* data, unsigned n,
                                                                     const unsigned* totals) {
  const unsigned i = blockIdx.x * (unsigned)kFilmThreads + threadIdx.x;
  if (i < n) data[i] += totals[i / (unsigned)kFilmScanChunk];
}

// data[0, n) into exclusive prefix sums; `sums` holds film_scan_words(n) words.
void film_scan(unsigned* data, size_t n, unsigned* sums, hipStream_t stream) {
  const size_t chunks = (n + kFilmScanChunk - 1) / kFilmScanChunk;
  hipLaunchKernelGGL(film_scan_kernel, dim3((unsigned)chunks), dim3(kFilmThreads), 0, stream, data,
                     (unsigned)n, sums);
  if (chunks <= 1) return;
  film_scan(sums, chunks, sums + chunks, stream);
  hipLaunchKernelGGL(film_scan_add_kernel, dim3((unsigned)((n + kFilmThreads - 1) / kFilmThreads)),
                     dim3(kFilmThreads), 0, stream, data, (unsigned)n, sums);
}

// A pixel's start is the cursor of its list; the counts sum to the valid samples, so every
// position is below n.  Afterwards offs[p] is the END of list p = the start of list p + 1.
__global__ __launch_bounds__(kFilmThreads) void film_scatter_kernel(FilmParams F) {
  const long long i = (long long)blockIdx.x * kFilmThreads + threadIdx.x;
  const unsigned p = i < F.n ? film_source(F, i) : kFilmNoPixel;
  const bool valid = p != kFilmNoPixel;
  const unsigned at = film_cursor(F.offs, p, valid);
  if (valid && at < (unsigned long long)F.n) F.list[at] = (unsigned)i;
}

__device__ __forceinline__ unsigned film_list_start(const FilmParams& F, unsigned p) {
  return p ? F.offs[p - 1] : 0u;
}

// The cursors hand out positions in any order: one lane per pixel puts its list into batch order
// (insertion sort — the lists arrive nearly sorted) or, beyond kFilmShortList entries, queues the
// pixel for film_sort_long_kernel.  Queue positions are below n / (kFilmShortList + 1).
__global__ __launch_bounds__(kFilmThreads) void film_order_kernel(FilmParams F) {
  const unsigned p = blockIdx.x * (unsigned)kFilmThreads + threadIdx.x;
  if (p >= (unsigned)(F.width * F.height)) return;
  const unsigned s = film_list_start(F, p), e = F.offs[p];
  if (e - s > (unsigned)kFilmShortList) {
    F.longs[1 + atomicAdd(&F.longs[0], 1u)] = p;
    return;
  }
  unsigned* a = F.list + s;
  const int len = (int)(e - s);
  for (int k = 1; k < len; k++) {
    const unsigned v = a[k];
    int b = k;
    while (b > 0 && a[b - 1] > v) {
      a[b] = a[b - 1];
      b--;
    }
    a[b] = v;
  }
}

// One compare-exchange of a[i], a[l] (i < l), the minimum to the lower index; entries at or
// beyond len count as +inf, so they never move.
__device__ __forceinline__ void film_cmpx(unsigned* a, unsigned i, unsigned l, unsigned len) {
  if (l >= len) return;
  const unsigned x = a[i], y = a[l];
  if (x > y) {
    a[i] = y;
    a[l] = x;
  }
}

// Bitonic sort of a[0, len) by the workgroup, in the form whose comparators all point the same
// way (per merge of k: one "flip" step pairing i with its mirror in the block of k, then
// half-cleaners of k/4 .. 1), so a length that is no power of two needs only the virtual +inf
// padding of film_cmpx.  `a` is LDS or global memory: __syncthreads orders both within the
// workgroup.
__device__ __forceinline__ void film_bitonic(unsigned* a, unsigned len) {
  unsigned size = 1;
  while (size < len) size <<= 1;
  const unsigned pairs = size >> 1;
  for (unsigned k = 2; k <= size; k <<= 1) {
    const unsigned half = k >> 1;
    for (unsigned t = threadIdx.x; t < pairs; t += kFilmThreads) {
      const unsigned blk = t / half, o = t - blk * half;
      film_cmpx(a, blk * k + o, blk * k + k - 1 - o, len);
    }
    __syncthreads();
    for (unsigned j = k >> 2; j >= 1; j >>= 1) {
      for (unsigned t = threadIdx.x; t < pairs; t += kFilmThreads) {
        const unsigned blk = t / j, o = t - blk * j;
        film_cmpx(a, blk * 2 * j + o, blk * 2 * j + o + j, len);
      }
      __syncthreads();
    }
  }
}

// The queued long lists, one workgroup at a time: through LDS when the list fits, else in place.
__global__ __launch_bounds__(kFilmThreads) void film_sort_long_kernel(FilmParams F) {
  __shared__ unsigned lds[kFilmSortLds];
  const unsigned count = F.longs[0];
  for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
    const unsigned p = F.longs[1 + q];
    const unsigned s = film_list_start(F, p), len = F.offs[p] - s;
    unsigned* a = F.list + s;
    if (len <= (unsigned)kFilmSortLds) {
      for (unsigned t = threadIdx.x; t < len; t += kFilmThreads) lds[t] = a[t];
      __syncthreads();
      film_bitonic(lds, len);
      for (unsigned t = threadIdx.x; t < len; t += kFilmThreads) a[t] = lds[t];
      __syncthreads();
    } else {
      film_bitonic(a, len);
    }
  }
}

// One lane per destination pixel (16 x 16 pixels per workgroup, as msaa_resolve_kernel): the
// running Pixel, then every sample of the up to nine source lists in the film, source rows
// outermost, each list in batch order — HW2/Scene.cpp:51-62 and Pixel::add_color turned inside
// out.  The box filter adds a pixel's own list with weight 1.
__global__ __launch_bounds__(256) void film_gather_kernel(FilmParams F) {
  const int ai = (int)(blockIdx.x * 16 + (threadIdx.x & 15));
  const int aj = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
  if (ai >= F.width || aj >= F.height) return;
  f4* px = reinterpret_cast<f4*>(F.pixels) + ((size_t)aj * F.width + ai);
  f4 acc = *px;
  const float cx = (float)ai + 0.5f, cy = (float)aj + 0.5f;
  const bool box = F.filter == kFilmBox;
  const int reach = box ? 0 : 1;
  const f2* xy = reinterpret_cast<const f2*>(F.xy);
  const f4* rad = reinterpret_cast<const f4*>(F.rad);
  bool touched = false;
  for (int j = aj - reach; j <= aj + reach; j++) {
    if (j < 0 || j >= F.height) continue;
    for (int i = ai - reach; i <= ai + reach; i++) {
      if (i < 0 || i >= F.width) continue;
      const unsigned p = (unsigned)(j * F.width + i);
      const unsigned s = film_list_start(F, p), e = F.offs[p];
      for (unsigned k = s; k < e; k++) {
        const unsigned idx = F.list[k];
        const f2 pos = xy[idx];
        const f4 c = rad[idx];
        const float w = box ? 1.0f : gaussian_filter(pos.x - cx, pos.y - cy, F.sigma);
        acc.x = acc.x + c.x * w;
        acc.y = acc.y + c.y * w;
        acc.z = acc.z + c.z * w;
        acc.w = acc.w + w;
        touched = true;
      }
    }
  }
  if (touched) *px = acc;
}

// Pixel::get_color (HW2/Pixel.h:20): color / weight, 0 0 0 for a pixel no sample reached.
__global__ __launch_bounds__(kFilmThreads) void film_resolve_kernel(const float* pixels, float* out,
                                                                    unsigned n) {
  const unsigned p = blockIdx.x * (unsigned)kFilmThreads + threadIdx.x;
  if (p >= n) return;
  const f4 a = reinterpret_cast<const f4*>(pixels)[p];
  float* o = out + 3 * (size_t)p;
  const bool empty = a.w == 0.0f;
  o[0] = empty ? 0.0f : a.x / a.w;
  o[1] = empty ? 0.0f : a.y / a.w;
  o[2] = empty ? 0.0f : a.z / a.w;
}

void film_mark(const hipEvent_t* marks, int k, hipStream_t stream) {
  if (marks) (void)hipEventRecord(marks[k], stream);
}

}  // namespace

// One splat call: F.n samples (0 < n <= kFilmMaxSamples) into F.pixels, F's scratch pointing at
// film_scratch_words(width * height, n) words.  marks (nullable): kFilmStages + 1 events recorded
// around the stages (bin, scan, scatter, order, gather).
hipError_t launch_film_splat(const FilmParams& F, const hipEvent_t* marks, hipStream_t stream) {
  if (F.n <= 0) return hipSuccess;
  const size_t pixels = (size_t)F.width * F.height;
  hipError_t e = hipMemsetAsync(F.offs, 0, sizeof(unsigned) * pixels, stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(F.longs, 0, sizeof(unsigned), stream);
  if (e != hipSuccess) return e;
  const dim3 per_sample((unsigned)((F.n + kFilmThreads - 1) / kFilmThreads));
  const dim3 per_pixel((unsigned)((pixels + kFilmThreads - 1) / kFilmThreads));
  film_mark(marks, kFilmBin, stream);
  hipLaunchKernelGGL(film_bin_kernel, per_sample, dim3(kFilmThreads), 0, stream, F);
  film_mark(marks, kFilmScan, stream);
  film_scan(F.offs, pixels, F.sums, stream);
  film_mark(marks, kFilmScatter, stream);
  hipLaunchKernelGGL(film_scatter_kernel, per_sample, dim3(kFilmThreads), 0, stream, F);
  film_mark(marks, kFilmOrder, stream);
  hipLaunchKernelGGL(film_order_kernel, per_pixel, dim3(kFilmThreads), 0, stream, F);
  if (F.n > kFilmShortList)
    hipLaunchKernelGGL(film_sort_long_kernel, dim3(kFilmSortBlocks), dim3(kFilmThreads), 0, stream, F);
  film_mark(marks, kFilmGather, stream);
  hipLaunchKernelGGL(film_gather_kernel, dim3((F.width + 15) / 16, (F.height + 15) / 16), dim3(256),
                     0, stream, F);
  film_mark(marks, kFilmStages, stream);
  return hipGetLastError();
}

hipError_t launch_film_resolve(const float* pixels, float* out, int width, int height,
                               hipStream_t stream) {
  const size_t n = (size_t)width * height;
  hipLaunchKernelGGL(film_resolve_kernel, dim3((unsigned)((n + kFilmThreads - 1) / kFilmThreads)),
                     dim3(kFilmThreads), 0, stream, pixels, out, (unsigned)n);
  return hipGetLastError();
}

}  // namespace rt
