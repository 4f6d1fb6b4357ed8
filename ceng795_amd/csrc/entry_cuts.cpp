// Entry cuts: per camera and frame tile, up to kEntryCut culling-tree nodes that
// together hold every leaf a pixel ray of the tile can reach, so the frame kernel's primary walk
// starts below the root without a test of its own.  A camera and a scene are fixed for the life
// of a scene object, so which slots a tile's frustum can enter is decided here, once, in double.
//
// Why it is exact.  A leaf the reference can reach for a pixel ray has a guard box the exact ray
// meets within the reference's rounding; every slot box above the leaf holds that guard box with
// the scene margin M, so the exact ray meets each of them once they are inflated by the ray's own
// share (2^-18 |cam_e| per axis; here twice that).  A slot whose inflated box lies wholly outside
// one side plane of the tile's frustum — widened by a whole pixel, so every pixel ray lies inside
// with more than half a pixel to spare — therefore has no reachable leaf below it for any ray of
// the tile.  The kernel may enter a cut node with lanes that would not have entered it from
// above: that only adds candidates, and the guard in the leaf batch decides exactly, as it does
// for every candidate.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "host_scene.h"

namespace rt {

namespace {

double half_bits_value(uint16_t h) {
  const int E = (h >> 10) & 31, M = h & 1023;
  if (E == 31) return M ? NAN : INFINITY;
  const double v = E == 0 ? std::ldexp((double)M, -24) : std::ldexp(1.0 + M / 1024.0, E - 15);
  return (h & 0x8000) ? -v : v;
}

DevNode8 wide_at(const HostScene& s, int ref) {
  DevNode8 W;
  std::memcpy(&W, &s.nodes[(size_t)(ref & ~kWideTag)], sizeof W);
  return W;
}

unsigned inner_mask(const DevNode8& W) {
  return (unsigned)W.kinds & ~((unsigned)W.kinds >> 8) & 0xffu;
}
unsigned leafy_mask(const DevNode8& W) { return ((unsigned)W.kinds >> 8) & (unsigned)W.kinds & 0xffu; }

// Slot c's box of copy 0 (lo plane in the low half), as the kernel decodes it.
void slot_box(const DevNode8& W, int c, double* lo, double* hi) {
  for (int a = 0; a < 3; a++) {
    const int k = (int)(int8_t)(uint8_t)((W.scale >> (8 * a)) & 255);
    lo[a] = (double)W.origin[a] + std::ldexp(half_bits_value((uint16_t)(W.box[c][a] & 0xffff)), k);
    hi[a] = (double)W.origin[a] + std::ldexp(half_bits_value((uint16_t)(W.box[c][a] >> 16)), k);
  }
}

// The tile's frustum: four inward side-plane normals through the apex cam_e.
struct Frustum {
  double n[4][3];
  bool to_root;  // the sign / skip rule: the tile walks from the root
};

Frustum tile_frustum(const rt_camera& c, int tx, int ty) {
  Frustum F;
  // the tile's pixel rectangle on the image plane, one whole pixel wider on every side
  const double x0 = (double)tx * kTile - 1.0, x1 = (double)(tx + 1) * kTile + 1.0;
  const double y0 = (double)ty * kTile - 1.0, y1 = (double)(ty + 1) * kTile + 1.0;
  const double fx[4] = {x0, x1, x1, x0}, fy[4] = {y0, y0, y1, y1};
  double v[4][3], mid[3] = {0, 0, 0}, longest = 0.0;
  for (int j = 0; j < 4; j++) {
    double len2 = 0.0;
    for (int a = 0; a < 3; a++) {
      v[j][a] = ((double)c.top_left[a] + (double)c.s_u[a] * fx[j] - (double)c.s_v[a] * fy[j]) -
                (double)c.e[a];
      mid[a] += v[j][a];
      len2 += v[j][a] * v[j][a];
    }
    longest = std::max(longest, std::sqrt(len2));
  }
  // The reference skips an axis with |d_a| < 1e-6 and then accepts boxes the ray misses on it:
  // such a tile keeps the root.  No ray of the tile comes near that when the four corners share
  // strict signs on every axis and every component stays above 2^-10 of the direction's length.
  F.to_root = !(longest > 0.0 && longest < INFINITY);
  for (int a = 0; a < 3 && !F.to_root; a++) {
    double least = INFINITY;
    for (int j = 0; j < 4; j++) {
      if (!(v[j][a] != 0.0 && (v[j][a] > 0.0) == (v[0][a] > 0.0))) F.to_root = true;
      least = std::min(least, std::fabs(v[j][a]));
    }
    if (!(least / longest >= 0x1p-10)) F.to_root = true;
  }
  for (int j = 0; j < 4; j++) {
    const double* p = v[j];
    const double* q = v[(j + 1) & 3];
    double n[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
    const double side = n[0] * mid[0] + n[1] * mid[1] + n[2] * mid[2];
    const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    // a degenerate plane (or one that is not finite) excludes nothing
    const double f = (side != 0.0 && len > 0.0 && len < INFINITY) ? (side > 0.0 ? 1.0 : -1.0) / len : 0.0;
    for (int a = 0; a < 3; a++) F.n[j][a] = f == 0.0 ? 0.0 : n[a] * f;
  }
  return F;
}

// "May enter" = is not provably missed: the box, inflated by twice the ray's own margin share,
// lies wholly outside one side plane, with a slack that covers the double arithmetic.
bool may_enter(const Frustum& F, const rt_camera& c, const double* lo, const double* hi) {
  for (int j = 0; j < 4; j++) {
    double most = 0.0, mag = 0.0;
    for (int a = 0; a < 3; a++) {
      const double share = 2.0 * 0x1p-18 * std::fabs((double)c.e[a]);
      const double l = (lo[a] - share) - (double)c.e[a], h = (hi[a] + share) - (double)c.e[a];
      most += std::max(F.n[j][a] * l, F.n[j][a] * h);
      mag += std::fabs(F.n[j][a]) * (std::fabs(l) + std::fabs(h) + std::fabs((double)c.e[a]));
    }
    if (most < -1e-9 * mag) return false;  // (a NaN anywhere: not missed)
  }
  return true;
}

}  // namespace

bool entry_cuts_apply(const HostScene& s, int stack_entries) {
  if (s.accel_root < 0 || s.root_kind != kRootNode || s.accel_stride <= 0) return false;
  return s.accel_depth + kEntryCut - 1 <= stack_entries;
}

std::vector<int> build_entry_cuts(const HostScene& s, const rt_camera& c,
                                  long long stats[kEntryCutStats]) {
  const int tiles_x = (c.width + kTile - 1) / kTile, tiles_y = (c.height + kTile - 1) / kTile;
  std::vector<int> table((size_t)tiles_x * tiles_y * kEntryCut, -1);
  if (stats) std::fill(stats, stats + kEntryCutStats, 0ll);
  struct Entry {
    int ref, depth;
    bool done;
  };
  for (int ty = 0; ty < tiles_y; ty++)
    for (int tx = 0; tx < tiles_x; tx++) {
      const Frustum F = tile_frustum(c, tx, ty);
      Entry cut[kEntryCut] = {{s.accel_root, 0, F.to_root}};
      int n = 1;
      long long saved_visits = 0, saved_slots = 0;
      for (bool changed = true; changed;) {
        changed = false;
        for (int i = 0; i < n; i++) {
          if (cut[i].done) continue;
          cut[i].done = true;
          const DevNode8 W = wide_at(s, cut[i].ref);
          const unsigned inner = inner_mask(W), leafy = leafy_mask(W);
          int kids[kWideSlots], nk = 0;
          bool leaf_entered = false;
          for (int k = 0; k < kWideSlots; k++) {
            if (!((inner | leafy) >> k & 1)) continue;
            double lo[3], hi[3];
            slot_box(W, k, lo, hi);
            if (!may_enter(F, c, lo, hi)) continue;
            if (leafy >> k & 1)
              leaf_entered = true;
            else
              kids[nk++] = (W.inner_base + 2 * k) | kWideTag;
          }
          // (a node nothing of which can be entered stays: the record always names a node)
          if (leaf_entered || nk == 0 || n - 1 + nk > kEntryCut) continue;
          saved_visits++;
          saved_slots += __builtin_popcount(inner | leafy);
          const int depth = cut[i].depth + 1;
          cut[i] = {kids[0], depth, false};
          for (int k = 1; k < nk; k++) cut[n++] = {kids[k], depth, false};
          changed = true;
        }
      }
      int* rec = &table[((size_t)ty * tiles_x + tx) * kEntryCut];
      int shallowest = cut[0].depth;
      for (int i = 0; i < n; i++) {
        rec[i] = cut[i].ref;
        shallowest = std::min(shallowest, cut[i].depth);
      }
      if (stats) {
        stats[kEcTiles]++;
        stats[kEcBySize + n]++;
        stats[kEcByDepth + std::min(shallowest, kEntryCutDepths - 1)]++;
        stats[kEcToRoot] += F.to_root;
        stats[kEcSavedVisits] += saved_visits;
        stats[kEcSavedSlots] += saved_slots;
      }
    }
  return table;
}

// ---------------------------------------------------------------------------------- the checker
namespace {

// visit_wide's per-lane slot test in its unscaled form (rt_kernels.hip): the same fp16 decode,
// ldexpf, fmaf and margins, the reciprocal a correctly rounded division.
struct HostRay {
  float o[3], rc[3], mg[3];
  bool skip[3], neg[3];
};

HostRay pixel_ray(const rt_camera& c, int px, int py) {
  HostRay r;
  const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
  float d[3], len2 = 0.0f;
  for (int a = 0; a < 3; a++) {
    const float su = c.s_u[a] * fx, sv = c.s_v[a] * fy;
    const float sp = (c.top_left[a] + su) - sv;
    d[a] = sp - c.e[a];
  }
  len2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  const float len = std::sqrt(len2);
  for (int a = 0; a < 3; a++) {
    d[a] = d[a] / len;
    r.o[a] = c.e[a];
    r.rc[a] = 1.0f / d[a];
    r.mg[a] = 0x1p-18f * std::fabs(c.e[a]) * r.rc[a];
    r.skip[a] = std::fabs(d[a]) < 1e-6f;
    r.neg[a] = std::signbit(r.rc[a]);
  }
  return r;
}

bool lane_enters(const DevNode8& W, int c, const HostRay& r) {
  float tn = -INFINITY, tf = INFINITY;
  for (int a = 0; a < 3; a++) {
    const int k = (int)(int8_t)(uint8_t)((W.scale >> (8 * a)) & 255);
    float S = std::ldexp(r.rc[a], k);
    const float A = W.origin[a] - r.o[a];
    float Alo = std::fmaf(A, r.rc[a], -std::fabs(r.mg[a]));
    float Ahi = std::fmaf(A, r.rc[a], std::fabs(r.mg[a]));
    if (r.skip[a]) S = 0.0f, Alo = -INFINITY, Ahi = INFINITY;
    const float lo = (float)half_bits_value((uint16_t)(W.box[c][a] & 0xffff));
    const float hi = (float)half_bits_value((uint16_t)(W.box[c][a] >> 16));
    const float n = std::fmaf(r.neg[a] ? hi : lo, S, Alo);
    const float f = std::fmaf(r.neg[a] ? lo : hi, S, Ahi);
    tn = std::fmax(tn, n);  // (fmax and fmin drop a NaN, as v_max3 / v_min3 do)
    tf = std::fmin(tf, f);
  }
  return tf >= std::fmax(tn, 0.0f);
}

}  // namespace

long long check_entry_cuts(const HostScene& s, const rt_camera& c, const std::vector<int>& table,
                           long long first[4]) {
  const int tiles_x = (c.width + kTile - 1) / kTile, tiles_y = (c.height + kTile - 1) / kTile;
  long long bad = 0;
  if (table.size() != (size_t)tiles_x * tiles_y * kEntryCut || s.accel_root < 0) return -1;
  struct Item {
    int ref;
    bool under;
  };
  std::vector<Item> todo;
  for (int py = 0; py < c.height; py++)
    for (int px = 0; px < c.width; px++) {
      const int* rec = &table[((size_t)(py / kTile) * tiles_x + px / kTile) * kEntryCut];
      const HostRay r = pixel_ray(c, px, py);
      auto in_cut = [&](int ref) {
        for (int i = 0; i < kEntryCut; i++)
          if (rec[i] == ref) return true;
        return false;
      };
      todo.assign(1, {s.accel_root, in_cut(s.accel_root)});
      while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        const DevNode8 W = wide_at(s, it.ref);
        const unsigned inner = inner_mask(W), leafy = leafy_mask(W);
        for (int k = 0; k < kWideSlots; k++) {
          if (!((inner | leafy) >> k & 1) || !lane_enters(W, k, r)) continue;
          if (inner >> k & 1) {
            const int ch = (W.inner_base + 2 * k) | kWideTag;
            todo.push_back({ch, it.under || in_cut(ch)});
          } else if (!it.under) {
            if (bad++ == 0 && first) first[0] = px, first[1] = py, first[2] = it.ref & ~kWideTag, first[3] = k;
          }
        }
      }
    }
  return bad;
}

}  // namespace rt
