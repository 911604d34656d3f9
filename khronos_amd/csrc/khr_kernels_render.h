// khr_kernels_render.h — the live map seen from a pose (khr_render_view; ASSUMPTIONS.md A.12): one ray per pixel marched through
// the hashed block pool at fixed z-depth steps, trilinear TSDF samples, the first observed front crossing gives depth, normal,
// colour, label and voxel flags.  Reads the map only.  gfx950, wave64.
//
// Shape: one lane per ray, a wave covers an 8x8-pixel tile (its rays walk the same blocks, so the pool reads of a wave fall
// into few cache lines), four waves = one 16x16 tile per workgroup.  Every lane keeps the last two (block key -> slot) pairs it
// resolved in registers: the hash table is probed on a block change only.  No LDS.
#pragma once
#include "khr_device.h"
#include "khr_map_read.h"

namespace khr {

// Empty-space skipping (on in every shipped build).  -DKHR_RENDER_NO_SKIP builds the same kernel without it, for the A/B
// measurement of profiles/render_view.txt only; there is no run-time switch.
#ifdef KHR_RENDER_NO_SKIP
constexpr bool kRenderSkip = false;
#else
constexpr bool kRenderSkip = true;
#endif

enum RenderStat : int { RS_HIT = 0, RS_BLOCKED, RS_VISITED, RS_COUNT = 4 };
constexpr float kRenderIndexLimit = kMapIndexLimit;

struct RenderView {
  int W, H, K;  // K samples per ray
  float fx, fy, cx, cy, min_range, dt, min_weight;
  float Rw[9], tw[3];  // world_T_sensor as frame ingest has it (makePose)
  float* depth;        // every output may be null
  float* normal;
  uint32_t* color;
  uint32_t* label;
  uint8_t* vflags;
  uint8_t* status;
  unsigned long long* stats;  // RenderStat words, null when the caller wants none
};

struct RenderBlockCache {
  uint64_t k0 = kEmptyKey, k1 = kEmptyKey;  // (packKey never yields kEmptyKey: it fills 63 bits)
  uint32_t s0 = kInvalidSlot, s1 = kInvalidSlot;
};

// pool slot of block (bx, by, bz), kInvalidSlot when it is not allocated (or lies beyond the 21-bit index range of the keys)
__device__ inline uint32_t renderSlot(const DevMap& m, RenderBlockCache& c, int bx, int by, int bz) {
  if (!blockInKeyRange(bx, by, bz)) return kInvalidSlot;
  const uint64_t key = packKey(bx, by, bz);
  if (key == c.k0) return c.s0;
  const uint32_t s = key == c.k1 ? c.s1 : htLookup(m, key);
  c.k1 = c.k0;
  c.s1 = c.s0;
  c.k0 = key;
  c.s0 = s;
  return s;
}

// The trilinear sample of A.12 at world point pw.  Returns validity; *d = the interpolated distance of a valid sample.
// base[3] = the block of the sample's lowest-index tap and *base_missing = that block is not allocated: every sample whose
// lowest tap lies in the same block is then invalid too, which is what the march skips over.
template <int VPS>
__device__ inline bool renderSample(const DevMap& m, const DevParams& p, RenderBlockCache& c, float min_weight, const float* pw,
                                    float* d, int* base, bool* base_missing) {
  constexpr int NV = VPS * VPS * VPS, SH = VPS == 16 ? 4 : 3;
  *base_missing = false;
  int i0[3];
  float g[3], f[3];
  bool in_range = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g[a] = pw[a] * p.vs_inv - 0.5f;
    in_range = in_range && (fabsf(g[a]) < kRenderIndexLimit);
  }
  if (!in_range) return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float fl = floorf(g[a]);
    i0[a] = static_cast<int>(fl);
    f[a] = g[a] - fl;  // (= g - float(i0): fl is that integer's exact float)
  }
  const int lx = i0[0] & (VPS - 1), ly = i0[1] & (VPS - 1), lz = i0[2] & (VPS - 1);
  base[0] = i0[0] >> SH;  // floor division (arithmetic shift)
  base[1] = i0[1] >> SH;
  base[2] = i0[2] >> SH;
  const uint32_t s_base = renderSlot(m, c, base[0], base[1], base[2]);
  if (s_base == kInvalidSlot) {
    *base_missing = true;
    return false;
  }
  size_t at[8];
  if (lx < VPS - 1 && ly < VPS - 1 && lz < VPS - 1) {  // all eight taps in one block
    const size_t v = static_cast<size_t>(s_base) * NV + static_cast<size_t>(lx + VPS * (ly + VPS * lz));
#pragma unroll
    for (int t = 0; t < 8; ++t) at[t] = v + static_cast<size_t>((t & 1) + VPS * (((t >> 1) & 1) + VPS * (t >> 2)));
  } else {
    bool all = true;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int x = i0[0] + (t & 1), y = i0[1] + ((t >> 1) & 1), z = i0[2] + (t >> 2);
      const uint32_t s = t == 0 ? s_base : renderSlot(m, c, x >> SH, y >> SH, z >> SH);
      all = all && s != kInvalidSlot;
      at[t] = static_cast<size_t>(s) * NV + static_cast<size_t>((x & (VPS - 1)) + VPS * ((y & (VPS - 1)) + VPS * (z & (VPS - 1))));
    }
    if (!all) return false;
  }
  float w[8], v[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) w[t] = m.weight[at[t]];
#pragma unroll
  for (int t = 0; t < 8; ++t) v[t] = m.dist[at[t]];
  bool seen = true;
#pragma unroll
  for (int t = 0; t < 8; ++t) seen = seen && (w[t] >= min_weight);
  if (!seen) return false;
  *d = trilinear(v, f);
  return true;
}

// The first sample after k whose lowest tap can lie outside block `base`, given that sample k's lies inside.  In double, on the
// exact line through the float inputs: G_a(t) = (D_a t + T_a) * voxel_size_inv - 0.5 stays in [base_a VPS + E, (base_a + 1) VPS - E]
// up to t_hi.  E bounds what the float evaluation of A.12 can differ from the exact line by (9 roundings of relative size 2^-24
// on terms whose magnitudes sum to M_a voxel_size_inv + 1; E takes 2e-6 of that sum, 3.7 times the bound), so a sample this
// function passes over has floor(g_a) inside the block on every axis, in float as in exact arithmetic.  A ray that runs within E
// of a block face is not skipped at all.
template <int VPS>
__device__ inline int renderSkipTo(const DevParams& p, const RenderView& r, float x, float y, int k, const int* base) {
  const double vsi = static_cast<double>(p.vs_inv), dt = static_cast<double>(r.dt), t0 = static_cast<double>(r.min_range);
  const double t_k = t0 + static_cast<double>(k) * dt, t_max = t0 + static_cast<double>(r.K) * dt;
  double t_hi = t_max;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double r0 = static_cast<double>(r.Rw[3 * a]) * static_cast<double>(x), r1 = static_cast<double>(r.Rw[3 * a + 1]) * static_cast<double>(y),
                 r2 = static_cast<double>(r.Rw[3 * a + 2]), T = static_cast<double>(r.tw[a]);
    const double s = ((r0 + r1) + r2) * vsi, o = T * vsi - 0.5;
    const double M = (fabs(r0) + fabs(r1) + fabs(r2)) * t_max + fabs(T);
    const double E = 2e-6 * (M * vsi + 1.0);
    const double lo = static_cast<double>(base[a]) * VPS + E, hi = static_cast<double>(base[a] + 1) * VPS - E;
    const double g_k = s * t_k + o;
    if (!(g_k >= lo && g_k <= hi)) return k + 1;
    if (s > 0.0) t_hi = fmin(t_hi, (hi - o) / s);
    else if (s < 0.0) t_hi = fmin(t_hi, (lo - o) / s);
  }
  const double q = floor((t_hi - t0) / dt);  // samples up to q have t <= t_hi
  if (!(q > static_cast<double>(k))) return k + 1;
  return static_cast<int>(fmin(q, static_cast<double>(r.K - 1))) + 1;
}

// (a wave's total stays far below 2^32: 64 lanes x 65536 samples)
__device__ inline void renderStatAdd(unsigned long long* counter, uint32_t lane_value) { waveStatAdd(counter, lane_value); }

template <int VPS>
__global__ __launch_bounds__(256) void k_render_view(DevMap m, DevParams p, RenderView r) {
  constexpr int NV = VPS * VPS * VPS, SH = VPS == 16 ? 4 : 3;
  const int wave = static_cast<int>(threadIdx.x >> 6), lane = static_cast<int>(threadIdx.x & 63u);
  const int u = static_cast<int>(blockIdx.x) * 16 + (wave & 1) * 8 + (lane & 7);
  const int v = static_cast<int>(blockIdx.y) * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool in_image = u < r.W && v < r.H;
  uint32_t status = 0u, n_visited = 0u;
  float depth = 0.f, nrm[3] = {0.f, 0.f, 0.f};
  uint32_t color = 0u, label = 0u;
  uint8_t vflags = 0;
  if (in_image) {
    const float x = (static_cast<float>(u) - r.cx) / r.fx, y = (static_cast<float>(v) - r.cy) / r.fy;
    RenderBlockCache cache;
    bool prev_valid = false;
    float d_prev = 0.f, t_hit = 0.f;
    int k = 0;
    while (k < r.K) {
      const float t = r.min_range + static_cast<float>(k) * r.dt;
      float pw[3], d = 0.f;
      xform(r.Rw, r.tw, x * t, y * t, t, pw);
      int base[3];
      bool base_missing;
      ++n_visited;
      if (!renderSample<VPS>(m, p, cache, r.min_weight, pw, &d, base, &base_missing)) {
        prev_valid = false;
        k = (kRenderSkip && base_missing) ? renderSkipTo<VPS>(p, r, x, y, k, base) : k + 1;
        continue;
      }
      if (d <= 0.f) {
        if (prev_valid && d_prev > 0.f) {
          status = 1u;
          const float frac = d_prev / (d_prev - d);
          t_hit = (r.min_range + static_cast<float>(k - 1) * r.dt) + frac * r.dt;
        } else {
          status = 2u;
        }
        break;
      }
      prev_valid = true;
      d_prev = d;
      ++k;
    }
    if (status == 1u) {
      depth = t_hit;
      float ph[3];
      xform(r.Rw, r.tw, x * t_hit, y * t_hit, t_hit, ph);
      // attribute voxel: floor(p_hit * voxel_size_inv)
      float gi[3];
      bool in_range = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        gi[a] = floorf(ph[a] * p.vs_inv);
        in_range = in_range && (fabsf(gi[a]) < kRenderIndexLimit);
      }
      if (in_range) {
        const int ix = static_cast<int>(gi[0]), iy = static_cast<int>(gi[1]), iz = static_cast<int>(gi[2]);
        const uint32_t s = renderSlot(m, cache, ix >> SH, iy >> SH, iz >> SH);
        if (s != kInvalidSlot) {
          const size_t at = static_cast<size_t>(s) * NV + static_cast<size_t>((ix & (VPS - 1)) + VPS * ((iy & (VPS - 1)) + VPS * (iz & (VPS - 1))));
          if (r.color) color = m.color[at];
          if (r.label && p.with_semantics) label = m.sem_label[at];
          if (r.vflags) vflags = m.vflags[at] & VOX_PUBLIC_MASK;
        }
      }
      if (r.normal) {
        float g[3];
        bool all = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          float q[3] = {ph[0], ph[1], ph[2]}, dp = 0.f, dm = 0.f;
          int base[3];
          bool bm;
          q[a] = ph[a] + p.vs;
          all = renderSample<VPS>(m, p, cache, r.min_weight, q, &dp, base, &bm) && all;
          q[a] = ph[a] - p.vs;
          all = renderSample<VPS>(m, p, cache, r.min_weight, q, &dm, base, &bm) && all;
          g[a] = dp - dm;
        }
        const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        if (all && len != 0.f) {
          nrm[0] = g[0] / len;
          nrm[1] = g[1] / len;
          nrm[2] = g[2] / len;
        }
      }
    }
    const size_t px = static_cast<size_t>(v) * r.W + u;
    if (r.depth) r.depth[px] = depth;
    if (r.normal) {
      r.normal[3 * px] = nrm[0];
      r.normal[3 * px + 1] = nrm[1];
      r.normal[3 * px + 2] = nrm[2];
    }
    if (r.color) r.color[px] = color;
    if (r.label) r.label[px] = label;
    if (r.vflags) r.vflags[px] = vflags;
    if (r.status) r.status[px] = static_cast<uint8_t>(status);
  }
  if (r.stats) {  // one atomic per wave and counter (the waveAggInc pattern, on 64-bit totals)
    renderStatAdd(r.stats + RS_HIT, status == 1u ? 1u : 0u);
    renderStatAdd(r.stats + RS_BLOCKED, status == 2u ? 1u : 0u);
    renderStatAdd(r.stats + RS_VISITED, n_visited);
  }
}

}  // namespace khr
