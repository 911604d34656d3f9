// khr_kernels_query.h — the live map at world points (khr_query_points; ASSUMPTIONS.md A.13): trilinear distance, its index-space
// central-difference gradient and the attributes of the voxel each point lies in.  Reads the map only.  gfx950, wave64.
//
// Shape: one lane per point, 256-thread workgroups.  The seven samples of a point (the centre and six shifted by one voxel) have
// 56 taps on 32 distinct voxels: i0 + {-1 .. 2} on one axis, {0, 1} on the other two.  Those voxels span at most two blocks per
// axis; the lane resolves the block slots it needs (at most 8, each probed once, one when the neighbourhood lies inside a block),
// loads the 32 (weight, distance) pairs once and forms the samples from registers.  A tap of a missing block reads slot 0 and is
// masked, so the loads are issued together, without a branch per tap.  No LDS.
#pragma once
#include "khr_device.h"
#include "khr_map_read.h"

namespace khr {

enum QueryStat : int { QS_VALUE = 0, QS_GRADIENT, QS_VOXEL, QS_COUNT = 4 };
constexpr uint32_t kQpValue = 1u, kQpGradient = 2u, kQpVoxel = 4u;  // KHR_QP_*

struct QueryPoints {
  long long n;
  const float* points;  // 3 per point
  float min_weight;
  float* distance;  // every output may be null
  float* gradient;  // 3 per point
  float* weight;
  uint32_t* color;
  uint32_t* label;
  uint8_t* vflags;
  uint64_t* last_observed;
  uint8_t* status;
  unsigned long long* stats;  // QueryStat words, null when the caller wants none
};

// slot of block (lo + (hx, hy, hz)) out of the eight a neighbourhood can touch
__device__ inline uint32_t querySlot(const uint32_t (&s)[8], bool hx, bool hy, bool hz) {
  const uint32_t a0 = hx ? s[1] : s[0], a1 = hx ? s[3] : s[2], a2 = hx ? s[5] : s[4], a3 = hx ? s[7] : s[6];
  const uint32_t b0 = hy ? a1 : a0, b1 = hy ? a3 : a2;
  return hz ? b1 : b0;
}

template <int VPS>
__global__ __launch_bounds__(256) void k_query_points(DevMap m, DevParams p, QueryPoints q) {
  constexpr int NV = VPS * VPS * VPS, SH = VPS == 16 ? 4 : 3;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + static_cast<long long>(threadIdx.x);
  // what the null outputs leave to do (uniform): the status and the counters report all three bits
  const bool all_bits = q.status != nullptr || q.stats != nullptr;
  const bool want_grad = q.gradient != nullptr;
  const bool want_nbr = want_grad || all_bits;                // the 24 taps around the centre cube
  const bool want_value = q.distance != nullptr || want_nbr;  // the centre cube
  const bool want_attr = q.weight || q.color || q.label || q.vflags || q.last_observed;
  const bool want_voxel = want_attr || all_bits;
  uint32_t status = 0u;
  float dist = 0.f, grad[3] = {0.f, 0.f, 0.f}, weight = 0.f;
  uint32_t color = 0u, label = 0u;
  uint8_t vflags = 0;
  uint64_t last_obs = 0ull;
  if (i < q.n) {
    const float pw[3] = {q.points[3 * i], q.points[3 * i + 1], q.points[3 * i + 2]};
    float g[3], f[3];
    int i0[3];
    bool in_range = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      g[a] = pw[a] * p.vs_inv - 0.5f;
      in_range = in_range && (fabsf(g[a]) < kMapIndexLimit);  // (false for NaN)
    }
    if (in_range && want_value) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float fl = floorf(g[a]);
        i0[a] = static_cast<int>(fl);
        f[a] = g[a] - fl;  // (= g - float(i0): fl is that integer's exact float)
      }
      // per axis and offset o = k - 1 in -1 .. 2: the local index (scaled to the voxel's place in the block) and whether the
      // voxel lies in the upper of the axis' two blocks
      const int k_lo = want_nbr ? 0 : 1, k_hi = want_nbr ? 3 : 2;
      int lo[3], loc[3][4];
      bool up[3][4];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = (i0[a] + k_lo - 1) >> SH;  // floor division (arithmetic shift)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int x = i0[a] + k - 1;
          loc[a][k] = (x & (VPS - 1)) * (a == 0 ? 1 : (a == 1 ? VPS : VPS * VPS));
          up[a][k] = (x >> SH) != lo[a];
        }
      }
      // the blocks the taps fall into: bit (hx | hy << 1 | hz << 2).  A tap set is i0 + {k_lo - 1 .. k_hi - 1} on one axis and
      // {0, 1} on the others, so an axis contributes its upper block through the taps that are shifted along it or not at all.
      uint32_t need = 0u;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < k_lo || k > k_hi) continue;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const uint32_t sel = (static_cast<uint32_t>(up[a][k]) << a) | (static_cast<uint32_t>(up[b][1 + (t & 1)]) << b) |
                                 (static_cast<uint32_t>(up[c][1 + (t >> 1)]) << c);
            need |= 1u << sel;
          }
        }
      }
      uint32_t slots[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        slots[c] = kInvalidSlot;
        if ((need >> c) & 1u) {  // each block probed once
          const int bx = lo[0] + (c & 1), by = lo[1] + ((c >> 1) & 1), bz = lo[2] + (c >> 2);
          if (blockInKeyRange(bx, by, bz)) slots[c] = htLookup(m, packKey(bx, by, bz));
        }
      }
      // tap (kx, ky, kz) (offsets k - 1): observed?, *d = its distance when asked for
      auto tap = [&](int kx, int ky, int kz, bool with_d, float* d) -> bool {
        const uint32_t s = querySlot(slots, up[0][kx], up[1][ky], up[2][kz]);
        const bool found = s != kInvalidSlot;
        const size_t at = static_cast<size_t>(found ? s : 0u) * NV + static_cast<size_t>(loc[0][kx] + loc[1][ky] + loc[2][kz]);
        const float w = m.weight[at];
        if (with_d) *d = m.dist[at];
        return found && (w >= q.min_weight);
      };
      // seen bits: 0 .. 7 the centre cube (tap t), 8 + 4 k + j the x-shifted taps (k: 0 below, 1 above; j = z << 1 | y),
      // 16 + 4 k + j the y-shifted (j = z << 1 | x), 24 + 4 k + j the z-shifted (j = y << 1 | x)
      uint32_t seen = 0u;
      float c[8], ex[2][4], ey[2][4], ez[2][4];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        c[t] = 0.f;
        seen |= static_cast<uint32_t>(tap(1 + (t & 1), 1 + ((t >> 1) & 1), 1 + (t >> 2), true, &c[t])) << t;
      }
      if (want_nbr) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ex[k][j] = ey[k][j] = ez[k][j] = 0.f;
            seen |= static_cast<uint32_t>(tap(3 * k, 1 + (j & 1), 1 + (j >> 1), want_grad, &ex[k][j])) << (8 + 4 * k + j);
            seen |= static_cast<uint32_t>(tap(1 + (j & 1), 3 * k, 1 + (j >> 1), want_grad, &ey[k][j])) << (16 + 4 * k + j);
            seen |= static_cast<uint32_t>(tap(1 + (j & 1), 1 + (j >> 1), 3 * k, want_grad, &ez[k][j])) << (24 + 4 * k + j);
          }
      }
      if ((seen & 0xffu) == 0xffu) {
        status |= kQpValue;
        dist = trilinear(c, f);
      }
      if (want_nbr && seen == 0xffffffffu) {
        status |= kQpGradient;
        if (want_grad) {
          float vp[8], vm[8];
          const float scale = 0.5f * p.vs_inv;
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            vp[t] = (t & 1) ? ex[1][t >> 1] : c[t | 1];
            vm[t] = (t & 1) ? c[t & ~1] : ex[0][t >> 1];
          }
          grad[0] = (trilinear(vp, f) - trilinear(vm, f)) * scale;
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const int j = ((t >> 2) << 1) | (t & 1);
            vp[t] = (t & 2) ? ey[1][j] : c[t | 2];
            vm[t] = (t & 2) ? c[t & ~2] : ey[0][j];
          }
          grad[1] = (trilinear(vp, f) - trilinear(vm, f)) * scale;
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            vp[t] = (t & 4) ? ez[1][t & 3] : c[t | 4];
            vm[t] = (t & 4) ? c[t & ~4] : ez[0][t & 3];
          }
          grad[2] = (trilinear(vp, f) - trilinear(vm, f)) * scale;
        }
      }
    }
    if (in_range && want_voxel) {  // attribute voxel: floor(p * voxel_size_inv)
      float gi[3];
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        gi[a] = floorf(pw[a] * p.vs_inv);
        ok = ok && (fabsf(gi[a]) < kMapIndexLimit);
      }
      if (ok) {
        // (one of the centre cube's taps when those were read; probed on its own all the same: keeping the eight slots alive
        // down to here costs registers -- 97 VGPRs and SGPR spills against 96 and none -- for a probe that hits cached lines)
        const int ix = static_cast<int>(gi[0]), iy = static_cast<int>(gi[1]), iz = static_cast<int>(gi[2]);
        const int bx = ix >> SH, by = iy >> SH, bz = iz >> SH;
        const uint32_t s = blockInKeyRange(bx, by, bz) ? htLookup(m, packKey(bx, by, bz)) : kInvalidSlot;
        if (s != kInvalidSlot) {
          status |= kQpVoxel;
          const uint32_t lin = static_cast<uint32_t>((ix & (VPS - 1)) + VPS * ((iy & (VPS - 1)) + VPS * (iz & (VPS - 1))));
          const size_t at = static_cast<size_t>(s) * NV + lin;
          if (q.weight) weight = m.weight[at];
          if (q.color) color = m.color[at];
          if (q.label && p.with_semantics) label = m.sem_label[at];
          if (q.vflags) vflags = m.vflags[at] & VOX_PUBLIC_MASK;
          if (q.last_observed && p.with_tracking) last_obs = lastObserved(m, s, lin, NV);
        }
      }
    }
    if (q.distance) q.distance[i] = dist;
    if (q.gradient) {
      q.gradient[3 * i] = grad[0];
      q.gradient[3 * i + 1] = grad[1];
      q.gradient[3 * i + 2] = grad[2];
    }
    if (q.weight) q.weight[i] = weight;
    if (q.color) q.color[i] = color;
    if (q.label) q.label[i] = label;
    if (q.vflags) q.vflags[i] = vflags;
    if (q.last_observed) q.last_observed[i] = last_obs;
    if (q.status) q.status[i] = static_cast<uint8_t>(status);
  }
  if (q.stats) {  // one atomic per wave and counter
    waveStatAdd(q.stats + QS_VALUE, (status & kQpValue) ? 1u : 0u);
    waveStatAdd(q.stats + QS_GRADIENT, (status & kQpGradient) ? 1u : 0u);
    waveStatAdd(q.stats + QS_VOXEL, (status & kQpVoxel) ? 1u : 0u);
  }
}

}  // namespace khr
