// khr_kernels_align.h — the live map as a registration target (khr_align_linearize; ASSUMPTIONS.md A.14): per source point the
// residual d (A.13's trilinear distance at the transformed point) and the Jacobian J = (q x g, g) of a twist about the sensor
// origin, summed over the inliers as 27 fixed-point products (the upper triangle of J^T J, J^T d), the weighted squared residual,
// the weight sum and three counts.  Reads the map only.  gfx950, wave64.
//
// Shape: one lane per source point, one 256-thread workgroup per 256 sources, no tile loop (the kernel arguments are dead before
// the neighbourhood is read, which keeps the SGPRs free of spills).  Per lane the neighbourhood of k_query_points -- the 32
// distinct voxels of the seven samples, each block probed once, the taps of a missing block masked -- in this file's own copy.  The sums are 64-bit integers, so they neither depend on the order of the points nor on how the lanes,
// waves and workgroups split them:
//   lane   one product at a time: two double multiplies, the scaling by 2^24, round-to-nearest-even to an integer;
//   wave   each word is reduced right away with DPP row shifts and row broadcasts (VALU only: 6 steps of two v_mov_dpp and a
//          64-bit add), so that no lane keeps 28 accumulators alive;
//   group  the last lane of a wave stores the wave's word in the wave's row of a 4 x 32 LDS table;
//   grid   after one barrier 32 threads add the four rows and issue one non-returning 64-bit atomic per non-zero word into the
//          accumulator, whose words lie 128 bytes apart (a line each).
#pragma once
#include "khr_device.h"
#include "khr_map_read.h"

namespace khr {

constexpr int kAlignWords = 32;        // H (21), b (6), e, n_inlier, n_gradient, n_source, sum of w * rho
constexpr int kAlignAccStride = 16;    // 64-bit words between two accumulator words on the device (128 bytes)
constexpr int AW_B = 21, AW_E = 27, AW_INLIER = 28, AW_GRADIENT = 29, AW_SOURCE = 30, AW_WEIGHT = 31;
constexpr float kAlignMaxGradSq = 16.f, kAlignMaxArm = 64.f;

enum AlignSrc : int { ALIGN_POINTS = 0, ALIGN_DEPTH = 1 };

struct AlignArgs {
  uint32_t n;            // lanes: points, or pixels of the strided grid (ws * hs); at most 2^20
  const float* points;   // ALIGN_POINTS: 3 per point, source frame
  const float* depth;    // ALIGN_DEPTH: W * H
  const float* weights;  // per point / per pixel, null = 1
  uint32_t W, ws, stride;  // image width, width of the strided grid
  float fx, fy, cx, cy, min_range, max_range;
  float Rw[9], tw[3];    // world_T_source as frame ingest has it (makePose)
  float min_weight, gate, huber_delta;
  unsigned long long* acc;  // kAlignWords * kAlignAccStride words, zeroed in stream order before the launch
};

// A.13's distance and gradient at pw; true iff the point has KHR_QP_GRADIENT (all 32 voxels observed), else both are untouched.
// slot_tab: the workgroup's 8 x 256 table of block slots, entry [c][thread] -- a lane reads and writes its own column only (no
// barrier), consecutive lanes sit on consecutive banks.  Which of the eight blocks a tap falls into is carried as three bits above
// the tap's voxel offset, so that a tap costs two adds, a shift and one LDS read instead of a select chain over twelve lane masks
// (which the compiler keeps in 24 SGPRs and then spills).
template <int VPS>
__device__ inline bool alignSample(const DevMap& m, const DevParams& p, const float* pw, float min_weight, uint32_t* slot_tab, float* dist,
                                   float* grad) {
  constexpr int NV = VPS * VPS * VPS, SH = VPS == 16 ? 4 : 3;
  float f[3], gi[3];
  int i0[3];
  bool in_range = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    gi[a] = pw[a] * p.vs_inv - 0.5f;
    in_range = in_range && (fabsf(gi[a]) < kMapIndexLimit);  // (false for NaN)
  }
  // (a point with no voxel is sampled at index 0 and its result dropped: one level of divergent control less than a branch)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float g = in_range ? gi[a] : 0.f;
    const float fl = floorf(g);
    i0[a] = static_cast<int>(fl);
    f[a] = g - fl;
  }
  // per axis and offset o = k - 1 in -1 .. 2: the voxel's place in its block (bits 0 .. 11) and, at bit 16 + axis, whether it lies in
  // the upper of the axis' two blocks
  int lo[3], loc[3][4];
  uint32_t need = 0u;  // the blocks the taps fall into: bit (hx | hy << 1 | hz << 2)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = (i0[a] - 1) >> SH;  // floor division (arithmetic shift)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = i0[a] + k - 1;
      loc[a][k] = ((x & (VPS - 1)) * (a == 0 ? 1 : (a == 1 ? VPS : VPS * VPS))) | (((x >> SH) - lo[a]) << (16 + a));
    }
  }
  // a tap set is i0 + {-1 .. 2} on one axis and {0, 1} on the others
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int t = 0; t < 4; ++t) need |= 1u << (static_cast<uint32_t>(loc[a][k] + loc[b][1 + (t & 1)] + loc[c][1 + (t >> 1)]) >> 16);
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    uint32_t s = kInvalidSlot;
    if ((need >> c) & 1u) {  // each block probed once
      const int bx = lo[0] + (c & 1), by = lo[1] + ((c >> 1) & 1), bz = lo[2] + (c >> 2);
      if (blockInKeyRange(bx, by, bz)) s = htLookup(m, packKey(bx, by, bz));
    }
    slot_tab[c * 256] = s;
  }
  // tap (kx, ky, kz) (offsets k - 1): observed?, *d = its distance; a tap of a missing block reads slot 0 and is masked
  auto tap = [&](int kx, int ky, int kz, float* d) -> bool {
    const uint32_t at_sel = static_cast<uint32_t>(loc[0][kx] + loc[1][ky] + loc[2][kz]);
    const uint32_t s = slot_tab[(at_sel >> 16) * 256];
    const bool found = s != kInvalidSlot;
    const size_t at = static_cast<size_t>(found ? s : 0u) * NV + static_cast<size_t>(at_sel & 0xffffu);
    const float w = m.weight[at];
    *d = m.dist[at];
    return found && (w >= min_weight);
  };
  bool seen = true;
  float c[8], ex[2][4], ey[2][4], ez[2][4];
#pragma unroll
  for (int t = 0; t < 8; ++t) seen = tap(1 + (t & 1), 1 + ((t >> 1) & 1), 1 + (t >> 2), &c[t]) && seen;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      seen = tap(3 * k, 1 + (j & 1), 1 + (j >> 1), &ex[k][j]) && seen;
      seen = tap(1 + (j & 1), 3 * k, 1 + (j >> 1), &ey[k][j]) && seen;
      seen = tap(1 + (j & 1), 1 + (j >> 1), 3 * k, &ez[k][j]) && seen;
    }
  if (!(seen && in_range)) return false;
  *dist = trilinear(c, f);
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
  return true;
}

// llrint(ldexp(w * (a * b), 24)) for |result| < 2^51: adding 1.5 * 2^52 rounds the scaled product to an integer, to nearest even
// (the default rounding of the double add), and leaves that integer in the low bits of the sum's representation
__device__ inline long long alignTerm(double w, double a, double b) {
  constexpr double kMagic = 6755399441055744.0;  // 1.5 * 2^52
  const double x = ldexp(w * (a * b), 24) + kMagic;
  return __double_as_longlong(x) - __double_as_longlong(kMagic);
}

// the wave's sum of v in lane 63: an inclusive scan over each row of 16 lanes (row_shr 1, 2, 4, 8; lanes shifted in from outside
// the row read zero), then row 0's and row 2's totals go to rows 1 and 3 (row_bcast:15), then row 1's to rows 2 and 3
// (row_bcast:31).  DPP moves are VALU operations and leave the LDS pipe to the map loads' address traffic.
template <int CTRL, int ROW_MASK>
__device__ inline unsigned long long alignDppAdd(unsigned long long v) {
  const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(v)), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<uint32_t>(v >> 32)), CTRL, ROW_MASK, 0xf, false);
  return v + ((static_cast<unsigned long long>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo));
}
__device__ inline unsigned long long alignWaveSum(unsigned long long v) {
  v = alignDppAdd<0x111, 0xf>(v);  // row_shr:1
  v = alignDppAdd<0x112, 0xf>(v);  // row_shr:2
  v = alignDppAdd<0x114, 0xf>(v);  // row_shr:4
  v = alignDppAdd<0x118, 0xf>(v);  // row_shr:8
  v = alignDppAdd<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = alignDppAdd<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
  return v;
}

template <int VPS, int SRC>
__global__ __launch_bounds__(256) void k_align_linearize(DevMap m, DevParams p, AlignArgs a) {
  __shared__ unsigned long long part[4][kAlignWords];
  __shared__ uint32_t slot_tab[8 * 256];
  const int wave = static_cast<int>(threadIdx.x) >> 6;
  const bool last_lane = (threadIdx.x & 63u) == 63u;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool source = false, has_grad = false, inlier = false;
  float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, d = 0.f, wr = 0.f;
  {
    // (a lane past the end reads the last source and is no source)
    const uint32_t ic = i < a.n ? i : a.n - 1u;
    float pc[3] = {0.f, 0.f, 0.f};
    uint32_t wi = ic;
    if (SRC == ALIGN_POINTS) {
      source = i < a.n;
      pc[0] = a.points[3 * ic];
      pc[1] = a.points[3 * ic + 1];
      pc[2] = a.points[3 * ic + 2];
    } else {
      const uint32_t u = (ic % a.ws) * a.stride, v = (ic / a.ws) * a.stride;
      wi = v * a.W + u;  // (below 2^30: the image size is checked)
      const float z = a.depth[wi];
      source = i < a.n && z > 0.f && isfinite(z) && z >= a.min_range && z <= a.max_range;
      pc[0] = ((static_cast<float>(u) - a.cx) / a.fx) * z;
      pc[1] = ((static_cast<float>(v) - a.cy) / a.fy) * z;
      pc[2] = z;
    }
    if (source) {
      // everything that does not need the map first: the pose, the weight pointer and the image geometry are dead (their SGPRs
      // free) before the neighbourhood is read
      float pw[3], g[3] = {0.f, 0.f, 0.f};
      xform(a.Rw, a.tw, pc[0], pc[1], pc[2], pw);
      const float w = a.weights ? a.weights[wi] : 1.f;
      const float q[3] = {pw[0] - a.tw[0], pw[1] - a.tw[1], pw[2] - a.tw[2]};
      has_grad = alignSample<VPS>(m, p, pw, a.min_weight, slot_tab + threadIdx.x, &d, g);
      // (selects, not branches: every level of divergent control costs an SGPR pair for its lane mask)
      const float ad = fabsf(d);
      inlier = has_grad && (ad <= a.gate) && (((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) <= kAlignMaxGradSq) && (fabsf(q[0]) < kAlignMaxArm) &&
               (fabsf(q[1]) < kAlignMaxArm) && (fabsf(q[2]) < kAlignMaxArm) && (w > 0.f) && (w <= 1.f);
      const float rho = (a.huber_delta == 0.f || ad <= a.huber_delta) ? 1.f : a.huber_delta / ad;
      wr = inlier ? w * rho : 0.f;
      d = inlier ? d : 0.f;
      J[0] = inlier ? q[1] * g[2] - q[2] * g[1] : 0.f;
      J[1] = inlier ? q[2] * g[0] - q[0] * g[2] : 0.f;
      J[2] = inlier ? q[0] * g[1] - q[1] * g[0] : 0.f;
      J[3] = inlier ? g[0] : 0.f;
      J[4] = inlier ? g[1] : 0.f;
      J[5] = inlier ? g[2] : 0.f;
    }
  }
  // (a lane that is no inlier carries wr = 0, J = 0, d = 0: its products are exact zeros)
  const double wd = static_cast<double>(wr), dd = static_cast<double>(d);
  int word = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c, ++word) {
      const unsigned long long s = alignWaveSum(static_cast<unsigned long long>(alignTerm(wd, static_cast<double>(J[r]), static_cast<double>(J[c]))));
      if (last_lane) part[wave][word] = s;
    }
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const unsigned long long s = alignWaveSum(static_cast<unsigned long long>(alignTerm(wd, static_cast<double>(J[r]), dd)));
    if (last_lane) part[wave][AW_B + r] = s;
  }
  {
    const unsigned long long s = alignWaveSum(static_cast<unsigned long long>(alignTerm(wd, dd, dd)));
    if (last_lane) part[wave][AW_E] = s;
  }
  {
    const unsigned long long s = alignWaveSum(static_cast<unsigned long long>(alignTerm(wd, 1.0, 1.0)));
    if (last_lane) part[wave][AW_WEIGHT] = s;
  }
  const unsigned long long n_in = __popcll(__ballot(inlier)), n_gr = __popcll(__ballot(has_grad)), n_src = __popcll(__ballot(source));
  if (last_lane) {
    part[wave][AW_INLIER] = n_in;
    part[wave][AW_GRADIENT] = n_gr;
    part[wave][AW_SOURCE] = n_src;
  }
  __syncthreads();
  if (threadIdx.x < kAlignWords) {
    const unsigned long long s = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
    if (s) atomicAdd(a.acc + static_cast<size_t>(threadIdx.x) * kAlignAccStride, s);
  }
}

}  // namespace khr
