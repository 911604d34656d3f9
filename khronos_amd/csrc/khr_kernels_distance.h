// khr_kernels_distance.h — the exact Euclidean distance field of a box of the live map (khr_distance_field; ASSUMPTIONS.md A.15).
// Reads the map only.  gfx950, wave64.  Everything between the gather and the finish is int32 arithmetic in squared cell units.
//
// Shape: k_df_gather, one workgroup per block index the box overlaps (one hash probe per workgroup), classifies the block's
// cells and writes the two seed grids (0 at a site, kDfFar elsewhere) in the output order x + nx * (y + ny * z).  k_df_pass<AXIS>
// then runs g(i) = min over |i - j| <= R of f(j) + (i - j)^2 along x, y and z in place: a workgroup loads whole lines into LDS,
// waits, and every lane walks outwards from its own cell until k^2 reaches its best value.  Values never exceed kDfFar (a
// candidate that does is no improvement on the start value min(f(i), kDfFar)), so nothing wraps.  The x pass takes consecutive
// lines as one contiguous run; the y and z passes take a strip of kDfStrip adjacent x, so that global accesses stay contiguous
// along x and the lanes of a wave (16 x by 4 consecutive line positions) touch 64 consecutive LDS words in every step: no bank
// conflicts.  The inner transform (distance of an obstacle cell to free space) is the same three launches on the second grid.
#pragma once
#include "khr_device.h"
#include "khr_map_read.h"

namespace khr {

enum DfStat : int { DFS_OBSERVED = 0, DFS_OBSTACLE, DFS_IN_RANGE, DFS_COUNT = 4 };
constexpr int32_t kDfFar = 1 << 30;                                // KHR_DF_FAR
constexpr uint32_t kDfObserved = 1u, kDfObstacle = 2u, kDfInRange = 4u;  // KHR_DF_*
constexpr int kDfStrip = 16;          // adjacent x of a y / z pass tile
constexpr int kDfTileCells = 8192;    // cells of a pass tile: 32 KB of LDS, a 512-long line times the strip

struct DfBox {
  int ox, oy, oz;     // first cell
  int nx, ny, nz;     // cells per axis
  int bx0, by0, bz0;  // first block index the box overlaps
};

struct DfGather {
  DfBox box;
  float min_weight, surface_distance;
  int unknown_is_obstacle;
  int32_t* outer;   // seed: 0 in the obstacle set O
  int32_t* inner;   // seed: 0 at FREE cells; null with positive_only
  uint8_t* status;  // bits 0 and 1; may be null
  unsigned long long* stats;  // DfStat words, null when the caller wants none
};

// the minimum distance over the observed voxels of the RATIO^3 cell whose first voxel is (vx, vy, vz) of the block whose weight
// and distance layers are `w` and `d`; false when none of them is observed
template <int VPS, int RATIO>
__device__ inline bool dfCell(const float* __restrict__ w, const float* __restrict__ d, int vx, int vy, int vz, float min_weight, float* value) {
  bool seen = false;
  float v = 0.f;
#pragma unroll
  for (int dz = 0; dz < RATIO; ++dz)
#pragma unroll
    for (int dy = 0; dy < RATIO; ++dy) {
      const int row = vx + VPS * ((vy + dy) + VPS * (vz + dz));  // RATIO consecutive voxels: one vector load per layer
      float wr[RATIO], dr[RATIO];
      if constexpr (RATIO == 4) {
        const float4 a = *reinterpret_cast<const float4*>(w + row), b = *reinterpret_cast<const float4*>(d + row);
        wr[0] = a.x, wr[1] = a.y, wr[2] = a.z, wr[3] = a.w, dr[0] = b.x, dr[1] = b.y, dr[2] = b.z, dr[3] = b.w;
      } else if constexpr (RATIO == 2) {
        const float2 a = *reinterpret_cast<const float2*>(w + row), b = *reinterpret_cast<const float2*>(d + row);
        wr[0] = a.x, wr[1] = a.y, dr[0] = b.x, dr[1] = b.y;
      } else {
        wr[0] = w[row], dr[0] = d[row];
      }
#pragma unroll
      for (int dx = 0; dx < RATIO; ++dx)
        if (wr[dx] >= min_weight) {
          v = seen ? fminf(v, dr[dx]) : dr[dx];
          seen = true;
        }
    }
  *value = v;
  return seen;
}

template <int VPS, int RATIO>
__global__ __launch_bounds__(256) void k_df_gather(DevMap m, DfGather g) {
  static_assert(VPS % RATIO == 0, "a cell never straddles a block");
  constexpr int CPS = VPS / RATIO, CPB = CPS * CPS * CPS, NV = VPS * VPS * VPS;
  const int bx = g.box.bx0 + static_cast<int>(blockIdx.x), by = g.box.by0 + static_cast<int>(blockIdx.y), bz = g.box.bz0 + static_cast<int>(blockIdx.z);
  const uint32_t slot = blockInKeyRange(bx, by, bz) ? htLookup(m, packKey(bx, by, bz)) : kInvalidSlot;  // (uniform)
  const float* const w = m.weight + static_cast<size_t>(slot == kInvalidSlot ? 0u : slot) * NV;
  const float* const d = m.dist + static_cast<size_t>(slot == kInvalidSlot ? 0u : slot) * NV;
  uint32_t n_obs = 0u, n_obst = 0u;
  for (int c0 = 0; c0 < CPB; c0 += 256) {  // (uniform trip count: every lane reaches the wave sums below)
    const int c = c0 + static_cast<int>(threadIdx.x);
    if (c >= CPB) continue;
    const int lx = c % CPS, ly = (c / CPS) % CPS, lz = c / (CPS * CPS);
    const int cx = bx * CPS + lx - g.box.ox, cy = by * CPS + ly - g.box.oy, cz = bz * CPS + lz - g.box.oz;  // (|block * CPS| < 2^30: checked by the host)
    if (cx < 0 || cx >= g.box.nx || cy < 0 || cy >= g.box.ny || cz < 0 || cz >= g.box.nz) continue;
    float v = 0.f;
    const bool observed = slot != kInvalidSlot && dfCell<VPS, RATIO>(w, d, lx * RATIO, ly * RATIO, lz * RATIO, g.min_weight, &v);
    const bool obstacle = observed && v <= g.surface_distance;
    const bool in_set = obstacle || (!observed && g.unknown_is_obstacle != 0);
    const size_t at = static_cast<size_t>(cx) + static_cast<size_t>(g.box.nx) * (static_cast<size_t>(cy) + static_cast<size_t>(g.box.ny) * static_cast<size_t>(cz));
    g.outer[at] = in_set ? 0 : kDfFar;
    if (g.inner) g.inner[at] = (observed && !obstacle) ? 0 : kDfFar;
    if (g.status) g.status[at] = static_cast<uint8_t>((observed ? kDfObserved : 0u) | (obstacle ? kDfObstacle : 0u));
    n_obs += observed ? 1u : 0u;
    n_obst += obstacle ? 1u : 0u;
  }
  if (g.stats) {
    waveStatAdd(g.stats + DFS_OBSERVED, n_obs);
    waveStatAdd(g.stats + DFS_OBSTACLE, n_obst);
  }
}

// the windowed minimum at position i of a line of `len` values `stride` LDS words apart, `at` = the word of position i
__device__ inline int32_t dfWindowMin(const int32_t* tile, int at, int stride, int i, int len, int R) {
  int32_t best = tile[at];
  const int kmax = R < len - 1 ? R : len - 1;
  for (int k = 1; k <= kmax; ++k) {
    const int32_t kk = k * k;
    if (kk >= best) break;  // nothing further out can improve
    if (i - k >= 0) {
      const int32_t cand = tile[at - k * stride] + kk;  // (<= 2^30 + 32767^2 < 2^31)
      best = cand < best ? cand : best;
    }
    if (i + k < len) {
      const int32_t cand = tile[at + k * stride] + kk;
      best = cand < best ? cand : best;
    }
  }
  return best;
}

// AXIS 0: the grid is ny * nz lines of nx contiguous values; a workgroup takes per_wg consecutive lines (per_wg * nx <= kDfTileCells).
// AXIS 1 / 2: lines along y / z; a workgroup takes kDfStrip adjacent x of per_wg consecutive "other" indices (z for the y pass,
// y for the z pass; per_wg * line length * kDfStrip <= kDfTileCells).  The host sizes per_wg.
template <int AXIS>
__global__ __launch_bounds__(256) void k_df_pass(int32_t* __restrict__ grid, int nx, int ny, int nz, int R, int per_wg) {
  __shared__ int32_t tile[kDfTileCells];
  const int tid = static_cast<int>(threadIdx.x);
  if constexpr (AXIS == 0) {
    const long long n_lines = static_cast<long long>(ny) * nz;
    const long long first = static_cast<long long>(blockIdx.x) * per_wg;
    const long long rest = n_lines - first;
    const int lines = static_cast<int>(rest < per_wg ? rest : per_wg);
    const int cells = lines * nx;
    int32_t* const base = grid + first * nx;
    for (int c = tid; c < cells; c += 256) tile[c] = base[c];
    __syncthreads();
    for (int c = tid; c < cells; c += 256) base[c] = dfWindowMin(tile, c, 1, c % nx, nx, R);
  } else {
    const int len = AXIS == 1 ? ny : nz, n_other = AXIS == 1 ? nz : ny;
    const int x0 = static_cast<int>(blockIdx.x) * kDfStrip;
    const int o0 = static_cast<int>(blockIdx.y) * per_wg;
    const int groups = n_other - o0 < per_wg ? n_other - o0 : per_wg;
    const int cells = groups * len * kDfStrip;
    const size_t step = AXIS == 1 ? static_cast<size_t>(nx) : static_cast<size_t>(nx) * ny;        // between line positions
    const size_t other = AXIS == 1 ? static_cast<size_t>(nx) * ny : static_cast<size_t>(nx);       // between groups
    const int xs = tid % kDfStrip;
    const bool live = x0 + xs < nx;
    // word c of the tile: x = c % strip, line position i = (c / strip) % len, group = c / (strip * len)
    for (int c = tid; c < cells; c += 256) {
      const int r = c / kDfStrip, i = r % len, gq = r / len;
      if (live) tile[c] = grid[static_cast<size_t>(x0 + xs) + step * i + other * (o0 + gq)];
    }
    __syncthreads();
    for (int c = tid; c < cells; c += 256) {
      const int r = c / kDfStrip, i = r % len, gq = r / len;
      if (live) grid[static_cast<size_t>(x0 + xs) + step * i + other * (o0 + gq)] = dfWindowMin(tile, c, kDfStrip, i, len, R);
    }
  }
}

struct DfFinish {
  long long n;
  const int32_t* outer;
  const int32_t* inner;  // null with positive_only
  int32_t r2;            // R^2
  float cell_size, max_distance;
  float* distance;  // every output may be null
  int32_t* d2;
  uint8_t* status;  // bit 2 is added to what k_df_gather wrote
  unsigned long long* stats;
};

__global__ __launch_bounds__(256) void k_df_finish(DfFinish f) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + static_cast<long long>(threadIdx.x);
  uint32_t in_range = 0u;
  if (i < f.n) {
    const int32_t a = f.outer[i];
    const bool in_set = a == 0;  // (a cell outside O is at least one cell away from it)
    int32_t mag = in_set ? (f.inner ? f.inner[i] : 0) : a;
    in_range = mag <= f.r2 ? 1u : 0u;
    float dist;
    if (in_range) {
      // the correctly rounded float root: the double root of an integer below 2^24, rounded once more (53 >= 2 * 24 + 2 bits, so
      // the second rounding cannot change the result)
      dist = f.cell_size * static_cast<float>(sqrt(static_cast<double>(mag)));
    } else {
      mag = kDfFar;
      dist = f.max_distance;
    }
    const bool neg = in_set && f.inner != nullptr;
    if (f.distance) f.distance[i] = neg ? -dist : dist;
    if (f.d2) f.d2[i] = neg ? -mag : mag;
    if (f.status && in_range) f.status[i] = static_cast<uint8_t>(f.status[i] | kDfInRange);
  }
  if (f.stats) waveStatAdd(f.stats + DFS_IN_RANGE, in_range);
}

}  // namespace khr
