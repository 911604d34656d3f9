// khr_kernels_voronoi.h — nearest obstacle cell (site) and generalized Voronoi cells of a box of the live map (khr_voronoi_field;
// ASSUMPTIONS.md A.20).  Reads the map only.  gfx950, wave64.  Integer arithmetic throughout, apart from the double root of the
// distance and of the angle test.
//
// Shape: k_df_gather (khr_kernels_distance.h, unchanged) classifies the cells and writes the int32 seeds.  k_vor_pass<AXIS> is
// k_df_pass on 64-bit keys (value << 32 | site): g(i) = min over |i - j| <= R of key(j) + ((i - j)^2 << 32), so that among equal
// values the least site index wins; a key whose value reaches kDfFar is reset to kVorFarKey.  The x pass reads the seeds and writes
// the keys (out of place), the y and z passes run in place.  The tiling is k_df_pass's: whole lines in LDS, x as contiguous runs,
// y / z as strips of kDfStrip adjacent x.  A 512-long line times the 16-wide strip of 8-byte keys is exactly 64 KB of static LDS
// (two workgroups per CU); a wave's lanes (16 x by 4 consecutive line positions) touch 64 consecutive keys = 512 contiguous bytes
// per step, which ds_read_b64 serves in its two lane groups without a bank conflict.  The walk stops only when k^2 EXCEEDS the
// best value: a site further out whose k^2 equals it ties the value and may have the smaller index.
// k_vor_classify, one lane per cell, unpacks the key into distance / d2 / the in-range bit / site, applies the basis rule to the
// 26 neighbours' keys with the basis in registers, and leaves the counters and a per-workgroup count of listed cells;
// after a scan of those counts k_vor_emit writes the list in ascending linear order (workgroup base + ballot rank).
#pragma once
#include "khr_kernels_distance.h"

namespace khr {

// the counter words: k_df_gather and the in-range count keep their DfStat places
enum VorStat : int { VS_ELIGIBLE = DFS_COUNT, VS_BASIS2, VS_BASIS3, VS_BASIS4, VS_LISTED, VS_COUNT };
constexpr uint64_t kVorFarKey = (static_cast<uint64_t>(kDfFar) << 32) | 0xFFFFFFFFull;
constexpr int kVorTileCells = 8192;  // keys of a pass tile: 64 KB of LDS
constexpr int kVorL1 = 0, kVorAngle = 1, kVorL1ThenAngle = 2, kVorMaxBasis = 4;  // KHR_VOR_*

// the windowed minimum at position i of a line of `len` keys `stride` LDS words apart, `at` = the word of position i
__device__ inline uint64_t vorWindowMin(const uint64_t* tile, int at, int stride, int i, int len, int R) {
  uint64_t best = tile[at];
  const int kmax = R < len - 1 ? R : len - 1;
  for (int k = 1; k <= kmax; ++k) {
    const uint64_t kk = static_cast<uint64_t>(k * k);
    if (kk > (best >> 32)) break;  // (not >=: a tie further out may carry the smaller site)
    if (i - k >= 0) {
      const uint64_t cand = tile[at - k * stride] + (kk << 32);  // (value <= 2^30 + 32767^2 < 2^31)
      best = cand < best ? cand : best;
    }
    if (i + k < len) {
      const uint64_t cand = tile[at + k * stride] + (kk << 32);
      best = cand < best ? cand : best;
    }
  }
  return (best >> 32) >= static_cast<uint64_t>(kDfFar) ? kVorFarKey : best;
}

// AXIS 0: reads the seeds (0 in O), writes the keys; a workgroup takes per_wg consecutive lines (per_wg * nx <= kVorTileCells).
// AXIS 1 / 2: in place on the keys; kDfStrip adjacent x of per_wg consecutive "other" indices, as k_df_pass.  The host sizes per_wg.
template <int AXIS>
__global__ __launch_bounds__(256) void k_vor_pass(const int32_t* __restrict__ seed, uint64_t* __restrict__ keys, int nx, int ny, int nz, int R, int per_wg) {
  __shared__ uint64_t tile[kVorTileCells];
  const int tid = static_cast<int>(threadIdx.x);
  if constexpr (AXIS == 0) {
    const long long n_lines = static_cast<long long>(ny) * nz;
    const long long first = static_cast<long long>(blockIdx.x) * per_wg;
    const long long rest = n_lines - first;
    const int lines = static_cast<int>(rest < per_wg ? rest : per_wg);
    const int cells = lines * nx;
    const long long base = first * nx;  // (the linear index of the tile's first cell; the box has at most 2^24 cells)
    for (int c = tid; c < cells; c += 256) tile[c] = seed[base + c] == 0 ? static_cast<uint64_t>(base + c) : kVorFarKey;
    __syncthreads();
    for (int c = tid; c < cells; c += 256) keys[base + c] = vorWindowMin(tile, c, 1, c % nx, nx, R);
  } else {
    const int len = AXIS == 1 ? ny : nz, n_other = AXIS == 1 ? nz : ny;
    const int x0 = static_cast<int>(blockIdx.x) * kDfStrip;
    const int o0 = static_cast<int>(blockIdx.y) * per_wg;
    const int groups = n_other - o0 < per_wg ? n_other - o0 : per_wg;
    const int cells = groups * len * kDfStrip;
    const size_t step = AXIS == 1 ? static_cast<size_t>(nx) : static_cast<size_t>(nx) * ny;   // between line positions
    const size_t other = AXIS == 1 ? static_cast<size_t>(nx) * ny : static_cast<size_t>(nx);  // between groups
    const int xs = tid % kDfStrip;
    const bool live = x0 + xs < nx;
    // key c of the tile: x = c % strip, line position i = (c / strip) % len, group = c / (strip * len)
    for (int c = tid; c < cells; c += 256) {
      const int r = c / kDfStrip, i = r % len, gq = r / len;
      if (live) tile[c] = keys[static_cast<size_t>(x0 + xs) + step * i + other * (o0 + gq)];
    }
    __syncthreads();
    for (int c = tid; c < cells; c += 256) {
      const int r = c / kDfStrip, i = r % len, gq = r / len;
      if (live) keys[static_cast<size_t>(x0 + xs) + step * i + other * (o0 + gq)] = vorWindowMin(tile, c, kDfStrip, i, len, R);
    }
  }
}

struct VorRule {
  int32_t r2;  // R^2
  float cell_size, max_distance, min_distance;
  int mode, l1_sep;
  float cos_sep;
  int min_basis;  // 2 .. 4
};

struct VorField {
  int ox, oy, oz;  // first cell
  int nx, ny, nz;
  const uint64_t* keys;
  VorRule rule;
  float* distance;  // the dense outputs, x + nx * (y + ny * z)
  int32_t* d2;
  uint8_t* status;  // bit 2 is added to what k_df_gather wrote
  int32_t* site;
  uint8_t* basis;
  uint32_t* wg_count;  // listed cells per workgroup of k_vor_classify; scanned in place before k_vor_emit
  unsigned long long* stats;  // VorStat words
  // the list (k_vor_emit)
  uint32_t n_listed;
  int32_t* cells;
  float* cell_distance;
  uint8_t* cell_basis;
  int32_t* cell_sites;
};

// a cell outside O within range has a site
__device__ inline bool vorHasSite(uint64_t key, int32_t r2) {
  const uint32_t v = static_cast<uint32_t>(key >> 32);
  return v != 0u && v <= static_cast<uint32_t>(r2);
}

// are the sites p and q separated as seen from cell c (A.20)
__device__ inline bool vorSeparated(const VorRule& r, int cx, int cy, int cz, int px, int py, int pz, int qx, int qy, int qz) {
  if (px == qx && py == qy && pz == qz) return false;
  const int l1 = abs(px - qx) + abs(py - qy) + abs(pz - qz);
  if (r.mode != kVorAngle && l1 >= r.l1_sep) return true;
  if (r.mode == kVorL1) return false;
  const int ax = px - cx, ay = py - cy, az = pz - cz, bx = qx - cx, by = qy - cy, bz = qz - cz;  // (|.| < 512)
  const int dot = ax * bx + ay * by + az * bz, aa = ax * ax + ay * ay + az * az, bb = bx * bx + by * by + bz * bz;
  // aa * bb < 2^40: the product is exact, the root correctly rounded
  return static_cast<double>(dot) <= static_cast<double>(r.cos_sep) * sqrt(static_cast<double>(aa) * static_cast<double>(bb));
}

// the basis of the eligible cell (x, y, z) whose own site is `own`: entries in sx / sy / sz (box-local), their number returned.
// The arrays are only indexed by constants once the inner loops are unrolled: they stay in registers.
__device__ inline int vorBasis(const VorField& f, int x, int y, int z, uint32_t own, int (&sx)[kVorMaxBasis], int (&sy)[kVorMaxBasis], int (&sz)[kVorMaxBasis]) {
  const uint32_t unx = static_cast<uint32_t>(f.nx), uplane = static_cast<uint32_t>(f.nx) * static_cast<uint32_t>(f.ny);
#pragma unroll
  for (int j = 0; j < kVorMaxBasis; ++j) sx[j] = sy[j] = sz[j] = 0;
  sx[0] = static_cast<int>(own % unx), sy[0] = static_cast<int>((own / unx) % static_cast<uint32_t>(f.ny)), sz[0] = static_cast<int>(own / uplane);
  int nb = 1;
#pragma unroll 1
  for (int t = 0; t < 27 && nb < kVorMaxBasis; ++t) {  // dz outer, dy middle, dx inner
    if (t == 13) continue;
    const int X = x + t % 3 - 1, Y = y + (t / 3) % 3 - 1, Z = z + t / 9 - 1;
    if (X < 0 || X >= f.nx || Y < 0 || Y >= f.ny || Z < 0 || Z >= f.nz) continue;
    const uint64_t key = f.keys[static_cast<size_t>(X) + static_cast<size_t>(f.nx) * (static_cast<size_t>(Y) + static_cast<size_t>(f.ny) * static_cast<size_t>(Z))];
    if (!vorHasSite(key, f.rule.r2)) continue;
    const uint32_t q = static_cast<uint32_t>(key);
    const int qx = static_cast<int>(q % unx), qy = static_cast<int>((q / unx) % static_cast<uint32_t>(f.ny)), qz = static_cast<int>(q / uplane);
    bool apart = true;
#pragma unroll
    for (int j = 0; j < kVorMaxBasis; ++j)
      if (j < nb && apart) apart = vorSeparated(f.rule, x, y, z, sx[j], sy[j], sz[j], qx, qy, qz);
    if (!apart) continue;
#pragma unroll
    for (int j = 1; j < kVorMaxBasis; ++j)
      if (j == nb) sx[j] = qx, sy[j] = qy, sz[j] = qz;
    ++nb;
  }
  return nb;
}

__global__ __launch_bounds__(256) void k_vor_classify(VorField f) {
  __shared__ uint32_t s_cnt[4];
  const long long n = static_cast<long long>(f.nx) * f.ny * f.nz;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + static_cast<long long>(threadIdx.x);
  uint32_t in_range = 0u, eligible = 0u;
  int nb = 0;
  if (i < n) {
    const uint64_t key = f.keys[i];
    const int32_t v = static_cast<int32_t>(key >> 32);
    in_range = v <= f.rule.r2 ? 1u : 0u;
    // k_df_finish's expression: the correctly rounded float root through the double root
    const float dist = in_range ? f.rule.cell_size * static_cast<float>(sqrt(static_cast<double>(v))) : f.rule.max_distance;
    const bool has = vorHasSite(key, f.rule.r2);
    f.distance[i] = dist;
    f.d2[i] = in_range ? v : kDfFar;
    if (in_range) f.status[i] = static_cast<uint8_t>(f.status[i] | kDfInRange);
    f.site[i] = has ? static_cast<int32_t>(static_cast<uint32_t>(key)) : -1;
    if (has && dist >= f.rule.min_distance) {
      eligible = 1u;
      const int x = static_cast<int>(i % f.nx), y = static_cast<int>((i / f.nx) % f.ny), z = static_cast<int>(i / (static_cast<long long>(f.nx) * f.ny));
      int sx[kVorMaxBasis], sy[kVorMaxBasis], sz[kVorMaxBasis];
      nb = vorBasis(f, x, y, z, static_cast<uint32_t>(key), sx, sy, sz);
    }
    f.basis[i] = static_cast<uint8_t>(nb);
  }
  const bool listed = nb >= f.rule.min_basis;
  waveStatAdd(f.stats + DFS_IN_RANGE, in_range);
  waveStatAdd(f.stats + VS_ELIGIBLE, eligible);
  waveStatAdd(f.stats + VS_BASIS2, nb == 2 ? 1u : 0u);
  waveStatAdd(f.stats + VS_BASIS3, nb == 3 ? 1u : 0u);
  waveStatAdd(f.stats + VS_BASIS4, nb == 4 ? 1u : 0u);
  waveStatAdd(f.stats + VS_LISTED, listed ? 1u : 0u);
  const unsigned long long bal = __ballot(listed);
  if (laneId() == 0) s_cnt[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(bal));
  __syncthreads();
  if (threadIdx.x == 0) f.wg_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// the same grid as k_vor_classify; f.wg_count now holds the exclusive scan of the counts (one word more than workgroups)
__global__ __launch_bounds__(256) void k_vor_emit(VorField f) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t first = f.wg_count[blockIdx.x];
  if (f.wg_count[blockIdx.x + 1] == first) return;  // (uniform)
  const long long n = static_cast<long long>(f.nx) * f.ny * f.nz;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + static_cast<long long>(threadIdx.x);
  const uint32_t lane = laneId(), wave = threadIdx.x >> 6;
  const int nb_cell = i < n ? static_cast<int>(f.basis[i]) : 0;
  const bool listed = nb_cell >= f.rule.min_basis;
  const unsigned long long bal = __ballot(listed);
  if (lane == 0) s_cnt[wave] = static_cast<uint32_t>(__popcll(bal));
  __syncthreads();
  if (!listed) return;
  uint32_t pos = first + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)));
#pragma unroll
  for (uint32_t w = 0; w < 3; ++w)
    if (w < wave) pos += s_cnt[w];
  if (pos >= f.n_listed) return;  // (cannot happen while the keys are what k_vor_classify saw: no write beyond the arrays)
  const int x = static_cast<int>(i % f.nx), y = static_cast<int>((i / f.nx) % f.ny), z = static_cast<int>(i / (static_cast<long long>(f.nx) * f.ny));
  int sx[kVorMaxBasis], sy[kVorMaxBasis], sz[kVorMaxBasis];
  const int nb = vorBasis(f, x, y, z, static_cast<uint32_t>(f.keys[i]), sx, sy, sz);
  int32_t* const cell = f.cells + 3 * static_cast<size_t>(pos);
  cell[0] = f.ox + x, cell[1] = f.oy + y, cell[2] = f.oz + z;
  f.cell_distance[pos] = f.distance[i];
  f.cell_basis[pos] = static_cast<uint8_t>(nb);
  int32_t* const sites = f.cell_sites + 3 * kVorMaxBasis * static_cast<size_t>(pos);
#pragma unroll
  for (int j = 0; j < kVorMaxBasis; ++j) {
    const bool used = j < nb;
    sites[3 * j] = used ? f.ox + sx[j] : 0, sites[3 * j + 1] = used ? f.oy + sy[j] : 0, sites[3 * j + 2] = used ? f.oz + sz[j] : 0;
  }
}

}  // namespace khr
