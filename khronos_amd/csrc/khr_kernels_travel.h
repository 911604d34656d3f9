// khr_kernels_travel.h — clearance-bounded travel cost, nearest goal by travel and paths in a box of cells (khr_travel_field /
// khr_travel_field_from / khr_travel_paths; ASSUMPTIONS.md A.22).  Reads a distance / status field and a list of goal cells, writes
// buffers of its own.  gfx950, wave64.  Integers throughout, apart from the one float compare of the traversable test.
//
// The state is one 64-bit key per cell, cost << 32 | goal, kTfFarKey for "not reached"; the result is the unique fixed point of
// key(c) = min(key(c), key(n) + (w << 32)) over the allowed moves, so it does not depend on the order in which cells are relaxed.
//   k_tf_seed         one lane per cell: the traversable mask and its count; one lane per goal: atomic min of (0, g) on the goal's
//                     key (the keys are preset to kTfFarKey), the flag of its tile for round 0
//   k_tf_relax<CONN>  one workgroup per TILE of 8^3 cells, one launch per ROUND.  A workgroup whose flag for this round is clear
//                     leaves at once.  The others load the tile's keys with a one-cell halo (10^3 keys = 8000 bytes of LDS: LDS does
//                     not limit the workgroups of a CU) and relax inside LDS, two cells per lane, in sweeps of "read the neighbours,
//                     barrier, write" until a sweep changes nothing: at most kTfTileCells sweeps, since a key that changes in sweep
//                     k ends a path of k cells inside the tile.  Then they write back the interior keys that fell and raise the
//                     flags, for the NEXT round, of the neighbour tiles a fallen boundary cell touches, and the round's "someone
//                     goes on" word.  A tile has one writer; a halo key may be read while the neighbour's workgroup replaces it
//                     (relaxed 64-bit atomics: never torn) and be a round old -- keys only fall and the flag runs the reader again.
//                     No workgroup waits for another inside a launch.
//   (host: kTfRoundsPerWait rounds are queued, then the words of those rounds are read; until the last one is clear, or the cap of
//    n + kTfRoundsPerWait rounds -- a shortest path crosses fewer than n tile faces -- ends the call with an error)
//   k_tf_finish<CONN> one lane per cell: cost, goal, the parent code, the reached count and the greatest cost
//   k_tf_path_count / hipcub scan / k_tf_path_emit   one lane per start cell walks the parent codes to the goal: lengths, offsets,
//                     cells.  A walk ends after n steps whatever the codes say.
#pragma once
#include "khr_device.h"
#include "khr_map_read.h"

namespace khr {

constexpr uint64_t kTfFarKey = ~0ull;        // cost KHR_TF_UNREACHED, goal -1
constexpr uint32_t kTfUnreached = 0xFFFFFFFFu;
constexpr int kTfEdge = 8;                   // cells along a tile's axis
constexpr int kTfTileCells = kTfEdge * kTfEdge * kTfEdge;
constexpr int kTfHalo = kTfEdge + 2;
constexpr int kTfHaloCells = kTfHalo * kTfHalo * kTfHalo;
constexpr int kTfRoundsPerWait = 8;          // KHR_TF_ROUNDS_PER_WAIT
constexpr uint8_t kTfParentSelf = 13, kTfParentNone = 255;
constexpr uint8_t kTfObserved = 1, kTfObstacle = 2;  // KHR_DF_OBSERVED, KHR_DF_OBSTACLE

enum TfCounter : int { TFC_TRAVERSABLE = 0, TFC_GOALS_USED, TFC_REACHED, TFC_MAX_COST, TFC_COUNT };

struct TfField {
  int ox, oy, oz;  // first cell
  int nx, ny, nz;
  int ntx, nty, ntz;  // tiles per axis
  const float* distance;  // the input field, x + nx * (y + ny * z)
  const uint8_t* status;
  float clearance;
  int allow_unknown;
  uint32_t max_cost;      // 0: no limit
  const int32_t* goals;   // 3 per goal, global cells
  uint32_t n_goals;
  uint8_t* mask;          // [n] 1 = traversable
  unsigned long long* keys;  // [n] preset to kTfFarKey
  uint8_t* flags;         // [2][tiles] a tile runs in round r iff flags[r & 1][tile]; preset 0
  uint32_t* go_on;        // [kTfRoundsPerWait] word j: round j of the batch raised a flag; cleared before every batch
  unsigned long long* ctr;  // TfCounter words
  // the result (k_tf_finish)
  uint32_t* cost;
  int32_t* goal;
  uint8_t* parent;
};

__device__ inline bool tfTraversable(const TfField& f, size_t lin) {
  const uint8_t s = f.status[lin];
  const bool cls = (s & kTfObserved) ? !(s & kTfObstacle) : f.allow_unknown != 0;
  return cls && f.distance[lin] >= f.clearance;  // (false for a NaN)
}
__device__ inline size_t tfLin(const TfField& f, int x, int y, int z) {
  return static_cast<size_t>(x) + static_cast<size_t>(f.nx) * (static_cast<size_t>(y) + static_cast<size_t>(f.ny) * static_cast<size_t>(z));
}
__device__ inline unsigned long long tfLoadKey(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void tfStoreKey(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// is the move (dx, dy, dz) one of the connectivity's, and what does it cost
template <int CONN>
__host__ __device__ constexpr bool tfMove(int dx, int dy, int dz) {
  const int nz = (dx != 0) + (dy != 0) + (dz != 0);
  return nz != 0 && (CONN == 26 || (CONN == 18 && nz <= 2) || nz == 1);
}
__host__ __device__ constexpr uint32_t tfWeight(int dx, int dy, int dz) {
  const int nz = (dx != 0) + (dy != 0) + (dz != 0);
  return nz == 1 ? 10u : nz == 2 ? 14u : 17u;
}

// grid: enough lanes for the cells and for the goals
__global__ __launch_bounds__(256) void k_tf_seed(TfField f) {
  const size_t n = static_cast<size_t>(f.nx) * f.ny * f.nz;
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  uint32_t trav = 0u, used = 0u;
  if (i < n) {
    trav = tfTraversable(f, i) ? 1u : 0u;
    f.mask[i] = static_cast<uint8_t>(trav);
  }
  if (i < f.n_goals) {
    const long long gx = static_cast<long long>(f.goals[3 * i]) - f.ox, gy = static_cast<long long>(f.goals[3 * i + 1]) - f.oy,
                    gz = static_cast<long long>(f.goals[3 * i + 2]) - f.oz;
    if (gx >= 0 && gx < f.nx && gy >= 0 && gy < f.ny && gz >= 0 && gz < f.nz) {
      const int x = static_cast<int>(gx), y = static_cast<int>(gy), z = static_cast<int>(gz);
      const size_t lin = tfLin(f, x, y, z);
      if (tfTraversable(f, lin)) {
        used = 1u;
        atomicMin(f.keys + lin, static_cast<unsigned long long>(i));  // cost 0; the least index among the goals of a cell
        f.flags[(x / kTfEdge) + f.ntx * ((y / kTfEdge) + f.nty * (z / kTfEdge))] = 1;
      }
    }
  }
  waveStatAdd(f.ctr + TFC_TRAVERSABLE, trav);
  waveStatAdd(f.ctr + TFC_GOALS_USED, used);
}

// grid: one workgroup per tile; `round` counts from 0 over the whole call, `slot` inside the batch
template <int CONN>
__global__ __launch_bounds__(256) void k_tf_relax(TfField f, uint32_t round, uint32_t slot) {
  __shared__ unsigned long long s_key[kTfHaloCells];
  __shared__ uint32_t s_dirs;
  const int tid = static_cast<int>(threadIdx.x);
  const int t = static_cast<int>(blockIdx.x);
  const int n_tiles = f.ntx * f.nty * f.ntz;
  uint8_t* const mine = f.flags + static_cast<size_t>(round & 1u) * n_tiles;
  uint8_t* const next = f.flags + static_cast<size_t>((round + 1u) & 1u) * n_tiles;
  if (mine[t] == 0) return;  // (uniform: nobody writes this round's flags during the round)
  const int tx = t % f.ntx, ty = (t / f.ntx) % f.nty, tz = t / (f.ntx * f.nty);
  const int bx = tx * kTfEdge, by = ty * kTfEdge, bz = tz * kTfEdge;
  if (tid == 0) s_dirs = 0u;
  for (int l = tid; l < kTfHaloCells; l += 256) {
    const int x = bx + l % kTfHalo - 1, y = by + (l / kTfHalo) % kTfHalo - 1, z = bz + l / (kTfHalo * kTfHalo) - 1;
    const bool in = x >= 0 && x < f.nx && y >= 0 && y < f.ny && z >= 0 && z < f.nz;
    s_key[l] = in ? tfLoadKey(f.keys + tfLin(f, x, y, z)) : kTfFarKey;  // (a cell that is not traversable keeps kTfFarKey for good)
  }
  // this lane's two cells: c = tid and tid + 256
  int at[2];
  size_t lin[2];
  bool live[2];
  unsigned long long first[2], cur[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int c = tid + 256 * k;
    const int lx = c % kTfEdge, ly = (c / kTfEdge) % kTfEdge, lz = c / (kTfEdge * kTfEdge);
    at[k] = (lx + 1) + kTfHalo * ((ly + 1) + kTfHalo * (lz + 1));
    const int x = bx + lx, y = by + ly, z = bz + lz;
    live[k] = x < f.nx && y < f.ny && z < f.nz;
    lin[k] = live[k] ? tfLin(f, x, y, z) : 0;
    if (live[k]) live[k] = f.mask[lin[k]] != 0;
  }
  __syncthreads();
  if (tid == 0) mine[t] = 0;  // (read above by every lane; the flag is raised again two rounds on at the earliest)
#pragma unroll
  for (int k = 0; k < 2; ++k) first[k] = cur[k] = s_key[at[k]];
  const unsigned long long limit = f.max_cost ? static_cast<unsigned long long>(f.max_cost) : static_cast<unsigned long long>(kTfUnreached - 1u);
  bool settled = false;
#pragma unroll 1
  for (int sweep = 0; sweep < kTfTileCells + 1; ++sweep) {
    unsigned long long best[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      best[k] = cur[k];
      if (live[k]) {
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
              if (tfMove<CONN>(dx, dy, dz)) {
                const unsigned long long nk = s_key[at[k] + dx + kTfHalo * (dy + kTfHalo * dz)];
                // (cost < 17 * 2^24 for every reached cell, so the sum does not carry out of the cost)
                const unsigned long long cand = nk + (static_cast<unsigned long long>(tfWeight(dx, dy, dz)) << 32);
                if (nk != kTfFarKey && (cand >> 32) <= limit && cand < best[k]) best[k] = cand;
              }
      }
    }
    __syncthreads();
    const bool fell = best[0] < cur[0] || best[1] < cur[1];
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (best[k] < cur[k]) s_key[at[k]] = cur[k] = best[k];
    if (!__syncthreads_or(fell ? 1 : 0)) {
      settled = true;
      break;
    }
  }
  // write back what fell; which neighbour tiles see it: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
  uint32_t dirs = 0u;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (!(cur[k] < first[k])) continue;
    tfStoreKey(f.keys + lin[k], cur[k]);
    const int c = tid + 256 * k;
    const int lx = c % kTfEdge, ly = (c / kTfEdge) % kTfEdge, lz = c / (kTfEdge * kTfEdge);
    const uint32_t mx = 2u | (lx == 0 ? 1u : 0u) | (lx == kTfEdge - 1 ? 4u : 0u);
    const uint32_t my = 2u | (ly == 0 ? 1u : 0u) | (ly == kTfEdge - 1 ? 4u : 0u);
    const uint32_t mz = 2u | (lz == 0 ? 1u : 0u) | (lz == kTfEdge - 1 ? 4u : 0u);
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (((mz >> (j / 3)) & 1u) && ((my >> (j % 3)) & 1u)) dirs |= mx << (3 * j);
  }
  // bit 13 is the tile itself: it runs again only if it ran out of sweeps (it cannot), instead of stopping short
  dirs = settled ? dirs & ~(1u << 13) : dirs | (1u << 13);
  if (dirs) atomicOr(&s_dirs, dirs);
  __syncthreads();
  const uint32_t all = s_dirs;
  if (tid < 27 && ((all >> tid) & 1u)) {
    const int dx = tid % 3 - 1, dy = (tid / 3) % 3 - 1, dz = tid / 9 - 1;
    const int qx = tx + dx, qy = ty + dy, qz = tz + dz;
    const bool moves = tid == 13 || tfMove<CONN>(dx, dy, dz);  // (a tile across a corner is only reached by a space diagonal)
    if (moves && qx >= 0 && qx < f.ntx && qy >= 0 && qy < f.nty && qz >= 0 && qz < f.ntz) {
      next[qx + f.ntx * (qy + f.nty * qz)] = 1;
      f.go_on[slot] = 1u;
    }
  }
}

// one lane per cell
template <int CONN>
__global__ __launch_bounds__(256) void k_tf_finish(TfField f) {
  const size_t n = static_cast<size_t>(f.nx) * f.ny * f.nz;
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  uint32_t reached = 0u, cost = 0u;
  if (i < n) {
    const unsigned long long key = f.keys[i];
    uint8_t parent = kTfParentNone;
    if (key != kTfFarKey) {
      reached = 1u;
      cost = static_cast<uint32_t>(key >> 32);
      if (cost == 0u) {
        parent = kTfParentSelf;
      } else {
        const int x = static_cast<int>(i % f.nx), y = static_cast<int>((i / f.nx) % f.ny), z = static_cast<int>(i / (static_cast<size_t>(f.nx) * f.ny));
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
              if (tfMove<CONN>(dx, dy, dz)) {
                const int X = x + dx, Y = y + dy, Z = z + dz;
                if (parent == kTfParentNone && X >= 0 && X < f.nx && Y >= 0 && Y < f.ny && Z >= 0 && Z < f.nz) {
                  const unsigned long long nk = f.keys[tfLin(f, X, Y, Z)];
                  if (nk != kTfFarKey && nk + (static_cast<unsigned long long>(tfWeight(dx, dy, dz)) << 32) == key)
                    parent = static_cast<uint8_t>((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
                }
              }
      }
    }
    f.cost[i] = reached ? cost : kTfUnreached;
    f.goal[i] = reached ? static_cast<int32_t>(static_cast<uint32_t>(key)) : -1;
    f.parent[i] = parent;
  }
  waveStatAdd(f.ctr + TFC_REACHED, reached);
  uint32_t top = cost;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = __shfl_down(top, o);
    top = other > top ? other : top;
  }
  if (laneId() == 0 && top) atomicMax(f.ctr + TFC_MAX_COST, static_cast<unsigned long long>(top));
}

// the launches of the two templates, by connectivity (6, 18, 26: the host checks)
template <int CONN>
inline void tfLaunchRelax(const TfField& f, unsigned tiles, uint32_t round, uint32_t slot, hipStream_t st) {
  hipLaunchKernelGGL((k_tf_relax<CONN>), dim3(tiles), dim3(256), 0, st, f, round, slot);
}
template <int CONN>
inline void tfLaunchFinish(const TfField& f, size_t n, hipStream_t st) {
  hipLaunchKernelGGL((k_tf_finish<CONN>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, st, f);
}

struct TfPaths {
  int ox, oy, oz;
  int nx, ny, nz;
  const uint32_t* cost;   // the travel result
  const int32_t* goal;
  const uint8_t* parent;
  const int32_t* starts;  // 3 per start, global cells
  uint32_t n_starts;
  long long* offsets;     // [n_starts + 1] lengths, scanned in place
  uint32_t* path_cost;
  int32_t* path_goal;
  int32_t* cells;         // 3 per path cell (k_tf_path_emit)
  long long n_cells_total;
};

// the cells of the walk from box-local (x, y, z) to its goal, 0 where the walk does not end on a goal within n steps; with
// `out` the cells are written too, at most `room` of them
__device__ inline long long tfWalk(const TfPaths& p, int x, int y, int z, int32_t* out, long long room) {
  const long long n = static_cast<long long>(p.nx) * p.ny * p.nz;
  long long len = 0;
#pragma unroll 1
  for (long long step = 0; step < n; ++step) {
    const uint8_t code = p.parent[static_cast<size_t>(x) + static_cast<size_t>(p.nx) * (static_cast<size_t>(y) + static_cast<size_t>(p.ny) * static_cast<size_t>(z))];
    if (code > 26) return 0;
    if (out && len < room) out[3 * len] = p.ox + x, out[3 * len + 1] = p.oy + y, out[3 * len + 2] = p.oz + z;
    ++len;
    if (code == kTfParentSelf) return len;
    x += code % 3 - 1, y += (code / 3) % 3 - 1, z += code / 9 - 1;
    if (x < 0 || x >= p.nx || y < 0 || y >= p.ny || z < 0 || z >= p.nz) return 0;
  }
  return 0;
}

// one lane per start; lane n_starts clears the last word of the lengths
__global__ __launch_bounds__(256) void k_tf_path_count(TfPaths p) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == p.n_starts) p.offsets[i] = 0;
  if (i >= p.n_starts) return;
  const long long sx = static_cast<long long>(p.starts[3 * i]) - p.ox, sy = static_cast<long long>(p.starts[3 * i + 1]) - p.oy,
                  sz = static_cast<long long>(p.starts[3 * i + 2]) - p.oz;
  long long len = 0;
  size_t lin = 0;
  if (sx >= 0 && sx < p.nx && sy >= 0 && sy < p.ny && sz >= 0 && sz < p.nz) {
    const int x = static_cast<int>(sx), y = static_cast<int>(sy), z = static_cast<int>(sz);
    lin = static_cast<size_t>(x) + static_cast<size_t>(p.nx) * (static_cast<size_t>(y) + static_cast<size_t>(p.ny) * static_cast<size_t>(z));
    len = tfWalk(p, x, y, z, nullptr, 0);
  }
  p.offsets[i] = len;
  p.path_cost[i] = len ? p.cost[lin] : kTfUnreached;
  p.path_goal[i] = len ? p.goal[lin] : -1;
}

// one lane per start; p.offsets now holds the exclusive scan of the lengths
__global__ __launch_bounds__(256) void k_tf_path_emit(TfPaths p) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n_starts) return;
  const long long at = p.offsets[i], len = p.offsets[i + 1] - at;
  if (len <= 0 || at < 0 || at + len > p.n_cells_total) return;  // (no write beyond the list, whatever the offsets say)
  tfWalk(p, p.starts[3 * i] - p.ox, p.starts[3 * i + 1] - p.oy, p.starts[3 * i + 2] - p.oz, p.cells + 3 * at, len);
}

}  // namespace khr
