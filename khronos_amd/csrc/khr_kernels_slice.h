// khr_kernels_slice.h — one z-plane of the live map (ActiveWindowVisualizer's map slices, active_window_visualizer.cpp:345-520)
// read on the device: select the live blocks of the layer, sort them by (bx, by), gather the plane of each into SoA staging.
// No host round trip between the map and the staging (khr_map_slice).
#pragma once
#include "khr_device.h"

namespace khr {

// Sort keys: biased bx (21 bits) | biased by (21 bits) | pool slot (22 bits).  (bx, by) is unique on a layer, so the order is
// the (bx, by) order and the slot rides along.  khr_map_slice refuses pools of more than 2^22 blocks.
constexpr int kSliceSlotBits = 22;
constexpr uint32_t kSliceSlotMask = (1u << kSliceSlotBits) - 1u;
constexpr uint32_t kSliceSortTile = 4096;  // keys of the one-workgroup LDS sort (32 KiB); longer lists take the multi-pass path
constexpr int kSliceSortThreads = 1024;

__host__ __device__ inline uint32_t slicePadded(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}
__device__ inline uint64_t sliceKey(int bx, int by, uint32_t slot) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(bx + (1 << 20)) & 0x1fffffu) << 43) |
         (static_cast<uint64_t>(static_cast<uint32_t>(by + (1 << 20)) & 0x1fffffu) << kSliceSlotBits) | slot;
}

// live slots whose block index z is bz -> keys[count++].  Grid-stride over the pool's high-water mark as the device has it.
__global__ __launch_bounds__(256) void k_slice_select(DevMap m, int bz, uint32_t* __restrict__ count, uint64_t* __restrict__ keys) {
  const uint32_t n_slots = m.counters[C_MAX_SLOT];
  for (uint32_t base = blockIdx.x * blockDim.x; base < n_slots; base += gridDim.x * blockDim.x) {  // (uniform per workgroup)
    const uint32_t s = base + threadIdx.x;
    bool take = false;
    int4 bi = make_int4(0, 0, 0, 0);
    if (s < n_slots && (m.blk_flags[s] & BLK_LIVE)) {
      bi = m.blk_index[s];
      take = bi.z == bz;
    }
    const uint32_t pos = waveAggInc(count, take);
    if (take) keys[pos] = sliceKey(bi.x, bi.y, s);
  }
}

// Bitonic sort of keys[0, P), P = the count rounded up to a power of two, ascending.  The network's direction at stage k is
// ascending where (i & k) == 0, i the global position.
// k_merge == 0: each workgroup sorts one tile of min(P, kSliceSortTile) keys in LDS (positions >= count read as ~0, and the
//   tile is written back whole, so the padding exists in memory from here on).  For P <= kSliceSortTile this is the whole sort.
// k_merge > kSliceSortTile: the steps j = kSliceSortTile / 2 .. 1 of stage k_merge, one tile per workgroup; the steps with
//   j >= kSliceSortTile cross tiles and are k_slice_sort_step's.  Stages beyond P exit at once (the host launches for the
//   largest P the pool allows and does not know the count).
__global__ __launch_bounds__(kSliceSortThreads) void k_slice_sort_tile(uint64_t* __restrict__ keys, const uint32_t* __restrict__ count,
                                                                   uint32_t k_merge) {
  __shared__ uint64_t s[kSliceSortTile];
  const uint32_t n = *count, P = slicePadded(n);
  const uint32_t T = P < kSliceSortTile ? P : kSliceSortTile;
  const uint32_t base = blockIdx.x * kSliceSortTile;
  if (base >= P || k_merge > P) return;
  for (uint32_t i = threadIdx.x; i < T; i += kSliceSortThreads) s[i] = (k_merge || base + i < n) ? keys[base + i] : ~0ull;
  __syncthreads();
  const uint32_t k_lo = k_merge ? k_merge : 2u, k_hi = k_merge ? k_merge : T;
  for (uint32_t k = k_lo; k <= k_hi; k <<= 1)
    for (uint32_t j = (k_merge ? T : k) >> 1; j > 0; j >>= 1) {
      for (uint32_t t = threadIdx.x; t < T / 2; t += kSliceSortThreads) {
        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i + j;
        const bool up = ((base + i) & k) == 0u;
        const uint64_t a = s[i], b = s[l];
        if ((a > b) == up) {
          s[i] = b;
          s[l] = a;
        }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < T; i += kSliceSortThreads) keys[base + i] = s[i];
}

// one cross-tile step (j >= kSliceSortTile) of stage k in global memory
__global__ __launch_bounds__(256) void k_slice_sort_step(uint64_t* __restrict__ keys, const uint32_t* __restrict__ count, uint32_t k,
                                                       uint32_t j) {
  const uint32_t P = slicePadded(*count);
  if (k > P) return;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < P / 2; t += gridDim.x * blockDim.x) {
    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i + j;
    const bool up = (i & k) == 0u;
    const uint64_t a = keys[i], b = keys[l];
    if ((a > b) == up) {
      keys[i] = b;
      keys[l] = a;
    }
  }
}

// SoA staging of a slice; a NULL field is not gathered.  Nothing is written when the count exceeds cap_blocks (the host grows
// the staging and gathers again).
struct SliceOut {
  int32_t* block_xy;  // [block][2]
  float* pos;         // [voxel][3]
  float* dist;
  float* weight;
  uint64_t* last_obs;
  uint8_t* vflags;
  uint32_t cap_blocks;
};

// One workgroup of VPS^2 threads per block of the sorted list.  Output position of a voxel = rank * VPS^2 + x * VPS + y (the
// visualizer's x-outer / y-inner loops, :377-378), the transpose of the memory order x + VPS * y: the plane is read in memory
// order, staged through LDS (rows padded by one against bank conflicts) and written in output order, both coalesced.
template <int VPS>
__global__ __launch_bounds__(VPS * VPS) void k_slice_gather(DevMap m, DevParams p, const uint64_t* __restrict__ keys,
                                                           const uint32_t* __restrict__ count, int bz, int lz, SliceOut o) {
  constexpr int NV = VPS * VPS * VPS, NP = VPS * VPS, LD = VPS + 1;
  __shared__ float s_d[VPS * LD], s_w[VPS * LD];
  __shared__ uint64_t s_t[VPS * LD];
  __shared__ uint8_t s_f[VPS * LD];
  const uint32_t n = *count;
  if (n > o.cap_blocks) return;
  const int t = static_cast<int>(threadIdx.x);
  const int mx = t % VPS, my = t / VPS;  // memory order of the plane
  const int src_l = mx * LD + my, dst_l = (t / VPS) * LD + t % VPS;
  const uint32_t lin = static_cast<uint32_t>(mx + VPS * (my + VPS * lz));
  for (uint32_t b = blockIdx.x; b < n; b += gridDim.x) {
    const uint64_t key = keys[b];
    const uint32_t slot = static_cast<uint32_t>(key) & kSliceSlotMask;
    const int bx = static_cast<int>((key >> 43) & 0x1fffffu) - (1 << 20), by = static_cast<int>((key >> kSliceSlotBits) & 0x1fffffu) - (1 << 20);
    const size_t v = static_cast<size_t>(slot) * NV + lin;
    if (o.dist) s_d[src_l] = m.dist[v];
    if (o.weight) s_w[src_l] = m.weight[v];
    if (o.last_obs) s_t[src_l] = p.with_tracking ? lastObserved(m, slot, lin, NV) : 0ull;
    if (o.vflags) s_f[src_l] = m.vflags[v] & VOX_PUBLIC_MASK;
    __syncthreads();
    const size_t dst = static_cast<size_t>(b) * NP + static_cast<size_t>(t);
    if (o.dist) o.dist[dst] = s_d[dst_l];
    if (o.weight) o.weight[dst] = s_w[dst_l];
    if (o.last_obs) o.last_obs[dst] = s_t[dst_l];
    if (o.vflags) o.vflags[dst] = s_f[dst_l];
    if (o.pos) {  // voxel centre (ASSUMPTIONS.md A.1): float(b) * block_size + (float(i) + 0.5) * voxel_size; 3 floats per voxel
      const float oz = static_cast<float>(bz) * p.bs + (static_cast<float>(lz) + 0.5f) * p.vs;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int e = t + c * NP, vox = e / 3, comp = e - 3 * vox;
        float val = oz;
        if (comp == 0) val = static_cast<float>(bx) * p.bs + (static_cast<float>(vox / VPS) + 0.5f) * p.vs;
        if (comp == 1) val = static_cast<float>(by) * p.bs + (static_cast<float>(vox % VPS) + 0.5f) * p.vs;
        o.pos[static_cast<size_t>(b) * NP * 3 + static_cast<size_t>(e)] = val;
      }
    }
    if (o.block_xy && t < 2) o.block_xy[2 * static_cast<size_t>(b) + t] = t ? by : bx;
    __syncthreads();  // (the next block's plane reuses the LDS)
  }
}

}  // namespace khr
