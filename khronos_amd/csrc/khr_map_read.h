// khr_map_read.h — what the kernels that sample the live map share (khr_kernels_render.h, khr_kernels_query.h): the index guard of
// ASSUMPTIONS.md A.12, the key range of a block index, the trilinear combination and the per-wave 64-bit counter add.
#pragma once
#include "khr_device.h"

namespace khr {

constexpr float kMapIndexLimit = 1073741824.f;  // |p * voxel_size_inv - 0.5| at or beyond 2^30 (or NaN): no voxel there

// a block index the 21-bit-per-axis keys can hold (packKey would alias anything else onto another block)
__device__ inline bool blockInKeyRange(int bx, int by, int bz) {
  constexpr uint32_t R = 1u << 20;
  return static_cast<uint32_t>(bx) + R < 2u * R && static_cast<uint32_t>(by) + R < 2u * R && static_cast<uint32_t>(bz) + R < 2u * R;
}

// taps v[t] at corner offsets (t & 1, (t >> 1) & 1, t >> 2), fractions f: x first, then y, then z (A.12)
__device__ inline float trilinear(const float* v, const float* f) {
  const float c00 = v[0] + f[0] * (v[1] - v[0]), c10 = v[2] + f[0] * (v[3] - v[2]);
  const float c01 = v[4] + f[0] * (v[5] - v[4]), c11 = v[6] + f[0] * (v[7] - v[6]);
  const float c0 = c00 + f[1] * (c10 - c00), c1 = c01 + f[1] * (c11 - c01);
  return c0 + f[2] * (c1 - c0);
}

// one atomic per wave and counter: every lane of the wave calls it, the wave's total must stay below 2^32
__device__ inline void waveStatAdd(unsigned long long* counter, uint32_t lane_value) {
  uint32_t sum = lane_value;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
  if (laneId() == 0 && sum) atomicAdd(counter, static_cast<unsigned long long>(sum));
}

}  // namespace khr
