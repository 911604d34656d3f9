// khr_kernels_diff.h — device side of khr_diff_map (include/khronos_amd.h; ASSUMPTIONS.md A.18): the voxels that appeared or
// vanished in the live map (`now`) against another context's map (`then`), sampled as khr_merge_map samples a source (A.17:
// mergeLocate, ALIGNED or RESAMPLE).  Both maps are only read.  gfx950, wave64.
//   k_merge_candidates  (khr_kernels_merge.h, `then` as the source) every live block of `then` -> the blocks of `now` it can reach
//   k_diff_count        one workgroup per candidate: absent from `now` -> done; the five voxel counts, the block's two counts, and
//                       the changed blocks as a compact list of {(x, y, z)-ordered key, candidate}
//   (the host's one wait: the counts size the result, the sort, the scan and the emit)
//   hipcub radix sort   the changed blocks into (x, y, z) order
//   k_diff_block_counts per sorted block its number of changed voxels; an exclusive scan of it is the block's `first`
//   k_diff_emit         one workgroup per changed block: the block record and its voxel records in ascending linear index
// Like the merge's probe, the count keeps no per-wave ballots (they would be sized by what the pool of `then` can reach): the emit
// classifies the block's voxels again, the same function on the same unchanged maps, and only the changed lanes then evaluate the
// sample a third time for the values they write.
#pragma once
#include "khr_device.h"
#include "khr_kernels_merge.h"
#include "khr_map_read.h"

namespace khr {

// counters of one diff: the first words are k_merge_candidates' (MC_SRC, MC_LIST, MC_CAND, MC_ERR keep their places)
enum DiffCounter : int {
  DC_PRESENT = 3,  // candidates that are live in `now`
  DC_CHANGED = 4,  // ... of them with a kind-1 or kind-2 voxel (the length of the changed list)
  DC_COUNT = 8     // (five 64-bit words follow: DiffVoxelCounter)
};
enum DiffVoxelCounter : int { DV_COMPARED = 0, DV_APPEARED, DV_DISAPPEARED, DV_ONLY_NOW, DV_ONLY_THEN, DV_COUNT };
constexpr int kDiffCounterWords = DC_COUNT + 2 * DV_COUNT;
static_assert(DC_PRESENT != MC_SRC && DC_PRESENT != MC_LIST && DC_PRESENT != MC_CAND && DC_PRESENT != MC_ERR && DC_CHANGED != MC_ERR &&
                  MC_ERR < DC_COUNT,
              "the diff's counters sit beside the candidate kernel's");
constexpr uint8_t kDiffAppeared = 1, kDiffDisappeared = 2;  // `kind`

struct DiffArgs {
  float occupied_distance, free_distance;
};

// Per-candidate words and the changed list (one block of the context's merge scratch: five arrays of `cap` entries, the keys
// last), the sorted list and its scan.  One base pointer, not five: the kernels hold the base pointers of two maps besides.
struct DiffWork {
  uint32_t* words;
  uint32_t cap;
  uint64_t* sorted_key;   // the changed list in (x, y, z) order
  uint32_t* sorted_cand;
  uint32_t* blk_count;    // [n_blocks + 1] changed voxels per sorted block
  uint32_t* blk_first;    // [n_blocks + 1] exclusive scan of blk_count
  uint32_t n_blocks;      // changed blocks (host: after the wait)
  uint32_t n_voxels;      // changed voxels = the length of the voxel arrays
};
constexpr int kDiffWordsPerCandidate = 6;
__host__ __device__ inline uint32_t* diffCandSlot(const DiffWork& W) { return W.words; }  // slot of a present candidate in `now`
__host__ __device__ inline uint32_t* diffCandAppeared(const DiffWork& W) { return W.words + W.cap; }  // its kind-1 / kind-2 voxels
__host__ __device__ inline uint32_t* diffCandDisappeared(const DiffWork& W) { return W.words + 2 * static_cast<size_t>(W.cap); }
// the changed list, in the order the workgroups arrived: the candidate, and the block index with x most significant
__host__ __device__ inline uint32_t* diffChangedCand(const DiffWork& W) { return W.words + 3 * static_cast<size_t>(W.cap); }
__host__ __device__ inline uint64_t* diffChangedKey(const DiffWork& W) {  // (8-byte aligned: the block is, 16 * cap bytes lie in front)
  return reinterpret_cast<uint64_t*>(W.words + 4 * static_cast<size_t>(W.cap));
}

// The result, structure of arrays in one block: the byte offset of each array for n changed voxels in m changed blocks (256-byte
// aligned).  The emit kernel takes the block's base and forms the offsets itself, in place of eleven pointers.
struct DiffLayout {
  size_t voxels, kind, d_now, d_then, label, stamp_now, stamp_then, blocks, block_appeared, block_disappeared, block_first, bytes;
};
__host__ __device__ inline DiffLayout diffLayout(size_t n, size_t m) {
  DiffLayout L;
  size_t o = 0;
  const auto carve = [&o](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) & ~static_cast<size_t>(255);
    return at;
  };
  L.voxels = carve(12 * n), L.kind = carve(n), L.d_now = carve(4 * n), L.d_then = carve(4 * n), L.label = carve(4 * n);
  L.stamp_now = carve(8 * n), L.stamp_then = carve(8 * n), L.blocks = carve(12 * m), L.block_appeared = carve(4 * m);
  L.block_disappeared = carve(4 * m), L.block_first = carve(4 * m), L.bytes = o;
  return L;
}

// (x, y, z) order as one integer: the biased 21-bit fields of packKey with x most significant
__device__ inline uint64_t diffOrderKey(int x, int y, int z) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(x + (1 << 20)) & 0x1fffffu) << 42) |
         (static_cast<uint64_t>(static_cast<uint32_t>(y + (1 << 20)) & 0x1fffffu) << 21) |
         static_cast<uint64_t>(static_cast<uint32_t>(z + (1 << 20)) & 0x1fffffu);
}

// A.18's classes of one voxel: N = observed in `now`, T = the sample of `then` is valid
struct DiffClass {
  bool compared, appeared, disappeared, only_now, only_then;
};
__device__ inline DiffClass diffClassify(bool N, bool T, float d_now, float d_then, const DiffArgs& D) {
  DiffClass k;
  k.compared = N && T;
  k.appeared = k.compared && d_then >= D.free_distance && d_now <= D.occupied_distance;
  k.disappeared = k.compared && d_then <= D.occupied_distance && d_now >= D.free_distance;
  k.only_now = N && !T;
  k.only_then = !N && T;
  return k;
}

// One workgroup per candidate, one wave per 64 voxels.  Writes scratch only.  The voxel counts are popcounts of wave ballots
// (wave-uniform), summed over the block's four waves through LDS: one non-returning atomic per non-zero counter and workgroup.
template <int VPS, int MODE>
__global__ __launch_bounds__(256) void k_diff_count(DevMap now, DevMap then, DevParams p, MergeArgs X, DiffArgs D, MergeScratch S, DiffWork W) {
  constexpr int NV = VPS * VPS * VPS, NG = NV / 64;
  __shared__ float s_M[16];
  __shared__ uint32_t s_cnt[4][DV_COUNT];
  mergeStageTransform<MODE>(p, X, s_M);
  const uint32_t n = min(S.ctr[MC_LIST], S.cap);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long* const ctr64 = reinterpret_cast<unsigned long long*>(S.ctr + DC_COUNT);
  for (uint32_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const int4 c = S.cand[ci];
    if (c.w != 0) continue;  // outside the key range: not a block of `now` (uniform)
    const uint32_t slot = htLookup(now, packKey(c.x, c.y, c.z));
    if (slot == kInvalidSlot) continue;  // a candidate `now` lacks takes no part (uniform)
    const size_t o = static_cast<size_t>(slot) * NV;
    uint32_t cnt[DV_COUNT] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t g = wave; g < static_cast<uint32_t>(NG); g += 4) {
      const uint32_t lin = 64u * g + lane;
      float d_then;
      uint32_t ss, sl;
      const bool T = mergeLocate<VPS, MODE>(then, p, X, s_M, c.x, c.y, c.z, lin, &d_then, &ss, &sl);
      const bool N = now.weight[o + lin] >= X.min_weight;
      const DiffClass k = diffClassify(N, T, now.dist[o + lin], d_then, D);
      cnt[DV_COMPARED] += static_cast<uint32_t>(__popcll(__ballot(k.compared)));
      cnt[DV_APPEARED] += static_cast<uint32_t>(__popcll(__ballot(k.appeared)));
      cnt[DV_DISAPPEARED] += static_cast<uint32_t>(__popcll(__ballot(k.disappeared)));
      cnt[DV_ONLY_NOW] += static_cast<uint32_t>(__popcll(__ballot(k.only_now)));
      cnt[DV_ONLY_THEN] += static_cast<uint32_t>(__popcll(__ballot(k.only_then)));
    }
    __syncthreads();  // (the previous candidate's sums have been read)
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < DV_COUNT; ++i) s_cnt[wave][i] = cnt[i];
    }
    __syncthreads();
    if (threadIdx.x < static_cast<uint32_t>(DV_COUNT)) {
      const uint32_t sum = (s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x]) + (s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x]);
      if (sum) atomicAdd(&ctr64[threadIdx.x], static_cast<unsigned long long>(sum));
    }
    if (threadIdx.x == 64) atomicAdd(&S.ctr[DC_PRESENT], 1u);
    if (threadIdx.x == 128) {
      const uint32_t n_app = (s_cnt[0][DV_APPEARED] + s_cnt[1][DV_APPEARED]) + (s_cnt[2][DV_APPEARED] + s_cnt[3][DV_APPEARED]);
      const uint32_t n_dis = (s_cnt[0][DV_DISAPPEARED] + s_cnt[1][DV_DISAPPEARED]) + (s_cnt[2][DV_DISAPPEARED] + s_cnt[3][DV_DISAPPEARED]);
      diffCandSlot(W)[ci] = slot;
      diffCandAppeared(W)[ci] = n_app;
      diffCandDisappeared(W)[ci] = n_dis;
      if (n_app + n_dis != 0u) {  // (the one returning atomic, per changed block; ci < cap and every candidate is unique: pos < cap)
        const uint32_t pos = atomicAdd(&S.ctr[DC_CHANGED], 1u);
        if (pos < S.cap) {
          diffChangedKey(W)[pos] = diffOrderKey(c.x, c.y, c.z);
          diffChangedCand(W)[pos] = ci;
        }
      }
    }
  }
}

// per sorted block the number of its changed voxels, and a closing zero for the scan
__global__ __launch_bounds__(256) void k_diff_block_counts(DiffWork W) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > W.n_blocks) return;
  uint32_t v = 0u;
  if (i < W.n_blocks) {
    const uint32_t ci = min(W.sorted_cand[i], W.cap - 1u);
    v = diffCandAppeared(W)[ci] + diffCandDisappeared(W)[ci];
  }
  W.blk_count[i] = v;
}

// One workgroup per changed block in sorted order.  The order inside the block: every wave leaves the changed-lane ballot of each
// of its 64-voxel groups in LDS; after one barrier the first wave turns the groups' popcounts into bases; a lane's position is the
// block's first + its group's base + the changed lanes below it.  The loops stay rolled: unrolled, the sixteen groups of a wave at
// 16^3 hoist their loads (174 vector registers) and the base pointers spill out of the scalar registers.
template <int VPS, int MODE>
__global__ __launch_bounds__(256) void k_diff_emit(DevMap now, DevMap then, DevParams p, MergeArgs X, DiffArgs D, const int4* __restrict__ cand,
                                                   DiffWork W, uint8_t* __restrict__ out) {
  constexpr int NV = VPS * VPS * VPS, NG = NV / 64, SH = VPS == 16 ? 4 : 3;
  static_assert(NG <= 64 && NG % 4 == 0 && NG / 4 <= 16, "one ballot per group, the groups dealt to four waves, two kind bits per group");
  __shared__ float s_M[16];
  __shared__ unsigned long long s_bal[NG];
  __shared__ uint32_t s_base[NG];
  mergeStageTransform<MODE>(p, X, s_M);
  const uint32_t b = blockIdx.x;
  if (b >= W.n_blocks) return;  // (uniform)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t ci = min(W.sorted_cand[b], W.cap - 1u);
  const int4 c = cand[ci];
  const uint32_t slot = diffCandSlot(W)[ci], first = W.blk_first[b];
  if (slot >= now.capacity) return;  // (uniform; the count kernel stored a live slot)
  const size_t o = static_cast<size_t>(slot) * NV;
  uint32_t kinds = 0u;  // two bits per group of this wave
#pragma unroll 1
  for (int it = 0; it < NG / 4; ++it) {
    const uint32_t g = wave + 4u * it, lin = 64u * g + lane;
    float d_then;
    uint32_t ss, sl;
    const bool T = mergeLocate<VPS, MODE>(then, p, X, s_M, c.x, c.y, c.z, lin, &d_then, &ss, &sl);
    const bool N = now.weight[o + lin] >= X.min_weight;
    const DiffClass k = diffClassify(N, T, now.dist[o + lin], d_then, D);
    const uint32_t kind = k.appeared ? kDiffAppeared : (k.disappeared ? kDiffDisappeared : 0u);
    kinds |= kind << (2 * it);
    const unsigned long long bal = __ballot(kind != 0u);
    if (lane == 0) s_bal[g] = bal;
  }
  __syncthreads();
  if (wave == 0) {  // exclusive prefix over the NG popcounts
    const uint32_t v = lane < static_cast<uint32_t>(NG) ? static_cast<uint32_t>(__popcll(s_bal[lane])) : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= static_cast<uint32_t>(d)) incl += up;
    }
    if (lane < static_cast<uint32_t>(NG)) s_base[lane] = incl - v;
  }
  __syncthreads();
  const DiffLayout L = diffLayout(W.n_voxels, W.n_blocks);
  if (threadIdx.x == 0) {
    int32_t* const blocks = reinterpret_cast<int32_t*>(out + L.blocks) + 3 * static_cast<size_t>(b);
    blocks[0] = c.x, blocks[1] = c.y, blocks[2] = c.z;
    reinterpret_cast<uint32_t*>(out + L.block_appeared)[b] = diffCandAppeared(W)[ci];
    reinterpret_cast<uint32_t*>(out + L.block_disappeared)[b] = diffCandDisappeared(W)[ci];
    reinterpret_cast<uint32_t*>(out + L.block_first)[b] = first;
  }
#pragma unroll 1
  for (int it = 0; it < NG / 4; ++it) {
    const uint32_t kind = (kinds >> (2 * it)) & 3u;
    if (kind == 0u) continue;
    const uint32_t g = wave + 4u * it, lin = 64u * g + lane;
    const unsigned long long below = s_bal[g] & ((1ull << lane) - 1ull);
    const size_t pos = static_cast<size_t>(first) + s_base[g] + static_cast<uint32_t>(__popcll(below));
    if (pos >= W.n_voxels) continue;  // (cannot happen while the maps are what the count saw: no write beyond the arrays)
    float d_then;
    uint32_t ss, sl;
    mergeLocate<VPS, MODE>(then, p, X, s_M, c.x, c.y, c.z, lin, &d_then, &ss, &sl);
    uint32_t label_then = 0u;
    uint64_t stamp_then = 0ull;
    if (ss != kInvalidSlot) {
      if (p.with_semantics) label_then = then.sem_label[static_cast<size_t>(ss) * NV + sl];
      if (p.with_tracking) stamp_then = lastObserved(then, ss, sl, NV);
    }
    int32_t* const voxel = reinterpret_cast<int32_t*>(out + L.voxels) + 3 * pos;
    voxel[0] = c.x * VPS + static_cast<int>(lin & (VPS - 1));
    voxel[1] = c.y * VPS + static_cast<int>((lin >> SH) & (VPS - 1));
    voxel[2] = c.z * VPS + static_cast<int>(lin >> (2 * SH));
    (out + L.kind)[pos] = static_cast<uint8_t>(kind);
    reinterpret_cast<float*>(out + L.d_now)[pos] = now.dist[o + lin];
    reinterpret_cast<float*>(out + L.d_then)[pos] = d_then;
    reinterpret_cast<uint32_t*>(out + L.label)[pos] = kind == kDiffAppeared ? (p.with_semantics ? now.sem_label[o + lin] : 0u) : label_then;
    reinterpret_cast<uint64_t*>(out + L.stamp_now)[pos] = p.with_tracking ? lastObserved(now, slot, lin, NV) : 0ull;
    reinterpret_cast<uint64_t*>(out + L.stamp_then)[pos] = stamp_then;
  }
}

}  // namespace khr
