// khr_kernels_merge.h — device side of khr_merge_map (include/khronos_amd.h; ASSUMPTIONS.md A.17): another context's map fused
// into the live map, voxel to voxel under an integer voxel offset (ALIGNED) or sampled trilinearly at the destination's voxel
// centres under a rigid transform (RESAMPLE).  The source map is only read.  gfx950, wave64.
//   k_merge_candidates  every live source block -> the destination blocks it can reach, made unique through a scratch hash set
//   k_merge_probe       one workgroup per candidate: sample validity only; hit flag, destination slot, the counts the host reads
//   (the host's one wait: key range, pool space, statistics -- nothing of the destination has been written up to here)
//   k_merge_insert      hit-but-absent blocks take slots from the free list and enter the hash table (k_ckpt_insert's cursor and insert)
//   k_merge_rows        (semantics) one workgroup per touched block: labels and likelihood rows by A.17
//   k_merge_attributes  one workgroup per touched block: lazy forms of the destination resolved for all its voxels; flags and
//                       stamps by A.17; the block's public flags
//   k_merge_apply       one workgroup per touched block: distance, weight and colour by A.17
//   k_ckpt_rebuild      over the touched slots: the derived words (khr_kernels_checkpoint.h)
// The probe keeps no per-wave ballots: sized before the candidate count is known they would take 8 bytes per 64 voxels of every
// block the source's POOL could reach (hundreds of MB for a large pool); the three kernels that write evaluate the sample again
// instead, the same function (mergeLocate) on the same unchanged source.  Under RESAMPLE a lane probes each source block its
// eight taps touch once (one probe when the cube lies inside a block, as in k_query_points); sharing those probes across a wave
// of a 4x4x4 sub-cube is the next step if RESAMPLE merges of large maps matter.
#pragma once
#include "khr_device.h"
#include "khr_kernels_checkpoint.h"
#include "khr_kernels_query.h"
#include "khr_map_read.h"

namespace khr {

constexpr int kMergeAligned = 0, kMergeResample = 1;  // KHR_MERGE_*
constexpr int kMergeReachAligned = 8, kMergeReachResample = 27;

// counters of one merge (32-bit words; the two voxel counts are 64-bit words behind them)
enum MergeCounter : int {
  MC_SRC = 0,    // live source blocks
  MC_LIST,       // entries of the candidate list (in range and out of range)
  MC_CAND,       // ... of them inside the key range (unique)
  MC_TOUCHED,    // candidates with at least one valid sample
  MC_NEW,        // ... of them absent from the destination
  MC_ERR,        // bit 0: a touched block outside the key range, bit 1: the candidate list overflowed, bit 2: an insert failed
  MC_NLIST,      // touched slots (k_merge_insert -> k_merge_apply / k_ckpt_rebuild)
  MC_COUNT = 8   // (two 64-bit words follow: added voxels, merged voxels)
};
constexpr uint32_t kMergeErrRange = 1u, kMergeErrOverflow = 2u, kMergeErrInsert = 4u;

struct MergeArgs {
  int mode;
  int off[3];         // ALIGNED: destination voxel g receives source voxel g - off
  float M[12];        // RESAMPLE: src_T_dst, rows of [R | t]
  float F[12];        // RESAMPLE: dst_T_src (only for the candidate boxes)
  float min_weight;
  int ks_src;         // row stride of the source's likelihood array
  uint64_t src_stamp, dst_stamp;  // the latest tracking pass of either side = last_occupied of its VOX_OCC voxels
};

struct MergeScratch {
  uint64_t* set_keys;  // open-addressing set of candidate keys, kEmptyKey = free
  uint32_t set_mask;
  int4* cand;          // x, y, z, w: 0 inside the key range, 1 outside (never inserted; probed for the error alone)
  uint32_t cap;
  uint32_t* cand_slot;  // destination slot (k_merge_probe: present blocks, k_merge_insert: new ones)
  uint32_t* cand_hit;   // 0 no valid sample, 1 touched and present, 2 touched and absent
  uint32_t* touched;    // slots of the touched blocks
  uint32_t* ctr;        // MergeCounter
  unsigned long long* ctr64;  // [0] added voxels, [1] merged voxels
};

// floor(min) - 1 .. floor(max) + 1 of the transformed source block, clamped to +-2^30, as voxel indices
__device__ inline int mergeVoxelBound(float v, int margin) {
  const float c = fminf(fmaxf(floorf(v), -kMapIndexLimit), kMapIndexLimit);
  return static_cast<int>(c) + margin;
}

template <int VPS>
__global__ __launch_bounds__(256) void k_merge_candidates(DevMap src, DevParams p, MergeArgs X, MergeScratch S) {
  constexpr int SH = VPS == 16 ? 4 : 3;
  const uint32_t n_slots = min(src.counters[C_MAX_SLOT], src.capacity);
  for (uint32_t base = blockIdx.x * blockDim.x; base < n_slots; base += gridDim.x * blockDim.x) {  // (uniform per workgroup)
    const uint32_t s = base + threadIdx.x;
    const bool live = s < n_slots && (src.blk_flags[s] & BLK_LIVE);
    waveAggInc(&S.ctr[MC_SRC], live);
    if (!live) continue;
    const int4 bi = src.blk_index[s];
    const int b[3] = {bi.x, bi.y, bi.z};
    int lo[3], hi[3];
    if (X.mode == kMergeAligned) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const long long g = static_cast<long long>(b[a]) * VPS + X.off[a];
        lo[a] = static_cast<int>(g >> SH);
        hi[a] = static_cast<int>((g + (VPS - 1)) >> SH);
      }
    } else {
      // a destination voxel with a valid sample has its source point p inside [i0 + 0.5, i0 + 1.5) voxels with i0 a voxel of a
      // live block: the cube [origin + 0.5 voxel, origin + block + 0.5 voxel] of this block, transformed, one voxel of margin
      float mn[3], mx[3];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float l = static_cast<float>(b[a]) * p.bs + 0.5f * p.vs;
          q[a] = ((c >> a) & 1) ? l + p.bs : l;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float t = ((X.F[4 * a] * q[0] + X.F[4 * a + 1] * q[1]) + X.F[4 * a + 2] * q[2]) + X.F[4 * a + 3];
          mn[a] = c == 0 ? t : fminf(mn[a], t);
          mx[a] = c == 0 ? t : fmaxf(mx[a], t);
        }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = mergeVoxelBound(mn[a] * p.vs_inv, -1) >> SH;
        hi[a] = min(mergeVoxelBound(mx[a] * p.vs_inv, 1) >> SH, lo[a] + 2);  // (a rotated block spans at most three blocks per axis)
      }
    }
    for (int z = lo[2]; z <= hi[2]; ++z)
      for (int y = lo[1]; y <= hi[1]; ++y)
        for (int x = lo[0]; x <= hi[0]; ++x) {
          const bool in_range = blockInKeyRange(x, y, z);
          bool fresh = true;
          if (in_range) {  // unique through the set
            const uint64_t key = packKey(x, y, z);
            uint32_t h = hashKey(key) & S.set_mask;
            while (true) {
              const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(&S.set_keys[h]),
                                                        static_cast<unsigned long long>(kEmptyKey), static_cast<unsigned long long>(key));
              if (prev == kEmptyKey) break;
              if (prev == key) {
                fresh = false;
                break;
              }
              h = (h + 1) & S.set_mask;
            }
          }
          if (!fresh) continue;
          const uint32_t pos = atomicAdd(&S.ctr[MC_LIST], 1u);
          if (pos < S.cap) {
            S.cand[pos] = make_int4(x, y, z, in_range ? 0 : 1);
            if (in_range) atomicAdd(&S.ctr[MC_CAND], 1u);
          } else {
            atomicOr(&S.ctr[MC_ERR], kMergeErrOverflow);
          }
        }
  }
}

// RESAMPLE: src_T_dst and the sampler's four scalars into LDS, once per workgroup.  Read from there the sixteen words arrive in
// vector registers; as kernel arguments they stay in scalar registers for the whole kernel, which together with the base pointers
// of the two maps is more than there are (the kernels below then spill scalar registers).
template <int MODE>
__device__ inline void mergeStageTransform(const DevParams& p, const MergeArgs& X, float* s_M) {
  if (MODE != kMergeResample) return;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) s_M[i] = X.M[i];
    s_M[12] = p.bs, s_M[13] = p.vs, s_M[14] = p.vs_inv, s_M[15] = X.min_weight;  // (the sampler's four scalars ride along)
  }
  __syncthreads();
}

// The source sample of voxel `lin` of destination block (bx, by, bz) (A.17; M: the words mergeStageTransform staged): valid?,
// *d_s = the distance, *s_slot / *s_lin = the source voxel the other values come from (kInvalidSlot: none, every value 0).
template <int VPS, int MODE>
__device__ inline bool mergeLocate(const DevMap& src, const DevParams& p, const MergeArgs& X, const float* M, int bx, int by, int bz,
                                   uint32_t lin, float* d_s, uint32_t* s_slot, uint32_t* s_lin) {
  constexpr int NV = VPS * VPS * VPS, SH = VPS == 16 ? 4 : 3;
  const int b[3] = {bx, by, bz};
  const int iv[3] = {static_cast<int>(lin & (VPS - 1)), static_cast<int>((lin >> SH) & (VPS - 1)), static_cast<int>(lin >> (2 * SH))};
  *s_slot = kInvalidSlot;
  *s_lin = 0u;
  *d_s = 0.f;
  if (MODE == kMergeAligned) {
    int sb[3], sl[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const long long g = static_cast<long long>(b[a]) * VPS + iv[a] - X.off[a];
      sb[a] = static_cast<int>(g >> SH);  // floor division (A.1)
      sl[a] = static_cast<int>(g & (VPS - 1));
    }
    if (!blockInKeyRange(sb[0], sb[1], sb[2])) return false;
    const uint32_t s = htLookup(src, packKey(sb[0], sb[1], sb[2]));
    if (s == kInvalidSlot) return false;
    const uint32_t l = static_cast<uint32_t>(sl[0] + VPS * (sl[1] + VPS * sl[2]));
    const size_t at = static_cast<size_t>(s) * NV + l;
    if (!(src.weight[at] >= X.min_weight)) return false;
    *d_s = src.dist[at];
    *s_slot = s;
    *s_lin = l;
    return true;
  }
  // RESAMPLE: khr_query_points(src, p, min_weight) at the transformed centre (A.13)
  const float bs = M[12], vs = M[13], vs_inv = M[14], min_weight = M[15];
  float c[3], pw[3], g[3], f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = static_cast<float>(b[a]) * bs + (static_cast<float>(iv[a]) + 0.5f) * vs;
  bool in_range = true;
  int i0[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    pw[a] = ((M[4 * a] * c[0] + M[4 * a + 1] * c[1]) + M[4 * a + 2] * c[2]) + M[4 * a + 3];
    g[a] = pw[a] * vs_inv - 0.5f;
    in_range = in_range && (fabsf(g[a]) < kMapIndexLimit);  // (false for NaN)
  }
  if (!in_range) return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float fl = floorf(g[a]);
    i0[a] = static_cast<int>(fl);
    f[a] = g[a] - fl;
  }
  // the eight taps lie in at most two blocks per axis: each block is probed once (one probe when the cube lies inside a block)
  int lo[3];
  bool up[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = i0[a] >> SH;  // floor division (arithmetic shift)
    up[a] = ((i0[a] + 1) >> SH) != lo[a];
  }
  uint32_t slots[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    slots[c] = kInvalidSlot;
    if ((!(c & 1) || up[0]) && (!(c & 2) || up[1]) && (!(c & 4) || up[2])) {
      const int tx = lo[0] + (c & 1), ty = lo[1] + ((c >> 1) & 1), tz = lo[2] + (c >> 2);
      if (blockInKeyRange(tx, ty, tz)) slots[c] = htLookup(src, packKey(tx, ty, tz));
    }
  }
  float v[8];
  bool all = true;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int x = i0[0] + (t & 1), y = i0[1] + ((t >> 1) & 1), z = i0[2] + (t >> 2);
    const uint32_t s = querySlot(slots, (t & 1) && up[0], ((t >> 1) & 1) && up[1], (t >> 2) && up[2]);
    const bool found = s != kInvalidSlot;
    const size_t at = static_cast<size_t>(found ? s : 0u) * NV + static_cast<size_t>((x & (VPS - 1)) + VPS * ((y & (VPS - 1)) + VPS * (z & (VPS - 1))));
    v[t] = src.dist[at];
    all = all && found && (src.weight[at] >= min_weight);
  }
  if (!all) return false;
  *d_s = fminf(fmaxf(trilinear(v, f), -p.trunc), p.trunc);
  // attribute voxel: floor(p * voxel_size_inv)
  float gi[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    gi[a] = floorf(pw[a] * vs_inv);
    ok = ok && (fabsf(gi[a]) < kMapIndexLimit);
  }
  if (ok) {
    const int ix = static_cast<int>(gi[0]), iy = static_cast<int>(gi[1]), iz = static_cast<int>(gi[2]);
    const int ax = ix >> SH, ay = iy >> SH, az = iz >> SH;
    const uint32_t s = blockInKeyRange(ax, ay, az) ? htLookup(src, packKey(ax, ay, az)) : kInvalidSlot;
    if (s != kInvalidSlot) {
      *s_slot = s;
      *s_lin = static_cast<uint32_t>((ix & (VPS - 1)) + VPS * ((iy & (VPS - 1)) + VPS * (iz & (VPS - 1))));
    }
  }
  return true;
}

// One workgroup per candidate, one wave per 64 voxels: which candidates have a valid sample, where they live in the destination,
// and the voxel counts.  Writes scratch only.
template <int VPS, int MODE>
__global__ __launch_bounds__(256) void k_merge_probe(DevMap dst, DevMap src, DevParams p, MergeArgs X, MergeScratch S) {
  constexpr int NV = VPS * VPS * VPS, NG = NV / 64;
  __shared__ float s_M[16];
  mergeStageTransform<MODE>(p, X, s_M);
  const uint32_t n = min(S.ctr[MC_LIST], S.cap);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const int4 c = S.cand[ci];
    const bool in_range = c.w == 0;
    const uint32_t dslot = in_range ? htLookup(dst, packKey(c.x, c.y, c.z)) : kInvalidSlot;
    uint32_t n_valid = 0u, n_added = 0u;
    for (uint32_t g = wave; g < static_cast<uint32_t>(NG); g += 4) {
      const uint32_t lin = 64u * g + lane;
      float d_s;
      uint32_t ss, sl;
      if (mergeLocate<VPS, MODE>(src, p, X, s_M, c.x, c.y, c.z, lin, &d_s, &ss, &sl)) {
        ++n_valid;
        if (dslot == kInvalidSlot || dst.weight[static_cast<size_t>(dslot) * NV + lin] == 0.f) ++n_added;
      }
    }
    const int hit = __syncthreads_or(n_valid != 0u);
    if (hit && in_range) {
      waveStatAdd(&S.ctr64[0], n_added);
      waveStatAdd(&S.ctr64[1], n_valid - n_added);
    }
    if (threadIdx.x == 0) {
      S.cand_slot[ci] = dslot;
      S.cand_hit[ci] = hit ? (dslot == kInvalidSlot ? 2u : 1u) : 0u;
      if (hit) {
        if (!in_range) {
          atomicOr(&S.ctr[MC_ERR], kMergeErrRange);
        } else {
          atomicAdd(&S.ctr[MC_TOUCHED], 1u);
          if (dslot == kInvalidSlot) atomicAdd(&S.ctr[MC_NEW], 1u);
        }
      }
    }
  }
}

// One thread per candidate: a touched block the destination lacks takes a pool slot (the wave-aggregated cursor and the unique
// insert of k_ckpt_insert); every touched block's slot goes to the list k_merge_apply and k_ckpt_rebuild walk.  The host has
// checked that the free list holds enough slots.
__global__ __launch_bounds__(256) void k_merge_insert(DevMap dst, MergeScratch S) {
  const uint32_t n = min(S.ctr[MC_LIST], S.cap);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t hit = i < n ? S.cand_hit[i] : 0u;
  const bool need = hit == 2u;
  const uint32_t fidx = waveAggInc(&dst.counters[C_FREE_HEAD], need);
  uint32_t slot = hit == 1u ? S.cand_slot[i] : kInvalidSlot;
  if (need) {
    bool ok = false;
    if (fidx < dst.counters[C_N_FREE] && fidx < dst.capacity && dst.free_slots[fidx] < dst.capacity) {
      const uint32_t s = dst.free_slots[fidx];
      const int4 c = S.cand[i];
      if (ckptInsert(dst, packKey(c.x, c.y, c.z), s)) {
        ok = true;
        slot = s;
        dst.blk_index[s] = make_int4(c.x, c.y, c.z, 0);
        dst.blk_flags[s] = BLK_LIVE;  // (k_merge_apply adds the public bits, k_ckpt_rebuild the derived ones)
        dst.mesh_desc[s] = MeshDesc{0u, 0u};
        atomicMax(&dst.counters[C_MAX_SLOT], s + 1);
      }
    }
    if (!ok) atomicOr(&S.ctr[MC_ERR], kMergeErrInsert);
    S.cand_slot[i] = slot;
  }
  const bool listed = slot != kInvalidSlot && hit != 0u;
  const uint32_t pos = waveAggInc(&S.ctr[MC_NLIST], listed);
  if (listed) S.touched[pos] = slot;
}

// The touched blocks are rewritten by three kernels, in this order: between them they name some forty arrays of the two maps, more
// base pointers than one kernel holds in scalar registers without spilling.  Each runs one workgroup per touched block and one wave
// per 64 consecutive voxels (x-rows: destination loads and stores are contiguous, and under ALIGNED the source's are too).  Each
// takes "destination unobserved" from the weight layer as it was before the merge, which only the last one (k_merge_apply)
// writes; k_merge_rows reads the voxel flags before k_merge_attributes rewrites them.
//
// k_merge_rows (maps with semantics): labels and likelihood rows (A.17); a new block's unsampled voxels get label 0.  The row
// layouts of the two sides are independent (KS of either).
template <int VPS, int MODE>
__global__ __launch_bounds__(256) void k_merge_rows(DevMap dst, DevMap src, DevParams p, MergeArgs X, MergeScratch S) {
  constexpr int NV = VPS * VPS * VPS, NG = NV / 64;
  __shared__ float s_M[16];
  mergeStageTransform<MODE>(p, X, s_M);
  const uint32_t n = min(S.ctr[MC_LIST], S.cap);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t K = static_cast<uint32_t>(p.K), KD = static_cast<uint32_t>(p.KS), KSRC = static_cast<uint32_t>(X.ks_src);
  for (uint32_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const uint32_t hit = S.cand_hit[ci], slot = S.cand_slot[ci];
    if (hit == 0u || slot >= dst.capacity) continue;  // (uniform)
    const int4 c = S.cand[ci];
    const bool is_new = hit == 2u;
    const size_t o = static_cast<size_t>(slot) * NV;
    for (uint32_t g = wave; g < static_cast<uint32_t>(NG); g += 4) {
      const uint32_t lin = 64u * g + lane;
      const size_t at = o + lin;
      float d_s;
      uint32_t ss, sl;
      const bool valid = mergeLocate<VPS, MODE>(src, p, X, s_M, c.x, c.y, c.z, lin, &d_s, &ss, &sl);
      uint32_t lab = 0u;
      bool write = is_new;
      if (valid) {
        const bool unobserved = is_new || dst.weight[at] == 0.f;
        const bool sem_d = !is_new && (dst.vflags[at] & VOX_SEM_VALID) != 0;
        const size_t sat = static_cast<size_t>(ss == kInvalidSlot ? 0u : ss) * NV + sl;
        const bool sem_s = ss != kInvalidSlot && (src.vflags[sat] & VOX_SEM_VALID) != 0;
        const uint32_t lab_s = ss != kInvalidSlot ? src.sem_label[sat] : 0u;
        if (unobserved) {  // the source's label (and row, if it has one) unchanged
          lab = lab_s;
          write = true;
        }
        if (sem_s) {
          if (unobserved || !sem_d) {
            for (uint32_t k = 0; k < K; ++k) dst.lik[at * KD + k] = src.lik[sat * KSRC + k];
            lab = lab_s;
          } else {  // rows add (sums of log-likelihoods / counts); first argmax
            float best = 0.f;
            for (uint32_t k = 0; k < K; ++k) {
              const float l = dst.lik[at * KD + k] + src.lik[sat * KSRC + k];
              dst.lik[at * KD + k] = l;
              if (k == 0u || l > best) {
                best = l;
                lab = k;
              }
            }
          }
          write = true;
        }
      }
      if (write) dst.sem_label[at] = lab;
    }
  }
}

// k_merge_attributes: voxel flags and stamps (A.17), and the block's public flags.  Every voxel of the block leaves in its public
// form: deferred last_observed and VOX_OCC resolved as k_ckpt_pack resolves them, a new block's unsampled voxels as k_init_blocks
// leaves them.
template <int VPS, int MODE>
__global__ __launch_bounds__(256) void k_merge_attributes(DevMap dst, DevMap src, DevParams p, MergeArgs X, MergeScratch S) {
  constexpr int NV = VPS * VPS * VPS, NG = NV / 64;
  __shared__ float s_M[16];
  mergeStageTransform<MODE>(p, X, s_M);
  const uint32_t n = min(S.ctr[MC_LIST], S.cap);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const uint32_t hit = S.cand_hit[ci], slot = S.cand_slot[ci];
    if (hit == 0u || slot == kInvalidSlot) continue;  // (uniform)
    const int4 c = S.cand[ci];
    const bool is_new = hit == 2u;
    const size_t o = static_cast<size_t>(slot) * NV;
    bool active = false;
    for (uint32_t g = wave; g < static_cast<uint32_t>(NG); g += 4) {
      const uint32_t lin = 64u * g + lane;
      const size_t at = o + lin;
      // the destination voxel's public values
      bool unobserved = true;
      uint8_t vf_d = 0;
      uint64_t lobs_d = 0ull, locc_d = 0ull;
      if (!is_new) {
        unobserved = dst.weight[at] == 0.f;
        const uint8_t raw = dst.vflags[at];
        vf_d = raw & VOX_PUBLIC_MASK;
        if (p.with_tracking) {
          lobs_d = lastObserved(dst, slot, lin, NV);
          locc_d = (raw & VOX_OCC) ? X.dst_stamp : dst.last_occ[at];
        }
      }
      float d_s;
      uint32_t ss, sl;
      if (mergeLocate<VPS, MODE>(src, p, X, s_M, c.x, c.y, c.z, lin, &d_s, &ss, &sl)) {
        uint8_t vf_s = 0;
        uint64_t lobs_s = 0ull, locc_s = 0ull;
        if (ss != kInvalidSlot) {
          const size_t sat = static_cast<size_t>(ss) * NV + sl;
          const uint8_t raw = src.vflags[sat];
          vf_s = raw & VOX_PUBLIC_MASK;
          if (p.with_tracking) {
            lobs_s = lastObserved(src, ss, sl, NV);
            locc_s = (raw & VOX_OCC) ? X.src_stamp : src.last_occ[sat];
          }
        }
        if (unobserved) {  // the source's values unchanged
          vf_d = vf_s;
          lobs_d = lobs_s;
          locc_d = locc_s;
        } else {
          lobs_d = lobs_s > lobs_d ? lobs_s : lobs_d;
          locc_d = locc_s > locc_d ? locc_s : locc_d;
          vf_d = static_cast<uint8_t>(((vf_d | vf_s) & (VOX_ACTIVE | VOX_SEM_VALID)) | (vf_d & vf_s & (VOX_EVER_FREE | VOX_TO_REMOVE)));
        }
      }
      dst.vflags[at] = vf_d;  // (public bits: VOX_OCC is resolved)
      if (p.with_tracking) {
        dst.last_obs[at] = lobs_d;
        dst.last_occ[at] = locc_d;
      }
      active = active || (vf_d & VOX_ACTIVE);
    }
    const int any_active = __syncthreads_or(active);
    if (threadIdx.x == 0)  // (a new block's word is k_merge_insert's BLK_LIVE)
      dst.blk_flags[slot] = dst.blk_flags[slot] | BLK_UPDATED | BLK_MESH_UPDATED | BLK_TRACKING_UPDATED | (any_active ? BLK_HAS_ACTIVE : 0u);
  }
}

// k_merge_apply: distance, weight and colour (A.17); a new block's unsampled voxels are zero
template <int VPS, int MODE>
__global__ __launch_bounds__(256) void k_merge_apply(DevMap dst, DevMap src, DevParams p, MergeArgs X, MergeScratch S) {
  constexpr int NV = VPS * VPS * VPS, NG = NV / 64;
  __shared__ float s_M[16];
  mergeStageTransform<MODE>(p, X, s_M);
  const uint32_t n = min(S.ctr[MC_LIST], S.cap);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const uint32_t hit = S.cand_hit[ci], slot = S.cand_slot[ci];
    if (hit == 0u || slot >= dst.capacity) continue;  // (uniform)
    const int4 c = S.cand[ci];
    const bool is_new = hit == 2u;
    const size_t o = static_cast<size_t>(slot) * NV;
    for (uint32_t g = wave; g < static_cast<uint32_t>(NG); g += 4) {
      const uint32_t lin = 64u * g + lane;
      const size_t at = o + lin;
      float d_d = 0.f, w_d = 0.f;
      uint32_t col_d = 0u;
      if (!is_new) {
        d_d = dst.dist[at];
        w_d = dst.weight[at];
        col_d = dst.color[at];
      }
      float d_s;
      uint32_t ss, sl;
      const bool valid = mergeLocate<VPS, MODE>(src, p, X, s_M, c.x, c.y, c.z, lin, &d_s, &ss, &sl);
      if (valid) {
        float w_s = 0.f;
        uint32_t col_s = 0u;
        if (ss != kInvalidSlot) {
          const size_t sat = static_cast<size_t>(ss) * NV + sl;
          w_s = src.weight[sat];
          col_s = src.color[sat];
        }
        if (w_d == 0.f) {  // destination unobserved (or the block is new): the source's values unchanged
          d_d = d_s;
          w_d = fminf(w_s, p.max_weight);
          col_d = col_s;
        } else {
          const float ws = w_d + w_s;
          d_d = (d_d * w_d + d_s * w_s) / ws;
          const uint32_t a_s = col_s >> 24, a_d = col_d >> 24;
          if (a_s != 0u) {
            if (a_d == 0u) {
              col_d = col_s;
            } else {
              uint32_t out = 0xff000000u;
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) {
                const float cd = static_cast<float>((col_d >> (8 * ch)) & 0xffu), cs = static_cast<float>((col_s >> (8 * ch)) & 0xffu);
                out |= static_cast<uint32_t>(floorf((cd * w_d + cs * w_s) / ws + 0.5f)) << (8 * ch);
              }
              col_d = out;
            }
          }
          w_d = fminf(ws, p.max_weight);
        }
      }
      if (valid || is_new) {
        dst.dist[at] = d_d;
        dst.weight[at] = w_d;
        dst.color[at] = col_d;
      }
    }
  }
}

}  // namespace khr
