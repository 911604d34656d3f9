// khr_kernels_checkpoint.h — device side of khr_checkpoint_save / khr_checkpoint_load (include/khronos_amd.h): the live map as one
// slot-independent stream of public values and back.  gfx950 only.
//   save:  k_ckpt_select -> bitonic sort of khr_kernels_slice.h (keys in (x, y, z) order) -> k_ckpt_pack per chunk of blocks
//   load:  k_ckpt_insert + k_ckpt_unpack per chunk of blocks -> k_ckpt_rebuild once over the restored blocks
// A chunk travels through a staging area of fixed size (CkptStage: one region per section, blocks in stream order), so that the
// copy of chunk i overlaps the kernels of chunk i + 1 and the device footprint does not grow with the map.
#pragma once
#include "khr_device.h"
#include "khr_kernels_slice.h"

namespace khr {

// sort key of a block: biased x | y | z, 21 bits each, x most significant -- ascending keys are the lexicographic (x, y, z)
// order of khr_block_indices.  (packKey has x lowest: the hash key is rebuilt from the sort key.)
__host__ __device__ inline uint64_t ckptSortKey(int x, int y, int z) {
  return (static_cast<uint64_t>(static_cast<uint32_t>(x + (1 << 20)) & 0x1fffffu) << 42) |
         (static_cast<uint64_t>(static_cast<uint32_t>(y + (1 << 20)) & 0x1fffffu) << 21) |
         (static_cast<uint64_t>(static_cast<uint32_t>(z + (1 << 20)) & 0x1fffffu));
}
__host__ __device__ inline void ckptSortKeyIndex(uint64_t k, int* x, int* y, int* z) {
  *x = static_cast<int>((k >> 42) & 0x1fffffu) - (1 << 20);
  *y = static_cast<int>((k >> 21) & 0x1fffffu) - (1 << 20);
  *z = static_cast<int>(k & 0x1fffffu) - (1 << 20);
}

// one chunk of the stream in device memory: blocks [b0, b0 + nb) of every section, a section the configuration does not have is
// nullptr.  Every region starts on a 256-byte boundary; a block's share of a voxel layer is a multiple of 16 bytes.
struct CkptStage {
  int32_t* idx;    // [block][3]
  float* dist;
  float* weight;
  uint32_t* color;
  uint64_t* lobs;
  uint64_t* locc;
  uint8_t* vfl;
  uint32_t* label;
  uint8_t* bfl;    // [block] public block flags
  float* lik;      // [block][voxel][K], rows packed
};

// error bits of a load (k_ckpt_insert)
constexpr uint32_t kCkptErrPool = 1u, kCkptErrDuplicate = 2u, kCkptErrIndex = 4u;

// every live slot -> keys[count++] (the map's blocks in no order yet)
__global__ __launch_bounds__(256) void k_ckpt_select(DevMap m, uint32_t* __restrict__ count, uint64_t* __restrict__ keys) {
  const uint32_t n_slots = min(m.counters[C_MAX_SLOT], m.capacity);
  for (uint32_t base = blockIdx.x * blockDim.x; base < n_slots; base += gridDim.x * blockDim.x) {  // (uniform per workgroup)
    const uint32_t s = base + threadIdx.x;
    bool take = false;
    int4 bi = make_int4(0, 0, 0, 0);
    if (s < n_slots && (m.blk_flags[s] & BLK_LIVE)) {
      bi = m.blk_index[s];
      take = true;
    }
    const uint32_t pos = waveAggInc(count, take);
    if (take) keys[pos] = ckptSortKey(bi.x, bi.y, bi.z);
  }
}

// Blocks [b0, b0 + nb) of the sorted list -> the staging area, one workgroup per block, 16-byte loads and stores.  The lazy
// forms are resolved as khr_download_block resolves them: last_observed through DevMap::obs, last_occupied of a VOX_OCC voxel
// = the latest tracking pass's stamp, public flag bits only, likelihood rows packed (and zero for a voxel without a semantic
// entry, whose storage is undefined).
template <int VPS>
__global__ __launch_bounds__(256) void k_ckpt_pack(DevMap m, DevParams p, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ count,
                                                  uint32_t b0, uint32_t nb, CkptStage o, uint64_t track_stamp) {
  constexpr int NV = VPS * VPS * VPS;
  const uint32_t n = *count;
  for (uint32_t bl = blockIdx.x; bl < nb; bl += gridDim.x) {
    if (b0 + bl >= n) break;
    int x, y, z;
    ckptSortKeyIndex(keys[b0 + bl], &x, &y, &z);
    const uint32_t slot = htLookup(m, packKey(x, y, z));
    if (slot == kInvalidSlot) continue;  // (a listed block is live: not taken)
    const size_t src = static_cast<size_t>(slot) * NV, dst = static_cast<size_t>(bl) * NV;
    auto copy16 = [&](const void* s, void* d, size_t bytes) {
      const uint4* s4 = reinterpret_cast<const uint4*>(s);
      uint4* d4 = reinterpret_cast<uint4*>(d);
      for (size_t i = threadIdx.x; i < bytes / 16; i += 256) d4[i] = s4[i];
    };
    copy16(m.dist + src, o.dist + dst, NV * 4);
    copy16(m.weight + src, o.weight + dst, NV * 4);
    copy16(m.color + src, o.color + dst, NV * 4);
    {
      const uint4* s4 = reinterpret_cast<const uint4*>(m.vflags + src);
      uint4* d4 = reinterpret_cast<uint4*>(o.vfl + dst);
      const uint32_t pm = VOX_PUBLIC_MASK * 0x01010101u;
      for (int i = threadIdx.x; i < NV / 16; i += 256) {
        const uint4 v = s4[i];
        d4[i] = make_uint4(v.x & pm, v.y & pm, v.z & pm, v.w & pm);
      }
    }
    if (o.lobs) {  // two voxels per thread and store
      const ulonglong2* s2 = reinterpret_cast<const ulonglong2*>(m.last_obs + src);
      const uint16_t* f2 = reinterpret_cast<const uint16_t*>(m.vflags + src);
      ulonglong2* lo2 = reinterpret_cast<ulonglong2*>(o.lobs + dst);
      ulonglong2* oc2 = reinterpret_cast<ulonglong2*>(o.locc + dst);
      const ulonglong2* q2 = reinterpret_cast<const ulonglong2*>(m.last_occ + src);
      for (int i = threadIdx.x; i < NV / 2; i += 256) {
        const ulonglong2 w = m.obs[static_cast<size_t>(slot) * (NV / 64) + (i >> 5)];
        const uint32_t bits = static_cast<uint32_t>(w.x >> ((2 * i) & 63)) & 3u;
        ulonglong2 v = s2[i];
        if (bits & 1u) v.x = w.y;
        if (bits & 2u) v.y = w.y;
        lo2[i] = v;
        const uint32_t f = f2[i];
        ulonglong2 q = q2[i];
        if (f & VOX_OCC) q.x = track_stamp;
        if ((f >> 8) & VOX_OCC) q.y = track_stamp;
        oc2[i] = q;
      }
    }
    if (o.label) copy16(m.sem_label + src, o.label + dst, NV * 4);
    if (o.lik) {
      const uint32_t K = static_cast<uint32_t>(p.K), KS = static_cast<uint32_t>(p.KS);
      float4* d4 = reinterpret_cast<float4*>(o.lik + dst * K);
      for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(NV) * K / 4u; i += 256) {
        float r[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t e = 4u * i + j, v = e / K, k = e - v * K;
          r[j] = (m.vflags[src + v] & VOX_SEM_VALID) ? m.lik[(src + v) * KS + k] : 0.f;
        }
        d4[i] = make_float4(r[0], r[1], r[2], r[3]);
      }
    }
    if (threadIdx.x < 3) o.idx[3 * static_cast<size_t>(bl) + threadIdx.x] = threadIdx.x == 0 ? x : (threadIdx.x == 1 ? y : z);
    if (threadIdx.x == 0) o.bfl[bl] = static_cast<uint8_t>(m.blk_flags[slot] & 0xfu);
  }
}

// 64-bit CAS insert that notices a key which is already there (htInsertUnique assumes it is not)
__device__ inline bool ckptInsert(const DevMap& m, uint64_t key, uint32_t slot) {
  uint32_t h = hashKey(key) & m.ht_mask;
  while (true) {
    const unsigned long long prev =
        atomicCAS(reinterpret_cast<unsigned long long*>(&m.ht_keys[h]), static_cast<unsigned long long>(kEmptyKey),
                  static_cast<unsigned long long>(key));
    if (prev == kEmptyKey) {
      m.ht_vals[h] = slot;
      return true;
    }
    if (prev == key) return false;
    h = (h + 1) & m.ht_mask;
  }
}

// One thread per block of the chunk: the blocks this rank owns take pool slots from the free list (the same wave-aggregated
// cursor as k_alloc_list) and enter the hash table; slots[i] = the block's slot, kInvalidSlot for a block that is skipped.
// The block flags are the stream's public bits for now; k_ckpt_rebuild adds the derived ones.
__global__ __launch_bounds__(256) void k_ckpt_insert(DevMap m, DevParams p, const int32_t* __restrict__ idx, const uint8_t* __restrict__ bfl,
                                                    uint32_t nb, uint32_t* __restrict__ slots, uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool mine = false;
  int x = 0, y = 0, z = 0;
  if (i < nb) {
    x = idx[3 * i];
    y = idx[3 * i + 1];
    z = idx[3 * i + 2];
    const int lim = 1 << 20;
    if (x < -lim || x >= lim || y < -lim || y >= lim || z < -lim || z >= lim) atomicOr(err, kCkptErrIndex);
    else mine = ownerOf(x, y, z, p.world) == p.rank;
  }
  const uint32_t fidx = waveAggInc(&m.counters[C_FREE_HEAD], mine);
  uint32_t slot = kInvalidSlot;
  if (mine) {
    if (fidx < m.counters[C_N_FREE] && fidx < m.capacity && m.free_slots[fidx] < m.capacity) {
      const uint32_t s = m.free_slots[fidx];
      if (ckptInsert(m, packKey(x, y, z), s)) {
        slot = s;
        m.blk_index[s] = make_int4(x, y, z, 0);
        m.blk_flags[s] = BLK_LIVE | (bfl[i] & 0xfu);
        m.mesh_desc[s] = MeshDesc{0u, 0u};
        atomicMax(&m.counters[C_MAX_SLOT], s + 1);
      } else {
        atomicOr(err, kCkptErrDuplicate);
      }
    } else {
      atomicOr(err, kCkptErrPool);
    }
  }
  waveAggInc(&m.counters[C_N_LIVE], slot != kInvalidSlot);
  if (i < nb) slots[i] = slot;
}

// the chunk's voxel layers into the pool, in its own stride; one workgroup per block, 16-byte loads and stores
template <int VPS>
__global__ __launch_bounds__(256) void k_ckpt_unpack(DevMap m, DevParams p, const uint32_t* __restrict__ slots, uint32_t nb, CkptStage in) {
  constexpr int NV = VPS * VPS * VPS;
  for (uint32_t bl = blockIdx.x; bl < nb; bl += gridDim.x) {
    const uint32_t slot = slots[bl];
    if (slot >= m.capacity) continue;  // skipped block (another rank's, or refused)
    const size_t dst = static_cast<size_t>(slot) * NV, src = static_cast<size_t>(bl) * NV;
    auto copy16 = [&](const void* s, void* d, size_t bytes) {
      const uint4* s4 = reinterpret_cast<const uint4*>(s);
      uint4* d4 = reinterpret_cast<uint4*>(d);
      for (size_t i = threadIdx.x; i < bytes / 16; i += 256) d4[i] = s4[i];
    };
    copy16(in.dist + src, m.dist + dst, NV * 4);
    copy16(in.weight + src, m.weight + dst, NV * 4);
    copy16(in.color + src, m.color + dst, NV * 4);
    {  // public bits only, whatever the stream holds: the internal ones are k_ckpt_rebuild's
      const uint4* s4 = reinterpret_cast<const uint4*>(in.vfl + src);
      uint4* d4 = reinterpret_cast<uint4*>(m.vflags + dst);
      const uint32_t pm = VOX_PUBLIC_MASK * 0x01010101u;
      for (int i = threadIdx.x; i < NV / 16; i += 256) {
        const uint4 v = s4[i];
        d4[i] = make_uint4(v.x & pm, v.y & pm, v.z & pm, v.w & pm);
      }
    }
    if (p.with_tracking && in.lobs) {
      copy16(in.lobs + src, m.last_obs + dst, NV * 8);
      copy16(in.locc + src, m.last_occ + dst, NV * 8);
    }
    if (p.with_semantics && in.label) {
      copy16(in.label + src, m.sem_label + dst, NV * 4);
      const uint32_t K = static_cast<uint32_t>(p.K), KS = static_cast<uint32_t>(p.KS);
      if (KS == K) {
        copy16(in.lik + src * K, m.lik + dst * K, static_cast<size_t>(NV) * K * 4);
      } else {  // packed rows in the stream, padded rows in the pool (the padding is never read as a value)
        const float4* s4 = reinterpret_cast<const float4*>(in.lik + src * K);
        for (uint32_t i = threadIdx.x; i < static_cast<uint32_t>(NV) * K / 4u; i += 256) {
          const float4 r = s4[i];
          const float rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t e = 4u * i + j, v = e / K, k = e - v * K;
            m.lik[(dst + v) * KS + k] = rv[j];
          }
        }
      }
    }
  }
}

// The derived words of every live block, recomputed from the restored layers: one workgroup per block, a wave per 64 voxels,
// ballots and shuffles inside the wave, LDS across the four waves.  Each word is either its maintaining kernel's definition or
// a value that kernel treats as "look again"; a restored block is flagged BLK_TRACK_DIRTY, so the first tracking pass after a
// load visits every block with its distances (k_tracking_select: need, reload) and rewrites the tracking words before anything
// reads them -- a full pass gives the results of a skipping one (the skips are exact, khr_kernels_fusion.h).
//   BLK_LIVE, public block bits  as inserted (k_ckpt_insert)
//   BLK_TRACK_DIRTY              set: conservative, the tracking pass may skip nothing (k_tracking_select)
//   BLK_ANY_KEEP                 exact: some voxel is not VOX_TO_REMOVE (k_tracking_update's any_keep; voxel flags change nowhere else)
//   BLK_HAS_NEG                  exact "holds a negative distance now" (k_fuse keeps the superset "has ever written one"; marching
//                                cubes only skips blocks that cannot contain a sign change, so the mesh is the same)
//   obs                          {0, 0} per 64 voxels: nothing deferred, last_obs holds every stamp
//   VOX_OCC                      clear on every voxel (the stream carries public bits): last_occ holds every stamp
//   freebits                     the ever-free bits: a subset of "free or ever-free" (k_tracking_update), which needs the stamp
//                                of the pass before the save; rewritten for every block by the first pass (all blocks dirty)
//                                before k_ever_free or a halo export reads it
//   trk_lim[0]                   exact: earliest last_observed of an active voxel
//   trk_lim[1]                   conservative (never later than the exact value): earliest last_occupied of an observed voxel
//                                that is not ever-free
//   blk_band                     per wave item, the voxels with weight > 0 inside the truncation band: an estimate of what
//                                k_fuse reports; only the culling pass's cost class reads it, the results do not depend on it
// list != nullptr: only the slots list[0, *n_list) (khr_merge_map: the blocks a merge has rewritten) instead of every live block
template <int VPS>
__global__ __launch_bounds__(256) void k_ckpt_rebuild(DevMap m, DevParams p, uint32_t wpb, const uint32_t* __restrict__ list = nullptr,
                                                     const uint32_t* __restrict__ n_list = nullptr) {
  constexpr int NV = VPS * VPS * VPS, NG = NV / 64, PATCHES = VPS * VPS / 64;
  __shared__ uint32_t s_band[kBandSlots];
  __shared__ unsigned long long s_min[2][4];
  __shared__ uint32_t s_bits;  // 1 = some voxel not to_remove, 2 = some distance negative
  const uint32_t n_slots = min(m.counters[C_MAX_SLOT], m.capacity);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t zr = max(1u, static_cast<uint32_t>(VPS) / max(1u, wpb / PATCHES));  // z steps per wave item (cullBlocks)
  const uint32_t n_items = list ? *n_list : n_slots;
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint32_t s = list ? list[it] : it;
    if (s >= n_slots) continue;  // (uniform)
    const uint32_t fl = m.blk_flags[s];
    if (!(fl & BLK_LIVE)) continue;  // (uniform)
    if (threadIdx.x < kBandSlots) s_band[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_bits = 0u;
    __syncthreads();
    const size_t o = static_cast<size_t>(s) * NV;
    bool keep = false, neg = false;
    unsigned long long a_min = ~0ull, f_min = ~0ull;
    for (uint32_t g = wave; g < NG; g += 4) {
      const uint32_t lin = 64u * g + lane;
      const float d = m.dist[o + lin], w = m.weight[o + lin];
      const uint8_t vf = m.vflags[o + lin];
      keep = keep || !(vf & VOX_TO_REMOVE);
      neg = neg || d < 0.f;
      const unsigned long long inband = __ballot(w > 0.f && fabsf(d) < p.trunc);
      if (lane == 0) {
        const uint32_t item = ((g % PATCHES) + PATCHES * ((g / PATCHES) / zr)) & (kBandSlots - 1);
        atomicAdd(&s_band[item], static_cast<uint32_t>(__popcll(inband)));
      }
      if (p.with_tracking) {
        const unsigned long long ever = __ballot((vf & VOX_EVER_FREE) != 0);
        const unsigned long long lo = m.last_obs[o + lin], oc = m.last_occ[o + lin];
        if ((vf & VOX_ACTIVE) && lo < a_min) a_min = lo;
        if (!(vf & VOX_EVER_FREE) && lo != 0ull && oc < f_min) f_min = oc;
        if (lane == 0) {
          m.freebits[static_cast<size_t>(s) * NG + g] = ever;
          m.obs[static_cast<size_t>(s) * NG + g] = make_ulonglong2(0ull, 0ull);
        }
      }
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
      const unsigned long long a2 = (static_cast<unsigned long long>(__shfl_xor(static_cast<uint32_t>(a_min >> 32), sh)) << 32) |
                                    __shfl_xor(static_cast<uint32_t>(a_min), sh);
      const unsigned long long f2 = (static_cast<unsigned long long>(__shfl_xor(static_cast<uint32_t>(f_min >> 32), sh)) << 32) |
                                    __shfl_xor(static_cast<uint32_t>(f_min), sh);
      a_min = a2 < a_min ? a2 : a_min;
      f_min = f2 < f_min ? f2 : f_min;
    }
    const uint32_t wbits = (__ballot(keep) != 0ull ? 1u : 0u) | (__ballot(neg) != 0ull ? 2u : 0u);
    if (lane == 0) {
      s_min[0][wave] = a_min;
      s_min[1][wave] = f_min;
      if (wbits) atomicOr(&s_bits, wbits);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long a = s_min[0][0], f = s_min[1][0];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        a = s_min[0][w] < a ? s_min[0][w] : a;
        f = s_min[1][w] < f ? s_min[1][w] : f;
      }
      if (p.with_tracking) reinterpret_cast<ulonglong2*>(m.trk_lim)[s] = make_ulonglong2(a, f);
      const uint32_t bits = s_bits;
      m.blk_flags[s] = (fl & (BLK_LIVE | 0xfu)) | BLK_TRACK_DIRTY | ((bits & 1u) ? BLK_ANY_KEEP : 0u) | ((bits & 2u) ? BLK_HAS_NEG : 0u);
    }
    if (threadIdx.x < kBandSlots)
      m.blk_band[static_cast<size_t>(s) * kBandSlots + threadIdx.x] = static_cast<uint16_t>(min(s_band[threadIdx.x], static_cast<uint32_t>(kItemBandMask)));
    __syncthreads();  // (the LDS words are reused by the workgroup's next block)
  }
}

}  // namespace khr
