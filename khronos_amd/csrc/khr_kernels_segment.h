// khr_kernels_segment.h — device side of khr_segment_map (include/khronos_amd.h; ASSUMPTIONS.md A.19): the connected components of
// the live map's member voxels (observed obstacle voxels that pass the request's flag and label filters) under 6-, 18- or
// 26-connectivity across block boundaries.  The map is only read.  gfx950, wave64.
//   k_ckpt_select + the bitonic sort of khr_kernels_slice.h   the live blocks in (x, y, z) order: a block's position is its rank
//   k_seg_local    one workgroup per block: membership (the one read of distance, weight, flags and label), the block's own
//                  voxels merged by union-find in LDS, one global parent word per voxel (or kSegNone), rank <-> slot tables
//   k_seg_seams    one workgroup per block, a launch of its own: the forward offsets that leave the block (3 faces, + 6 edges at
//                  18, + 4 corners at 26), the neighbour block through the map's hash, lock-free unions on the global parents
//   k_seg_count    every member flattens to its root and counts into it (one atomic per wave and root)
//   k_seg_flag     roots -> kept or not by size, the statistics; an exclusive scan of the flags (hipcub) numbers the kept roots
//   (the host's one wait: the counts size the result)
//   k_seg_heads    per kept root its label, size and representative; bounding box, sums and stamp initialised
//   k_seg_reduce   every kept member into its component's bounding box, sums and stamp; with a voxel list also its sort key
//   hipcub         exclusive scan of the sizes = `first`; radix sort of the {component id, node id} keys = the order of the list
//   k_seg_emit     the sorted keys -> global voxel index and component id
// A node id is rank * vps^3 + linear index (uint32: the host holds blocks * vps^3 below 2^31), so ascending node ids are A.19's voxel
// order; a union always hangs the larger root under the smaller one (ufUnion, khr_device.h), so a component's root is its
// representative.  Every loop is bounded by the data: a find walks a chain of strictly decreasing ids, a union retries only after
// another thread's successful hook, and no workgroup waits for another.  Inside k_seg_seams and k_seg_count the parent array is
// touched through device-scope atomics only (ufLoad / atomicMin / atomicCAS): workgroups on different XCDs never read each other's
// plain stores within a launch.
// Scratch: 12 bytes per voxel of the blocks the scratch is sized for (parent, count, number) -- the live blocks where the host
// knows their number without a wait, else the pool's capacity -- plus 8 bytes per block; the result takes 88 bytes per kept
// component and, with the voxel list, 16 + 16 (sort keys, twice) bytes per listed voxel.
#pragma once
#include "khr_device.h"
#include "khr_kernels_checkpoint.h"
#include "khr_kernels_objects.h"

namespace khr {

constexpr uint32_t kSegNone = 0xffffffffu;  // parent word of a voxel that is no member; rank of an absent block

// 64-bit counters of one call
enum SegCounter : int {
  SC_MEMBERS = 0,  // member voxels
  SC_ALL,          // components before the size filter
  SC_SMALL,        // ... below min_voxels
  SC_LARGE,        // ... above max_voxels
  SC_KEPT,         // ... kept
  SC_VOXELS,       // members of kept components
  SC_ERR,          // kSegErr* bits
  SC_APPEND,       // cursor of the sort-key list (k_seg_reduce)
  SC_COUNT
};
constexpr unsigned long long kSegErrBound = 1ull;  // more live blocks than the scratch was sized for

// membership (A.19): the request's thresholds, flag masks and label list
struct SegMember {
  float min_weight, surface_distance;
  uint32_t flags_require, flags_exclude;
  int32_t n_labels;
  uint32_t labels[64];
};
// adjacency and the size filter
struct SegRule {
  int32_t n_dirs;    // forward offsets of the neighbourhood: 3, 9 or 13 leading entries of c_obj_fwd13
  int32_t by_label;  // adjacent members must also carry the same label (0 without semantics: nothing to compare)
  unsigned long long min_voxels, max_voxels;  // inclusive; max = ~0 for unlimited
};
// the live blocks in (x, y, z) order and the tables between a block's rank and its pool slot
struct SegBlocks {
  const uint64_t* keys;    // ckptSortKey, ascending
  const uint32_t* count;   // their number
  uint32_t bound;          // blocks the scratch holds
  uint32_t* rank_of_slot;  // [capacity], valid for live slots
  uint32_t* slot_of_rank;  // [bound]
};

// The result, structure of arrays in one block: byte offsets for m components and n listed voxels (256-byte aligned).
struct SegLayout {
  size_t label, n_voxels, bbox_min, bbox_max, sum, representative, last_observed, first, voxels, voxel_component, bytes;
};
__host__ __device__ inline SegLayout segLayout(size_t m, size_t n) {
  SegLayout L;
  size_t o = 0;
  const auto carve = [&o](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) & ~static_cast<size_t>(255);
    return at;
  };
  L.label = carve(4 * m), L.n_voxels = carve(8 * m), L.bbox_min = carve(12 * m), L.bbox_max = carve(12 * m), L.sum = carve(24 * m);
  L.representative = carve(12 * m), L.last_observed = carve(8 * m), L.first = carve(8 * m), L.voxels = carve(12 * n);
  L.voxel_component = carve(4 * n), L.bytes = o;
  return L;
}

template <int VPS>
__device__ inline void segVoxelOf(uint32_t lin, int* x, int* y, int* z) {
  constexpr int SH = VPS == 16 ? 4 : 3;
  *x = static_cast<int>(lin & (VPS - 1)), *y = static_cast<int>((lin >> SH) & (VPS - 1)), *z = static_cast<int>(lin >> (2 * SH));
}

// One workgroup per live block (grid-stride over the ranks).  LDS: a parent word and a label word per voxel (32 KB at 16^3).
template <int VPS>
__global__ __launch_bounds__(256) void k_seg_local(DevMap m, DevParams p, SegMember M, SegRule R, SegBlocks B, uint32_t* __restrict__ parent,
                                                   uint32_t* __restrict__ cnt, unsigned long long* __restrict__ ctr) {
  constexpr int NV = VPS * VPS * VPS, SH = VPS == 16 ? 4 : 3;
  __shared__ uint32_t s_par[NV];
  __shared__ uint32_t s_lab[NV];
  __shared__ uint32_t s_list[64];
  if (threadIdx.x < 64u) s_list[threadIdx.x] = M.labels[threadIdx.x];
  const uint32_t live = *B.count, n = min(live, B.bound);
  if (live > B.bound && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&ctr[SC_ERR], kSegErrBound);
  uint32_t members = 0;  // (per wave)
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    int bx, by, bz;
    ckptSortKeyIndex(B.keys[r], &bx, &by, &bz);
    const uint32_t slot = htLookup(m, packKey(bx, by, bz));  // (uniform; a listed block is live)
    const bool have = slot != kInvalidSlot && slot < m.capacity;
    const size_t o = static_cast<size_t>(have ? slot : 0u) * NV;
    __syncthreads();  // (the previous block's LDS has been read; s_list is written)
    for (uint32_t lin = threadIdx.x; lin < static_cast<uint32_t>(NV); lin += 256) {
      const uint32_t label = p.with_semantics ? m.sem_label[o + lin] : 0u;
      const uint32_t fl = m.vflags[o + lin] & VOX_PUBLIC_MASK;
      bool mem = have && m.weight[o + lin] >= M.min_weight && m.dist[o + lin] <= M.surface_distance;
      mem = mem && (fl & M.flags_require) == M.flags_require && (fl & M.flags_exclude) == 0u;
      if (M.n_labels > 0) {
        bool listed = false;
        for (int i = 0; i < M.n_labels; ++i) listed = listed || s_list[i] == label;
        mem = mem && listed;
      }
      s_par[lin] = mem ? lin : kSegNone;
      s_lab[lin] = R.by_label ? label : 0u;
      members += static_cast<uint32_t>(__popcll(__ballot(mem)));
    }
    __syncthreads();
    for (uint32_t lin = threadIdx.x; lin < static_cast<uint32_t>(NV); lin += 256) {
      if (ufLoad(s_par, lin) == kSegNone) continue;
      int x, y, z;
      segVoxelOf<VPS>(lin, &x, &y, &z);
      const uint32_t label = s_lab[lin];
      for (int k = 0; k < R.n_dirs; ++k) {
        const int nx = x + c_obj_fwd13[k][0], ny = y + c_obj_fwd13[k][1], nz = z + c_obj_fwd13[k][2];
        if (((nx | ny | nz) & ~(VPS - 1)) != 0) continue;  // leaves the block: k_seg_seams
        const uint32_t nl = static_cast<uint32_t>(nx | (ny << SH) | (nz << (2 * SH)));
        if (ufLoad(s_par, nl) != kSegNone && s_lab[nl] == label) ufUnion(s_par, lin, nl);
      }
    }
    __syncthreads();
    const uint32_t base = r * static_cast<uint32_t>(NV);
    for (uint32_t lin = threadIdx.x; lin < static_cast<uint32_t>(NV); lin += 256) {
      const bool mem = s_par[lin] != kSegNone;
      parent[base + lin] = mem ? base + ufFind(static_cast<const uint32_t*>(s_par), lin) : kSegNone;
      cnt[base + lin] = 0u;
    }
    if (threadIdx.x == 0) {
      B.slot_of_rank[r] = have ? slot : kInvalidSlot;
      if (have) B.rank_of_slot[slot] = r;
    }
  }
  if ((threadIdx.x & 63u) == 0 && members) atomicAdd(&ctr[SC_MEMBERS], static_cast<unsigned long long>(members));
}

// One workgroup per live block: its boundary voxels against the forward neighbours in other blocks.  Both voxels of a pair see
// each other, so the forward half of the offsets covers every pair once.
template <int VPS>
__global__ __launch_bounds__(256) void k_seg_seams(DevMap m, DevParams p, SegRule R, SegBlocks B, uint32_t* parent) {
  constexpr int NV = VPS * VPS * VPS, SH = VPS == 16 ? 4 : 3;
  __shared__ uint32_t s_rank[27], s_slot[27];
  const uint32_t n = min(*B.count, B.bound);
  const bool labels = R.by_label != 0 && p.with_semantics != 0;
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    int bx, by, bz;
    ckptSortKeyIndex(B.keys[r], &bx, &by, &bz);
    const uint32_t slot = B.slot_of_rank[r];
    __syncthreads();  // (the previous block's table has been read)
    if (threadIdx.x < 27u) {
      const int t = static_cast<int>(threadIdx.x);
      const int cx = bx + t % 3 - 1, cy = by + (t / 3) % 3 - 1, cz = bz + t / 9 - 1;
      uint32_t nr = kSegNone, ns = kInvalidSlot;
      const int lim = 1 << 20;  // (outside the key range packKey would wrap: no block lives there)
      if (cx >= -lim && cx < lim && cy >= -lim && cy < lim && cz >= -lim && cz < lim) {
        ns = htLookup(m, packKey(cx, cy, cz));
        if (ns != kInvalidSlot && ns < m.capacity) {
          const uint32_t q = B.rank_of_slot[ns];
          if (q < n && B.slot_of_rank[q] == ns) nr = q;  // (a block in the hash is in the list; anything else is no neighbour)
        }
      }
      s_rank[t] = nr, s_slot[t] = ns;
    }
    __syncthreads();
    if (slot == kInvalidSlot) continue;  // (uniform)
    const uint32_t base = r * static_cast<uint32_t>(NV);
    const size_t o = static_cast<size_t>(slot) * NV;
    for (uint32_t lin = threadIdx.x; lin < static_cast<uint32_t>(NV); lin += 256) {
      int x, y, z;
      segVoxelOf<VPS>(lin, &x, &y, &z);
      if (x > 0 && x < VPS - 1 && y > 0 && y < VPS - 1 && z > 0 && z < VPS - 1) continue;  // no offset leaves the block
      if (ufLoad(parent, base + lin) == kSegNone) continue;
      const uint32_t label = labels ? m.sem_label[o + lin] : 0u;
      for (int k = 0; k < R.n_dirs; ++k) {
        const int nx = x + c_obj_fwd13[k][0], ny = y + c_obj_fwd13[k][1], nz = z + c_obj_fwd13[k][2];
        const int ox = nx >> SH, oy = ny >> SH, oz = nz >> SH;  // -1, 0, 1: the block the neighbour lies in
        if ((ox | oy | oz) == 0) continue;                      // inside the block: k_seg_local
        const int t = (ox + 1) + 3 * (oy + 1) + 9 * (oz + 1);
        const uint32_t nr = s_rank[t];
        if (nr == kSegNone) continue;
        const uint32_t nl = static_cast<uint32_t>((nx & (VPS - 1)) | ((ny & (VPS - 1)) << SH) | ((nz & (VPS - 1)) << (2 * SH)));
        const uint32_t other = nr * static_cast<uint32_t>(NV) + nl;
        if (ufLoad(parent, other) == kSegNone) continue;
        if (labels && m.sem_label[static_cast<size_t>(s_slot[t]) * NV + nl] != label) continue;
        ufUnion(parent, base + lin, other);
      }
    }
  }
}

// Every member flattens to its root and counts into it.  The lanes of a wave that share a root add once: the voxels of a block
// mostly do.  At most 64 rounds per wave (one per distinct root).
__global__ __launch_bounds__(256) void k_seg_count(SegBlocks B, uint32_t nv, uint32_t* parent, uint32_t* cnt) {
  const uint64_t total = static_cast<uint64_t>(min(*B.count, B.bound)) * nv;
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t at = (static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u)); at < total; at += static_cast<uint64_t>(gridDim.x) * 256u) {  // (uniform per wave)
    const uint64_t i64 = at + lane;
    const uint32_t i = static_cast<uint32_t>(i64);
    uint32_t root = kSegNone;
    if (i64 < total) {
      const uint32_t par = ufLoad(parent, i);
      if (par != kSegNone) {
        root = ufFind(parent, i);
        if (root != par) atomicMin(parent + i, root);
      }
    }
    unsigned long long todo = __ballot(root != kSegNone);
    while (todo) {
      const int leader = __ffsll(static_cast<long long>(todo)) - 1;
      const uint32_t r0 = __shfl(root, leader);
      const unsigned long long same = __ballot(root == r0);
      if (lane == static_cast<uint32_t>(leader)) atomicAdd(cnt + r0, static_cast<uint32_t>(__popcll(same)));
      todo &= ~same;
    }
  }
}

__device__ inline bool segKept(unsigned long long n, const SegRule& R) { return n >= R.min_voxels && n <= R.max_voxels; }

// number[i] = 1 for a kept root, else 0, over the whole scratch (the scan that follows runs over `bound` blocks and one closing
// element: the host does not know the live count yet); the statistics of the filter.
__global__ __launch_bounds__(256) void k_seg_flag(SegBlocks B, uint32_t nv, SegRule R, const uint32_t* __restrict__ parent,
                                                  const uint32_t* __restrict__ cnt, uint32_t* __restrict__ number, unsigned long long* __restrict__ ctr) {
  const uint64_t total = static_cast<uint64_t>(min(*B.count, B.bound)) * nv, all = static_cast<uint64_t>(B.bound) * nv + 1u;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t n_all = 0, n_small = 0, n_large = 0, n_kept = 0;
  unsigned long long n_vox = 0;
  for (uint64_t at = (static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u)); at < all; at += static_cast<uint64_t>(gridDim.x) * 256u) {
    const uint64_t i = at + lane;
    const bool root = i < total && parent[i] == static_cast<uint32_t>(i);
    const uint32_t c = root ? cnt[i] : 0u;
    const bool small = root && c < R.min_voxels, large = root && c > R.max_voxels, kept = root && !small && !large;
    if (i < all) number[i] = kept ? 1u : 0u;
    n_all += static_cast<uint32_t>(__popcll(__ballot(root)));
    n_small += static_cast<uint32_t>(__popcll(__ballot(small)));
    n_large += static_cast<uint32_t>(__popcll(__ballot(large)));
    n_kept += static_cast<uint32_t>(__popcll(__ballot(kept)));
    unsigned long long v = kept ? c : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    n_vox += v;
  }
  if (lane == 0) {
    if (n_all) atomicAdd(&ctr[SC_ALL], static_cast<unsigned long long>(n_all));
    if (n_small) atomicAdd(&ctr[SC_SMALL], static_cast<unsigned long long>(n_small));
    if (n_large) atomicAdd(&ctr[SC_LARGE], static_cast<unsigned long long>(n_large));
    if (n_kept) atomicAdd(&ctr[SC_KEPT], static_cast<unsigned long long>(n_kept));
    if (n_vox) atomicAdd(&ctr[SC_VOXELS], n_vox);
  }
}

// Per kept root (number[] now holds the exclusive scan: the component's id - 1): label, size, representative; the accumulators of
// k_seg_reduce initialised.
template <int VPS>
__global__ __launch_bounds__(256) void k_seg_heads(DevMap m, DevParams p, SegRule R, SegBlocks B, const uint32_t* __restrict__ parent,
                                                   const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ number, uint32_t n_components,
                                                   uint64_t n_listed, uint8_t* __restrict__ out) {
  constexpr int NV = VPS * VPS * VPS;
  const uint64_t total = static_cast<uint64_t>(min(*B.count, B.bound)) * NV;
  const SegLayout L = segLayout(n_components, n_listed);
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < total; i += static_cast<uint64_t>(gridDim.x) * 256u) {
    if (parent[i] != static_cast<uint32_t>(i)) continue;
    const uint32_t size = cnt[i];
    if (!segKept(size, R)) continue;
    const size_t c = number[i];
    if (c >= n_components) continue;  // (cannot happen: no write beyond the arrays)
    const uint32_t r = static_cast<uint32_t>(i / NV), lin = static_cast<uint32_t>(i % NV), slot = B.slot_of_rank[r];
    int bx, by, bz, x, y, z;
    ckptSortKeyIndex(B.keys[r], &bx, &by, &bz);
    segVoxelOf<VPS>(lin, &x, &y, &z);
    reinterpret_cast<int32_t*>(out + L.label)[c] = p.with_semantics ? static_cast<int32_t>(m.sem_label[static_cast<size_t>(slot) * NV + lin]) : 0;
    reinterpret_cast<uint64_t*>(out + L.n_voxels)[c] = size;
    int32_t* const rep = reinterpret_cast<int32_t*>(out + L.representative) + 3 * c;
    int32_t* const lo = reinterpret_cast<int32_t*>(out + L.bbox_min) + 3 * c;
    int32_t* const hi = reinterpret_cast<int32_t*>(out + L.bbox_max) + 3 * c;
    unsigned long long* const sum = reinterpret_cast<unsigned long long*>(out + L.sum) + 3 * c;
    rep[0] = bx * VPS + x, rep[1] = by * VPS + y, rep[2] = bz * VPS + z;
    lo[0] = lo[1] = lo[2] = INT32_MAX;
    hi[0] = hi[1] = hi[2] = INT32_MIN;
    sum[0] = sum[1] = sum[2] = 0ull;
    reinterpret_cast<uint64_t*>(out + L.last_observed)[c] = 0ull;
  }
}

// atomicMin / atomicMax that look first: a bound only ever moves one way, so a value read earlier (however stale) that the new one
// does not beat is reason enough to skip the atomic -- the members of a large component all aim at the same few words, and most
// of them do not move its box
template <typename T>
__device__ inline void segLower(T* p, T v) {
  if (v < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, v);
}
template <typename T>
__device__ inline void segRaise(T* p, T v) {
  if (v > __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMax(p, v);
}

// Every member of a kept component into its component's bounding box, sums and latest stamp (non-returning atomics: once per wave
// where the wave's kept members share a component, the common case; per lane otherwise).  LIST: also the member's sort key
// {component id, node id} into the key list, in the order the waves arrive (the sort orders it).
template <int VPS, bool LIST>
__global__ __launch_bounds__(256) void k_seg_reduce(DevMap m, DevParams p, SegRule R, SegBlocks B, const uint32_t* __restrict__ parent,
                                                    const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ number, uint32_t n_components,
                                                    uint64_t n_listed, uint8_t* __restrict__ out, uint64_t* __restrict__ sort_keys,
                                                    unsigned long long* __restrict__ ctr) {
  constexpr int NV = VPS * VPS * VPS;
  const uint64_t total = static_cast<uint64_t>(min(*B.count, B.bound)) * NV;
  const SegLayout L = segLayout(n_components, n_listed);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t at = (static_cast<uint64_t>(blockIdx.x) * 256u + (threadIdx.x & ~63u)); at < total; at += static_cast<uint64_t>(gridDim.x) * 256u) {  // (uniform per wave)
    const uint64_t i = at + lane;
    bool kept = false;
    uint32_t c = 0u;
    if (i < total) {
      const uint32_t root = parent[i];
      if (root != kSegNone && segKept(cnt[root], R)) {
        c = number[root];
        kept = c < n_components;
      }
    }
    const unsigned long long mask = __ballot(kept);
    if (mask == 0ull) continue;  // (uniform)
    int g[3] = {0, 0, 0};
    unsigned long long stamp = 0ull;
    if (kept) {
      const uint32_t r = static_cast<uint32_t>(i / NV), lin = static_cast<uint32_t>(i % NV);
      int bx, by, bz, x, y, z;
      ckptSortKeyIndex(B.keys[r], &bx, &by, &bz);
      segVoxelOf<VPS>(lin, &x, &y, &z);
      g[0] = bx * VPS + x, g[1] = by * VPS + y, g[2] = bz * VPS + z;
      if (p.with_tracking) stamp = lastObserved(m, B.slot_of_rank[r], lin, NV);
    }
    if (LIST) {
      const uint32_t below = static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
      const int leader = __ffsll(static_cast<long long>(mask)) - 1;
      unsigned long long first = 0ull;
      if (lane == static_cast<uint32_t>(leader)) first = atomicAdd(&ctr[SC_APPEND], static_cast<unsigned long long>(__popcll(mask)));
      first = __shfl(first, leader);
      if (kept && first + below < n_listed) sort_keys[first + below] = (static_cast<uint64_t>(c + 1u) << 32) | static_cast<uint32_t>(i);
    }
    int32_t* const lo = reinterpret_cast<int32_t*>(out + L.bbox_min);
    int32_t* const hi = reinterpret_cast<int32_t*>(out + L.bbox_max);
    unsigned long long* const sum = reinterpret_cast<unsigned long long*>(out + L.sum);
    unsigned long long* const last = reinterpret_cast<unsigned long long*>(out + L.last_observed);
    const uint32_t c0 = __shfl(c, __ffsll(static_cast<long long>(mask)) - 1);
    if (__ballot(kept && c != c0) == 0ull) {  // one component in this wave (uniform): reduce, then one lane adds
      int mn[3], mx[3];
      long long sm[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = kept ? g[a] : INT32_MAX, mx[a] = kept ? g[a] : INT32_MIN, sm[a] = kept ? g[a] : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
          mn[a] = min(mn[a], __shfl_xor(mn[a], d));
          mx[a] = max(mx[a], __shfl_xor(mx[a], d));
          sm[a] += __shfl_xor(sm[a], d);
        }
      }
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long s2 = __shfl_xor(stamp, d);
        stamp = s2 > stamp ? s2 : stamp;
      }
      if (lane == 0) {
        const size_t q = c0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          segLower(lo + 3 * q + a, mn[a]);
          segRaise(hi + 3 * q + a, mx[a]);
          atomicAdd(sum + 3 * q + a, static_cast<unsigned long long>(sm[a]));
        }
        segRaise(last + q, stamp);
      }
    } else if (kept) {
      const size_t q = c;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        segLower(lo + 3 * q + a, g[a]);
        segRaise(hi + 3 * q + a, g[a]);
        atomicAdd(sum + 3 * q + a, static_cast<unsigned long long>(static_cast<long long>(g[a])));
      }
      segRaise(last + q, stamp);
    }
  }
}

// the sorted keys -> the voxel list: ascending component id, ascending node id inside a component
template <int VPS>
__global__ __launch_bounds__(256) void k_seg_emit(const uint64_t* __restrict__ block_keys, const uint64_t* __restrict__ sorted, uint32_t n_components,
                                                  uint64_t n_listed, uint32_t n_blocks, uint8_t* __restrict__ out) {
  constexpr int NV = VPS * VPS * VPS;
  const SegLayout L = segLayout(n_components, n_listed);
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n_listed; i += static_cast<uint64_t>(gridDim.x) * 256u) {
    const uint64_t k = sorted[i];
    const uint32_t node = static_cast<uint32_t>(k), r = min(node / NV, n_blocks - 1u), lin = node % NV;
    int bx, by, bz, x, y, z;
    ckptSortKeyIndex(block_keys[r], &bx, &by, &bz);
    segVoxelOf<VPS>(lin, &x, &y, &z);
    int32_t* const v = reinterpret_cast<int32_t*>(out + L.voxels) + 3 * i;
    v[0] = bx * VPS + x, v[1] = by * VPS + y, v[2] = bz * VPS + z;
    reinterpret_cast<uint32_t*>(out + L.voxel_component)[i] = static_cast<uint32_t>(k >> 32);
  }
}

}  // namespace khr
