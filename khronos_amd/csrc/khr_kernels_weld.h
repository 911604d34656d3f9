// khr_kernels_weld.h — device side of khr_weld_mesh (include/khronos_amd.h, ASSUMPTIONS.md A.16): the triangle soup of the last
// khr_generate_mesh as an indexed mesh, one vertex per cell of a grid of `resolution`.  gfx950 only, wave64.
//   soup order:  k_ckpt_select -> bitonic sort of khr_kernels_slice.h (the live blocks in (x, y, z) order) -> k_weld_block_counts ->
//                exclusive scan (hipcub): the soup index of a block's first vertex, the soup's length in the scan's last word
//   insert:      k_weld_clear -> k_weld_insert: cell key -> open-addressing table (64-bit CAS), atomicMin of the soup index into the
//                slot's value: the cell's representative = its least soup index
//   resolve:     k_weld_resolve (is this vertex its cell's representative) -> exclusive scan: the welded index ->
//                k_weld_vertices (the representatives' attributes as SoA, soup_to_vertex)
//   faces:       k_weld_face_flags -> exclusive scan -> k_weld_faces (the kept faces; publishes the counts)
// The host knows an upper bound of the soup (n_cap: the extent of the vertex buffer, vertices of archived blocks included) and
// sizes buffers and grids from it; the soup's length itself stays on the device until the counts come back.
#pragma once
#include "khr_device.h"
#include "khr_kernels_aux.h"
#include "khr_kernels_checkpoint.h"

namespace khr {

// error bits of a weld (head[0]): a vertex outside the key range (or not finite); the descriptors do not fit the buffers
constexpr uint32_t kWeldErrRange = 1u, kWeldErrBounds = 2u;
constexpr int kWeldHeadWords = 8;  // head: {error bits, n_soup, n_vertices, n_faces, ...}

struct WeldWork {
  uint32_t* blk_count;  // [capacity + 1] vertices of the i-th block in sorted order (0 behind the last one)
  uint32_t* blk_base;   // [capacity + 1] exclusive scan of blk_count; [capacity] = soup length
  uint32_t* blk_off;    // [capacity] the block's first vertex in the vertex buffer
  uint32_t* src;        // [n_cap] soup index -> position in the vertex buffer
  uint32_t* hslot;      // [n_cap] soup index -> table slot of its cell
  uint32_t* is_rep;     // [n_cap + 1]
  uint32_t* widx;       // [n_cap + 1] exclusive scan of is_rep; [n_cap] = welded vertices
  uint32_t* keep;       // [n_cap / 3 + 1]
  uint32_t* fidx;       // [n_cap / 3 + 1] exclusive scan of keep; [n_cap / 3] = kept faces
  uint64_t* keys;       // table: kEmptyKey = free
  uint32_t* vals;       // least soup index of the cell (0xffffffff = none yet)
  uint32_t mask;
  uint32_t* head;       // [kWeldHeadWords]
  uint32_t n_cap;         // the host's upper bound of the soup's length
  uint32_t max_vertices;  // extent of the vertex buffers
};

// the result, structure of arrays (the context owns it)
struct WeldOut {
  float* points;      // [vertex][3]
  uint32_t* colors;   // rgba8
  uint32_t* labels;
  uint64_t* stamps;   // first_seen == stamps (ASSUMPTIONS.md A.5)
  uint32_t* faces;    // [face][3]
  uint32_t* soup_to_vertex;  // [soup vertex]
};

// the soup's length, or 0 when the weld has failed (the kernels then do nothing)
__device__ inline uint32_t weldSoup(const WeldWork& w, uint32_t capacity) {
  const uint32_t n = w.blk_base[capacity];
  return (n > w.n_cap || w.head[0] != 0u) ? 0u : n;
}

// cell key of a vertex at resolution r (A.16): floorf of the IEEE float32 quotient per axis, 3 x 21 bits
__device__ inline bool weldKey(float x, float y, float z, float r, uint64_t* key) {
  const float cx = floorf(__fdiv_rn(x, r)), cy = floorf(__fdiv_rn(y, r)), cz = floorf(__fdiv_rn(z, r));
  const float lo = -1048576.f, hi = 1048576.f;
  const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && cx >= lo && cx < hi && cy >= lo && cy < hi && cz >= lo && cz < hi;
  *key = ok ? packKey(static_cast<int>(cx), static_cast<int>(cy), static_cast<int>(cz)) : kEmptyKey;
  return ok;
}

__global__ __launch_bounds__(256) void k_weld_clear(WeldWork w) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x, t0 = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t n = static_cast<size_t>(w.mask) + 1;  // (a power of two >= 4)
  ulonglong2* k2 = reinterpret_cast<ulonglong2*>(w.keys);
  for (size_t i = t0; i < n / 2; i += stride) k2[i] = make_ulonglong2(kEmptyKey, kEmptyKey);
  uint4* v4 = reinterpret_cast<uint4*>(w.vals);
  for (size_t i = t0; i < n / 4; i += stride) v4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
  if (t0 < kWeldHeadWords) w.head[t0] = 0u;
}

// the i-th key of the sorted block list -> its vertex count and its place in the vertex buffer
__global__ __launch_bounds__(256) void k_weld_block_counts(DevMap m, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ count, WeldWork w) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > m.capacity) return;
  const uint32_t n = min(*count, m.capacity);
  uint32_t cnt = 0u, off = 0u;
  if (i < n) {
    int x, y, z;
    ckptSortKeyIndex(keys[i], &x, &y, &z);
    const uint32_t slot = htLookup(m, packKey(x, y, z));
    if (slot < m.capacity && (m.blk_flags[slot] & BLK_LIVE)) {
      const MeshDesc d = m.mesh_desc[slot];
      if (static_cast<uint64_t>(d.offset) + d.count <= w.max_vertices) cnt = d.count, off = d.offset;
      else atomicOr(&w.head[0], kWeldErrBounds);  // (a descriptor beyond the buffer: not a mesh khr_generate_mesh left)
    }
  }
  w.blk_count[i] = cnt;
  if (i < m.capacity) w.blk_off[i] = off;
}

// the slot of `key`, claimed if the key is new.  The table has at least twice as many slots as keys: a free one is found.
__device__ inline uint32_t weldInsert(const WeldWork& w, uint64_t key) {
  uint32_t h = hashKey(key) & w.mask;
  for (uint32_t probes = 0; probes <= w.mask; ++probes) {
    const uint64_t k = w.keys[h];  // (a key never changes once it is written: seeing it here is final, seeing "free" is not)
    if (k == key) return h;
    if (k == kEmptyKey) {
      const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(&w.keys[h]), static_cast<unsigned long long>(kEmptyKey),
                                                static_cast<unsigned long long>(key));
      if (prev == kEmptyKey || prev == key) return h;
    }
    h = (h + 1) & w.mask;
  }
  return kInvalidSlot;
}

// One lane per soup vertex.  MERGE: consecutive soup vertices often share a cell (the corners of a small triangle, the cubes round
// an edge), so the first lane of every run of equal keys in the wave inserts for the run -- soup indices ascend with the lane,
// its own index is the run's least -- and hands the slot to the others.  !MERGE: every lane inserts (the A/B of DESIGN.md section 4).
template <bool MERGE>
__global__ __launch_bounds__(256) void k_weld_insert(DevMap m, MeshBuffers mb, float r, WeldWork w) {
  const uint32_t n_soup = w.blk_base[m.capacity];
  if (n_soup > w.n_cap || (w.head[0] & kWeldErrBounds)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&w.head[0], kWeldErrBounds);
    return;
  }
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool has = i < n_soup;
  uint32_t at = 0u;
  uint64_t key = kEmptyKey;
  bool ok = false;
  if (has) {
    uint32_t lo = 0u, hi = m.capacity;  // the last block whose base is <= i (empty blocks share their successor's base)
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1u) >> 1;
      if (w.blk_base[mid] <= i) lo = mid;
      else hi = mid - 1u;
    }
    at = w.blk_off[lo] + (i - w.blk_base[lo]);
    ok = weldKey(mb.points[3 * static_cast<size_t>(at)], mb.points[3 * static_cast<size_t>(at) + 1], mb.points[3 * static_cast<size_t>(at) + 2], r, &key);
  }
  const unsigned long long bad = __ballot(has && !ok);
  if (bad && laneId() == static_cast<uint32_t>(__ffsll(static_cast<long long>(bad)) - 1)) atomicOr(&w.head[0], kWeldErrRange);
  uint32_t h = kInvalidSlot;
  if (MERGE) {
    const uint32_t lane = laneId();
    const uint32_t klo = static_cast<uint32_t>(key), khi = static_cast<uint32_t>(key >> 32);
    const uint32_t plo = __shfl_up(klo, 1), phi = __shfl_up(khi, 1);
    const unsigned long long hm = __ballot(ok);
    const bool prev_ok = lane > 0u && ((hm >> (lane - 1u)) & 1ull);
    const bool start = ok && !(prev_ok && plo == klo && phi == khi);
    const unsigned long long sm = __ballot(start);
    if (start) {
      h = weldInsert(w, key);
      if (h != kInvalidSlot && w.vals[h] > i) atomicMin(&w.vals[h], i);
    }
    const unsigned long long below = sm & ((2ull << lane) - 1ull);  // run starts at or below this lane
    const int leader = below ? 63 - __clzll(static_cast<long long>(below)) : static_cast<int>(lane);
    h = __shfl(h, leader);
  } else if (ok) {
    h = weldInsert(w, key);
    if (h != kInvalidSlot && w.vals[h] > i) atomicMin(&w.vals[h], i);
  }
  if (has) {
    w.src[i] = at;
    w.hslot[i] = ok ? h : kInvalidSlot;
  }
}

// is_rep over [0, n_cap]: zero behind the soup, so that the scan's last word is the number of welded vertices
__global__ __launch_bounds__(256) void k_weld_resolve(uint32_t capacity, WeldWork w) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > w.n_cap) return;
  const uint32_t n_soup = weldSoup(w, capacity);
  uint32_t rep = 0u;
  if (i < n_soup) {
    const uint32_t h = w.hslot[i];
    rep = (h <= w.mask && w.vals[h] == i) ? 1u : 0u;
  }
  w.is_rep[i] = rep;
}

__global__ __launch_bounds__(256) void k_weld_vertices(uint32_t capacity, MeshBuffers mb, WeldWork w, WeldOut o) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n_soup = weldSoup(w, capacity);
  if (i >= n_soup) return;
  const uint32_t h = w.hslot[i];
  if (h > w.mask) return;
  const uint32_t rep = w.vals[h];
  if (rep >= n_soup) return;
  const uint32_t j = w.widx[rep];
  o.soup_to_vertex[i] = j;
  if (rep == i) {
    const size_t at = w.src[i];
    o.points[3 * static_cast<size_t>(j)] = mb.points[3 * at];
    o.points[3 * static_cast<size_t>(j) + 1] = mb.points[3 * at + 1];
    o.points[3 * static_cast<size_t>(j) + 2] = mb.points[3 * at + 2];
    o.colors[j] = mb.colors[at];
    o.labels[j] = mb.labels[at];
    o.stamps[j] = mb.stamps[at];
  }
}

// keep over [0, n_cap / 3]: a face whose three welded indices differ; zero behind the soup's faces
__global__ __launch_bounds__(256) void k_weld_face_flags(uint32_t capacity, WeldWork w, WeldOut o) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f > w.n_cap / 3u) return;
  const uint32_t n_faces = weldSoup(w, capacity) / 3u;
  uint32_t keep = 0u;
  if (f < n_faces) {
    const uint32_t a = o.soup_to_vertex[3 * static_cast<size_t>(f)], b = o.soup_to_vertex[3 * static_cast<size_t>(f) + 1],
                   c = o.soup_to_vertex[3 * static_cast<size_t>(f) + 2];
    keep = (a != b && b != c && a != c) ? 1u : 0u;
  }
  w.keep[f] = keep;
}

__global__ __launch_bounds__(256) void k_weld_faces(uint32_t capacity, WeldWork w, WeldOut o) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n_soup = weldSoup(w, capacity);
  if (f == 0u) {  // the counts (zero when the weld has failed; the error bits say why)
    w.head[1] = n_soup;
    w.head[2] = n_soup ? w.widx[w.n_cap] : 0u;
    w.head[3] = n_soup ? w.fidx[w.n_cap / 3u] : 0u;
  }
  if (f >= n_soup / 3u || !w.keep[f]) return;
  const size_t g = w.fidx[f];
  o.faces[3 * g] = o.soup_to_vertex[3 * static_cast<size_t>(f)];
  o.faces[3 * g + 1] = o.soup_to_vertex[3 * static_cast<size_t>(f) + 1];
  o.faces[3 * g + 2] = o.soup_to_vertex[3 * static_cast<size_t>(f) + 2];
}

}  // namespace khr
