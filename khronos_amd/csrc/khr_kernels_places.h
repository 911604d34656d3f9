// khr_kernels_places.h — places and their links from the generalized Voronoi cells of a box (khr_places_graph / khr_places_graph_from;
// ASSUMPTIONS.md A.21).  Reads a distance / d2 / basis / site field, writes buffers of its own.  gfx950, wave64.  Integers and bit
// copies throughout.
//
// A place never leaves its bucket (compression^3 <= 4096 cells), so the labelling needs no seam pass:
//   k_pl_label     one workgroup per TILE of T^3 whole buckets, E = T * compression <= 16 cells along an axis (T = 1 from compression
//                  9 on: one workgroup per bucket; smaller buckets share a workgroup so that compression 1 is not a launch per
//                  cell).  Tiles are anchored in the world like the buckets, so partial tiles occur at both ends of every axis.
//                  LDS: a parent word per cell (16 KB), the flattened root as uint16 (8 KB), and per place of the tile (at most
//                  kPlSlots: the host picks T so) the centre key and the packed count / coordinate sums (8 KB each) -- 40 KB, three
//                  workgroups per CU.  Membership -> union-find with atomic-min hooking over the 13 forward offsets that stay in
//                  the bucket -> flatten -> slots -> one ds_max_u64 and one ds_add_u64 per member -> one global write per place,
//                  at its representative's cell.  A tile without members leaves after the first barrier.
//   hipcub scan    of the root flags over lin: the places in ascending order of their representatives
//   k_pl_pairs<0>  per member the forward neighbours that belong to another place: a count per cell; scanned
//   (host wait 1: members, places, adjacent pairs -- they size the work lists)
//   k_pl_pairs<1>  the pairs: key = min place << 32 | max place, value = min d2; hipcub radix sort by key
//   k_pl_edge_heads / scan / k_pl_edge_reduce   equal keys -> one edge: (max, count) by atomics on the edge's row
//   k_pl_comp_*    union-find over the places through the unique edges (ufUnion of khr_device.h: the larger root hangs under the
//                  smaller, so a component's root is its least place), flatten, sizes, keep flags; scans renumber places,
//                  components and edges monotonically, so every order survives the filter
//   (host wait 2: the kept counts size the result)
//   k_pl_finish_cells / k_pl_finish_edges   the dense place ids, one record per kept place, the kept edges and the degrees
// Every loop is bounded by the data: a find walks strictly decreasing ids, a union retries only after another thread's hook.
#pragma once
#include "khr_device.h"
#include "khr_map_read.h"
#include "khr_kernels_objects.h"

namespace khr {

constexpr uint32_t kPlNone = 0xffffffffu;  // label of a cell that is no member
constexpr int kPlMaxEdge = 16;             // cells along a tile's axis at most
constexpr int kPlTileCells = kPlMaxEdge * kPlMaxEdge * kPlMaxEdge;
constexpr int kPlSlots = 1024;             // places of one tile at most
constexpr int32_t kPlD2Limit = 1 << 30;    // a member's d2 lies below

enum PlCounter : int { PLC_MEMBERS = 0, PLC_PLACES_ALL, PLC_PAIRS, PLC_EDGES_ALL, PLC_COMPS_ALL, PLC_PLACES, PLC_EDGES, PLC_COMPS, PLC_ERR, PLC_COUNT };  // PLC_ERR: tiles whose places outgrew kPlSlots

// buckets of one tile along an axis: the most that keeps the tile within 16 cells and its places within kPlSlots (a bucket holds at
// most ceil(compression / 2)^3 places: one cell of each is an independent set of the 26-neighbourhood)
__host__ __device__ inline int plTileBuckets(int compression) {
  const int half = (compression + 1) / 2;
  int t = kPlMaxEdge / compression;
  while (t > 1 && t * t * t * half * half * half > kPlSlots) --t;
  return t;
}
__host__ __device__ inline int plFloorDiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

struct PlField {
  int ox, oy, oz;  // first cell
  int nx, ny, nz;
  const float* distance;  // the input field, x + nx * (y + ny * z)
  const int32_t* d2;
  const uint8_t* basis;
  const int32_t* site;
  int min_basis;
  float min_node_distance;
  int compression, edge;   // cells of a bucket / of a tile along an axis
  int tx0, ty0, tz0;       // the first tile's index per axis (world cell / edge, rounded down)
  int ntx, nty, ntz;
  uint32_t* label;         // [n] the representative's lin, kPlNone for no member (preset)
  uint32_t* number;        // [n + 1] root flags (preset 0), scanned in place: the place of a representative
  uint32_t* pair_count;    // [n + 1] pairs a cell emits, scanned in place
  uint64_t* rec_key;       // [n] at a representative: d2 << 32 | ~lin of the centre
  uint64_t* rec_acc;       // [n] at a representative: tile-local sums x | y << 16 | z << 32, cells << 48
  unsigned long long* ctr; // PlCounter words
};

__device__ inline bool plIsMember(const PlField& f, size_t lin) {
  const int32_t v = f.d2[lin];
  return static_cast<int>(f.basis[lin]) >= f.min_basis && f.distance[lin] >= f.min_node_distance && v >= 0 && v < kPlD2Limit;
}

// find with path halving and union with atomic-min hooking on LDS words.  A hook that finds `a` no longer a root has still lowered
// a's parent to min(old, b); old and b are then united, and max(a, b) falls with every round.
__device__ inline void plUnion(uint32_t* parent, uint32_t a, uint32_t b) {
  a = ufFind(parent, a);
  b = ufFind(parent, b);
  while (a != b) {
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(parent + a, b);
    if (old == a) return;
    a = ufFind(parent, old);
    b = ufFind(parent, b);
  }
}

__global__ __launch_bounds__(256) void k_pl_label(PlField f) {
  __shared__ uint32_t s_par[kPlTileCells];
  __shared__ uint16_t s_root[kPlTileCells];
  __shared__ unsigned long long s_key[kPlSlots];
  __shared__ unsigned long long s_acc[kPlSlots];
  __shared__ uint32_t s_n[2];  // members, places
  const int E = f.edge, C = f.compression, cells = E * E * E;
  const int tid = static_cast<int>(threadIdx.x);
  const int t = static_cast<int>(blockIdx.x);
  const int tx = t % f.ntx, ty = (t / f.ntx) % f.nty, tz = t / (f.ntx * f.nty);
  // the tile's first cell, box-local (may be negative: a partial tile)
  const int bx = (f.tx0 + tx) * E - f.ox, by = (f.ty0 + ty) * E - f.oy, bz = (f.tz0 + tz) * E - f.oz;
  if (tid < 2) s_n[tid] = 0u;
  __syncthreads();
  uint32_t mine = 0u;
  for (int l = tid; l < cells; l += 256) {
    const int x = bx + l % E, y = by + (l / E) % E, z = bz + l / (E * E);
    bool mem = x >= 0 && x < f.nx && y >= 0 && y < f.ny && z >= 0 && z < f.nz;
    if (mem) mem = plIsMember(f, static_cast<size_t>(x) + static_cast<size_t>(f.nx) * (static_cast<size_t>(y) + static_cast<size_t>(f.ny) * static_cast<size_t>(z)));
    s_par[l] = mem ? static_cast<uint32_t>(l) : kPlNone;
    mine += mem ? 1u : 0u;
  }
  if (mine) atomicAdd(&s_n[0], mine);
  __syncthreads();
  const uint32_t members = s_n[0];
  if (members == 0u) return;  // (uniform)
  if (C > 1) {
    for (int l = tid; l < cells; l += 256) {
      if (ufLoad(s_par, l) == kPlNone) continue;
      const int lx = l % E, ly = (l / E) % E, lz = l / (E * E);
      for (int k = 0; k < 13; ++k) {
        const int qx = lx + c_obj_fwd13[k][0], qy = ly + c_obj_fwd13[k][1], qz = lz + c_obj_fwd13[k][2];
        if (qx < 0 || qx >= E || qy < 0 || qy >= E || qz >= E) continue;
        if (qx / C != lx / C || qy / C != ly / C || qz / C != lz / C) continue;  // another bucket
        const uint32_t q = static_cast<uint32_t>(qx + E * (qy + E * qz));
        if (ufLoad(s_par, q) != kPlNone) plUnion(s_par, static_cast<uint32_t>(l), q);
      }
    }
    __syncthreads();
  }
  // flatten (reads only), then the parent word of a root becomes its slot
  for (int l = tid; l < cells; l += 256)
    if (s_par[l] != kPlNone) s_root[l] = static_cast<uint16_t>(ufFind(static_cast<const uint32_t*>(s_par), static_cast<uint32_t>(l)));
  __syncthreads();
  for (int l = tid; l < cells; l += 256) {
    if (s_par[l] == kPlNone || s_root[l] != static_cast<uint16_t>(l)) continue;
    const uint32_t slot = atomicAdd(&s_n[1], 1u);
    s_par[l] = slot;
    if (slot < static_cast<uint32_t>(kPlSlots)) s_key[slot] = 0ull, s_acc[slot] = 0ull;
  }
  __syncthreads();
  const uint32_t unx = static_cast<uint32_t>(f.nx), uny = static_cast<uint32_t>(f.ny);
  for (int l = tid; l < cells; l += 256) {
    if (s_par[l] == kPlNone) continue;
    const int r = static_cast<int>(s_root[l]);
    const uint32_t slot = s_par[r];
    if (slot >= static_cast<uint32_t>(kPlSlots)) continue;  // (cannot happen: plTileBuckets; counted in PLC_ERR if it does)
    const int lx = l % E, ly = (l / E) % E, lz = l / (E * E);
    const uint32_t lin = static_cast<uint32_t>(bx + lx) + unx * (static_cast<uint32_t>(by + ly) + uny * static_cast<uint32_t>(bz + lz));
    const uint32_t rlin = static_cast<uint32_t>(bx + r % E) + unx * (static_cast<uint32_t>(by + (r / E) % E) + uny * static_cast<uint32_t>(bz + r / (E * E)));
    f.label[lin] = rlin;
    const unsigned long long key = (static_cast<unsigned long long>(static_cast<uint32_t>(f.d2[lin])) << 32) | static_cast<unsigned long long>(0xffffffffu - lin);
    atomicMax(&s_key[slot], key);
    atomicAdd(&s_acc[slot], static_cast<unsigned long long>(lx) | (static_cast<unsigned long long>(ly) << 16) | (static_cast<unsigned long long>(lz) << 32) | (1ull << 48));
  }
  __syncthreads();
  for (int l = tid; l < cells; l += 256) {
    if (s_par[l] == kPlNone || s_root[l] != static_cast<uint16_t>(l)) continue;
    const uint32_t slot = s_par[l];
    if (slot >= static_cast<uint32_t>(kPlSlots)) continue;
    const uint32_t lin = static_cast<uint32_t>(bx + l % E) + unx * (static_cast<uint32_t>(by + (l / E) % E) + uny * static_cast<uint32_t>(bz + l / (E * E)));
    f.number[lin] = 1u;
    f.rec_key[lin] = s_key[slot];
    f.rec_acc[lin] = s_acc[slot];
  }
  if (tid == 0) {
    atomicAdd(&f.ctr[PLC_MEMBERS], static_cast<unsigned long long>(members));
    atomicAdd(&f.ctr[PLC_PLACES_ALL], static_cast<unsigned long long>(s_n[1]));
    if (s_n[1] > static_cast<uint32_t>(kPlSlots)) atomicAdd(&f.ctr[PLC_ERR], 1ull);  // (the host fails the call: nothing is dropped in silence)
  }
}

// One lane per cell.  EMIT 0: the number of forward neighbours of a member that belong to another place, per cell; EMIT 1: those
// pairs at the cell's scanned offset.  (All 13 forward offsets raise lin: each unordered pair is seen once, from its lower cell.)
template <int EMIT>
__global__ __launch_bounds__(256) void k_pl_pairs(PlField f, uint64_t* __restrict__ keys, int32_t* __restrict__ vals, uint32_t n_pairs) {
  const long long n = static_cast<long long>(f.nx) * f.ny * f.nz;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + static_cast<long long>(threadIdx.x);
  uint32_t cnt = 0u;
  if (i < n) {
    const uint32_t li = f.label[i];
    if (li != kPlNone) {
      const int x = static_cast<int>(i % f.nx), y = static_cast<int>((i / f.nx) % f.ny), z = static_cast<int>(i / (static_cast<long long>(f.nx) * f.ny));
      const uint32_t at = EMIT ? f.pair_count[i] : 0u;
      const uint32_t pi = EMIT ? f.number[li] : 0u;
      const int32_t di = EMIT ? f.d2[i] : 0;
      for (int k = 0; k < 13; ++k) {
        const int X = x + c_obj_fwd13[k][0], Y = y + c_obj_fwd13[k][1], Z = z + c_obj_fwd13[k][2];
        if (X < 0 || X >= f.nx || Y < 0 || Y >= f.ny || Z >= f.nz) continue;
        const size_t j = static_cast<size_t>(X) + static_cast<size_t>(f.nx) * (static_cast<size_t>(Y) + static_cast<size_t>(f.ny) * static_cast<size_t>(Z));
        const uint32_t lj = f.label[j];
        if (lj == kPlNone || lj == li) continue;
        if (EMIT) {
          const uint32_t pj = f.number[lj];
          const int32_t dj = f.d2[j];
          if (at + cnt < n_pairs) {  // (always, while the labels are what the count saw: no write beyond the arrays)
            keys[at + cnt] = (static_cast<uint64_t>(pi < pj ? pi : pj) << 32) | static_cast<uint64_t>(pi < pj ? pj : pi);
            vals[at + cnt] = di < dj ? di : dj;
          }
        }
        ++cnt;
      }
    }
    if (!EMIT) f.pair_count[i] = cnt;
  }
  if (!EMIT) waveStatAdd(f.ctr + PLC_PAIRS, cnt);
}

// what follows the sort: the pairs' rows, the unique edges, the places' components
struct PlGraph {
  uint32_t n_pairs, n_places;  // places before the filter
  const uint64_t* keys;        // sorted
  const int32_t* vals;
  uint32_t* head;              // [n_pairs + 1] 1 where a key differs from its predecessor; scanned in place
  uint32_t* n_unique;          // one word
  uint32_t* edge_a;            // [n_pairs] the unique edges
  uint32_t* edge_b;
  int32_t* edge_clear;         // (preset 0)
  uint32_t* edge_contacts;     // (preset 0)
  uint32_t* edge_new;          // [n_pairs + 1] keep flags, scanned in place
  uint32_t* parent;            // [n_places]
  uint32_t* root;              // [n_places]
  uint32_t* size;              // [n_places] at a root (preset 0)
  uint32_t* place_new;         // [n_places + 1] keep flags, scanned in place
  uint32_t* comp_new;          // [n_places + 1] flags of the kept roots, scanned in place
  uint32_t min_size;
  unsigned long long* ctr;
};

__global__ __launch_bounds__(256) void k_pl_edge_heads(PlGraph g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < g.n_pairs) g.head[i] = (i == 0u || g.keys[i] != g.keys[i - 1]) ? 1u : 0u;
  if (i < g.n_places) g.parent[i] = i;
}

// g.head holds the exclusive scan: the row of pair i is head[i + 1] - 1 (the heads up to and including i)
__global__ __launch_bounds__(256) void k_pl_edge_reduce(PlGraph g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= g.n_pairs) return;
  const uint32_t row = g.head[i + 1] - 1u;  // (pair 0 is a head: never below 0)
  if (row >= g.n_pairs) return;
  const uint64_t key = g.keys[i];
  if (g.head[i + 1] != g.head[i]) g.edge_a[row] = static_cast<uint32_t>(key >> 32), g.edge_b[row] = static_cast<uint32_t>(key);
  atomicMax(&g.edge_clear[row], g.vals[i]);
  atomicAdd(&g.edge_contacts[row], 1u);
  if (i == g.n_pairs - 1u) {
    *g.n_unique = row + 1u;
    atomicAdd(&g.ctr[PLC_EDGES_ALL], static_cast<unsigned long long>(row + 1u));
  }
}

__global__ __launch_bounds__(256) void k_pl_comp_union(PlGraph g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= g.n_pairs || i >= *g.n_unique) return;
  const uint32_t a = g.edge_a[i], b = g.edge_b[i];
  if (a < g.n_places && b < g.n_places) ufUnion(g.parent, a, b);
}

__global__ __launch_bounds__(256) void k_pl_comp_flatten(PlGraph g) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= g.n_places) return;
  const uint32_t r = ufFind(static_cast<const uint32_t*>(g.parent), p);
  g.root[p] = r;
  atomicAdd(&g.size[r], 1u);
}

// keep flags of the places, the kept roots and the unique edges (one grid over max(places, pairs))
__global__ __launch_bounds__(256) void k_pl_comp_keep(PlGraph g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t all = 0u, kept_place = 0u, kept_comp = 0u, kept_edge = 0u;
  if (i < g.n_places) {
    const uint32_t r = g.root[i];
    kept_place = g.size[r] >= g.min_size ? 1u : 0u;
    all = r == i ? 1u : 0u;
    kept_comp = all & kept_place;
    g.place_new[i] = kept_place;
    g.comp_new[i] = kept_comp;
  }
  if (i < g.n_pairs) {
    if (i < *g.n_unique) {
      const uint32_t a = g.edge_a[i];
      kept_edge = (a < g.n_places && g.size[g.root[a]] >= g.min_size) ? 1u : 0u;
    }
    g.edge_new[i] = kept_edge;
  }
  waveStatAdd(g.ctr + PLC_COMPS_ALL, all);
  waveStatAdd(g.ctr + PLC_PLACES, kept_place);
  waveStatAdd(g.ctr + PLC_COMPS, kept_comp);
  waveStatAdd(g.ctr + PLC_EDGES, kept_edge);
}

// the result: the dense place ids, one row per kept place and per kept edge
struct PlResult {
  uint32_t n_places, n_edges;  // kept
  int32_t* place;              // [n] dense
  int32_t* centre;             // [3 * n_places]
  int32_t* centre_d2;
  float* radius;
  uint8_t* basis;
  int32_t* site;               // [3 * n_places]
  uint32_t* n_cells;
  long long* sum;              // [3 * n_places]
  uint32_t* degree;            // (preset 0)
  uint32_t* component;
  uint32_t* edge_a;
  uint32_t* edge_b;
  int32_t* edge_clear;
  uint32_t* edge_contacts;
};

// One lane per cell.  g.place_new / g.comp_new hold the exclusive scans (so a flag is the difference of two neighbours).
__global__ __launch_bounds__(256) void k_pl_finish_cells(PlField f, PlGraph g, PlResult r) {
  const long long n = static_cast<long long>(f.nx) * f.ny * f.nz;
  const long long i = static_cast<long long>(blockIdx.x) * 256 + static_cast<long long>(threadIdx.x);
  if (i >= n) return;
  const uint32_t li = f.label[i];
  int32_t id = -1;
  uint32_t p = 0u;
  if (li != kPlNone) {
    p = f.number[li];
    if (p < g.n_places && g.place_new[p + 1] != g.place_new[p]) id = static_cast<int32_t>(g.place_new[p]);
  }
  r.place[i] = id;
  if (id < 0 || li != static_cast<uint32_t>(i) || static_cast<uint32_t>(id) >= r.n_places) return;
  // the representative writes its place's row
  const size_t q = static_cast<size_t>(id);
  const uint64_t key = f.rec_key[i], acc = f.rec_acc[i];
  const uint32_t c = 0xffffffffu - static_cast<uint32_t>(key);  // the centre's lin (a member: inside the box)
  const uint32_t unx = static_cast<uint32_t>(f.nx), uny = static_cast<uint32_t>(f.ny);
  if (static_cast<long long>(c) >= n) return;  // (cannot happen)
  r.centre[3 * q] = f.ox + static_cast<int>(c % unx), r.centre[3 * q + 1] = f.oy + static_cast<int>((c / unx) % uny), r.centre[3 * q + 2] = f.oz + static_cast<int>(c / (unx * uny));
  r.centre_d2[q] = static_cast<int32_t>(key >> 32);
  r.radius[q] = f.distance[c];
  r.basis[q] = f.basis[c];
  const int32_t s = f.site[c];
  const bool has = s >= 0 && static_cast<long long>(s) < n;
  const uint32_t us = static_cast<uint32_t>(has ? s : 0);
  r.site[3 * q] = has ? f.ox + static_cast<int>(us % unx) : 0, r.site[3 * q + 1] = has ? f.oy + static_cast<int>((us / unx) % uny) : 0;
  r.site[3 * q + 2] = has ? f.oz + static_cast<int>(us / (unx * uny)) : 0;
  const long long cells = static_cast<long long>(acc >> 48);
  r.n_cells[q] = static_cast<uint32_t>(cells);
  // the sums are tile-local: the tile's first cell, in world cells, times the count brings them home
  const int x = static_cast<int>(i % f.nx), y = static_cast<int>((i / f.nx) % f.ny), z = static_cast<int>(i / (static_cast<long long>(f.nx) * f.ny));
  const long long wx = static_cast<long long>(plFloorDiv(f.ox + x, f.edge)) * f.edge, wy = static_cast<long long>(plFloorDiv(f.oy + y, f.edge)) * f.edge;
  const long long wz = static_cast<long long>(plFloorDiv(f.oz + z, f.edge)) * f.edge;
  r.sum[3 * q] = static_cast<long long>(acc & 0xffffull) + cells * wx;
  r.sum[3 * q + 1] = static_cast<long long>((acc >> 16) & 0xffffull) + cells * wy;
  r.sum[3 * q + 2] = static_cast<long long>((acc >> 32) & 0xffffull) + cells * wz;
  const uint32_t root = g.root[p];
  r.component[q] = root < g.n_places ? g.comp_new[root] : 0u;
}

// One lane per unique edge.  g.edge_new holds the exclusive scan.
__global__ __launch_bounds__(256) void k_pl_finish_edges(PlGraph g, PlResult r) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= g.n_pairs || i >= *g.n_unique || g.edge_new[i + 1] == g.edge_new[i]) return;
  const uint32_t e = g.edge_new[i];
  const uint32_t pa = g.edge_a[i], pb = g.edge_b[i];
  if (e >= r.n_edges || pa >= g.n_places || pb >= g.n_places) return;
  const uint32_t a = g.place_new[pa], b = g.place_new[pb];
  if (a >= r.n_places || b >= r.n_places) return;
  r.edge_a[e] = a, r.edge_b[e] = b;
  r.edge_clear[e] = g.edge_clear[i];
  r.edge_contacts[e] = g.edge_contacts[i];
  atomicAdd(&r.degree[a], 1u);
  atomicAdd(&r.degree[b], 1u);
}

}  // namespace khr
