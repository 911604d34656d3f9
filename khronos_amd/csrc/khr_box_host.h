// khr_box_host.h — what the host sides of the box-field calls share (khr_distance_field, khr_voronoi_field, khr_places_graph,
// khr_travel_field and their _from / _into / _box forms): the 256-byte arena their buffers are carved with and every layout built
// on it, the check of a cell box, the launch geometry of a separable pass, and the box a result describes.  Plain C++17 on sizes
// and indices, no HIP: khronos_amd.hip adds the device pointers, tests/box_host_selftest.cpp prints the same numbers
// (tests/test_cpu_box_host.py holds them to the layouts they were moved from).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/khronos_amd.h"

namespace khr {

// byte offsets into one block, each a multiple of 256
struct Arena {
  static size_t align(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }
  size_t take(size_t bytes) { const size_t at = o_; o_ += align(bytes); return at; }  // where `bytes` more begin
  size_t bytes() const { return o_; }

 private:
  size_t o_ = 0;
};

// ---- the layouts: offsets of the arrays in their block and the block's size.  The fields are taken in the order written in
// each builder, which is the order in memory ----------------------------------------------------------------------------------

// khr_voronoi_field: the dense outputs of n cells one after the other, then the per-workgroup list counts (one word more than
// the workgroups of 256 cells).  khr_places_graph and khr_travel_field find the field they read with the same call.
struct VorDense {
  size_t distance, d2, site, status, basis, wg_count, bytes;
};
inline VorDense vorDense(size_t n) {
  VorDense L{};
  Arena a;
  L.distance = a.take(4 * n), L.d2 = a.take(4 * n), L.site = a.take(4 * n), L.status = a.take(n), L.basis = a.take(n);
  L.wg_count = a.take(4 * ((n + 255) / 256 + 1));
  L.bytes = a.bytes();
  return L;
}
// ... and the list of m cells
struct VorList {
  size_t cells, distance, basis, sites, bytes;
};
inline VorList vorList(size_t m) {
  VorList L{};
  Arena a;
  L.cells = a.take(12 * m), L.distance = a.take(4 * m), L.basis = a.take(m), L.sites = a.take(12 * KHR_VOR_MAX_BASIS * m);
  L.bytes = std::max<size_t>(a.bytes(), 256);  // (never empty: the owner exists from the first call on)
  return L;
}

// khr_places_graph_from: the device copy of a host caller's field of n cells
struct PlIn {
  size_t distance, d2, basis, site, bytes;
};
inline PlIn plIn(size_t n) {
  PlIn L{};
  Arena a;
  L.distance = a.take(4 * n), L.d2 = a.take(4 * n), L.basis = a.take(n), L.site = a.take(4 * n);
  L.bytes = a.bytes();
  return L;
}
// khr_places_graph: per-cell work arrays of n cells, the dense place ids last
struct PlDense {
  size_t rec_key, rec_acc, label, number, pair_count, place, bytes;
};
inline PlDense plDense(size_t n) {
  PlDense L{};
  Arena a;
  L.rec_key = a.take(8 * n), L.rec_acc = a.take(8 * n), L.label = a.take(4 * n), L.number = a.take(4 * (n + 1)), L.pair_count = a.take(4 * (n + 1));
  L.place = a.take(4 * n);
  L.bytes = a.bytes();
  return L;
}
// ... work lists of m adjacent pairs and p places (before the filter)
struct PlWork {
  size_t keys, keys_sorted, vals, vals_sorted, head, n_unique, edge_a, edge_b, edge_clear, edge_contacts, edge_new, parent, root, size, place_new, comp_new, bytes;
};
inline PlWork plWork(size_t m, size_t p) {
  PlWork L{};
  Arena a;
  L.keys = a.take(8 * m), L.keys_sorted = a.take(8 * m), L.vals = a.take(4 * m), L.vals_sorted = a.take(4 * m), L.head = a.take(4 * (m + 1)), L.n_unique = a.take(4);
  L.edge_a = a.take(4 * m), L.edge_b = a.take(4 * m), L.edge_clear = a.take(4 * m), L.edge_contacts = a.take(4 * m), L.edge_new = a.take(4 * (m + 1));
  L.parent = a.take(4 * p), L.root = a.take(4 * p), L.size = a.take(4 * p), L.place_new = a.take(4 * (p + 1)), L.comp_new = a.take(4 * (p + 1));
  L.bytes = a.bytes();
  return L;
}
// ... the result lists of p kept places and e kept edges
struct PlOut {
  size_t sum, centre, centre_d2, radius, basis, site, n_cells, degree, component, edge_a, edge_b, edge_clear, edge_contacts, bytes;
};
inline PlOut plOut(size_t p, size_t e) {
  PlOut L{};
  Arena a;
  L.sum = a.take(24 * p), L.centre = a.take(12 * p), L.centre_d2 = a.take(4 * p), L.radius = a.take(4 * p), L.basis = a.take(p), L.site = a.take(12 * p);
  L.n_cells = a.take(4 * p), L.degree = a.take(4 * p), L.component = a.take(4 * p);
  L.edge_a = a.take(4 * e), L.edge_b = a.take(4 * e), L.edge_clear = a.take(4 * e), L.edge_contacts = a.take(4 * e);
  L.bytes = std::max<size_t>(a.bytes(), 256);  // (never empty: the owner exists from the first call on)
  return L;
}

// khr_travel_field_from: the device copy of a host caller's field of n cells and of g goals
struct TfIn {
  size_t distance, status, goals, bytes;
};
inline TfIn tfIn(size_t n, size_t g) {
  TfIn L{};
  Arena a;
  L.distance = a.take(4 * n), L.status = a.take(n), L.goals = a.take(12 * g);
  L.bytes = a.bytes();
  return L;
}
// khr_travel_field: the per-cell arrays of n cells in `tiles` tiles -- the keys, the result, then the work arrays
struct TfDense {
  size_t keys, cost, goal, parent, mask, flags, go_on, bytes;
};
inline TfDense tfDense(size_t n, size_t tiles) {
  TfDense L{};
  Arena a;
  L.keys = a.take(8 * n), L.cost = a.take(4 * n), L.goal = a.take(4 * n), L.parent = a.take(n), L.mask = a.take(n), L.flags = a.take(2 * tiles);
  L.go_on = a.take(4 * KHR_TF_ROUNDS_PER_WAIT);
  L.bytes = a.bytes();
  return L;
}
// khr_travel_paths: the per-start arrays of s starts
struct TfStarts {
  size_t offsets, starts, path_cost, path_goal, bytes;
};
inline TfStarts tfStarts(size_t s) {
  TfStarts L{};
  Arena a;
  L.offsets = a.take(8 * (s + 1)), L.starts = a.take(12 * s), L.path_cost = a.take(4 * s), L.path_goal = a.take(4 * s);
  L.bytes = a.bytes();
  return L;
}

// ---- the box of cells a call works on ----------------------------------------------------------------------------------------

// The rules, in the order they are checked (per axis the first two, then the third): dims[axis] in 1 .. KHR_DF_MAX_DIM; the box,
// in voxels (cells of `ratio` voxels), inside the index range (-2^30, 2^30); at most 2^24 cells.  `bad` is the axis of a
// BOX_BAD_DIM / BOX_BAD_RANGE, -1 otherwise; `cells` is written with BOX_OK and BOX_BAD_CELLS.  64-bit throughout: no origin of
// 32 bits overflows.
enum BoxCheck { BOX_OK = 0, BOX_BAD_DIM, BOX_BAD_RANGE, BOX_BAD_CELLS };
inline BoxCheck checkCellBox(const int32_t origin[3], const int32_t dims[3], int ratio, size_t* cells, int* bad) {
  constexpr int64_t kEdge = int64_t(1) << 30;
  uint64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    const int64_t lo = static_cast<int64_t>(origin[a]) * ratio, hi = (static_cast<int64_t>(origin[a]) + dims[a]) * ratio - 1;
    const bool bad_dim = dims[a] < 1 || dims[a] > KHR_DF_MAX_DIM;
    if (bad_dim || lo <= -kEdge || hi >= kEdge) {
      *bad = a;
      return bad_dim ? BOX_BAD_DIM : BOX_BAD_RANGE;
    }
    n *= static_cast<uint64_t>(dims[a]);
  }
  *bad = -1;
  *cells = static_cast<size_t>(n);
  return n > (uint64_t(1) << 24) ? BOX_BAD_CELLS : BOX_OK;
}

// what a successful call leaves behind for the calls that read its result
struct BoxResult {
  bool valid = false;  // the call succeeded and nothing has discarded its result
  size_t cells = 0;    // cells of the box the result describes
  int32_t origin[3] = {0, 0, 0}, dims[3] = {0, 0, 0};
  void set(const int32_t o[3], const int32_t d[3], size_t n) {
    for (int a = 0; a < 3; ++a) origin[a] = o[a], dims[a] = d[a];
    cells = n;
    valid = true;
  }
  void boxOut(int32_t* o, int32_t* d) const {  // (either may be null)
    for (int a = 0; a < 3; ++a) {
      if (o) o[a] = origin[a];
      if (d) d[a] = dims[a];
    }
  }
};

// ---- a separable pass over a grid of nx * ny * nz cells ----------------------------------------------------------------------

// The x pass gives a workgroup `per_wg` whole lines (gx workgroups over the ny * nz lines); a y / z pass gives it strips of `strip`
// adjacent x and `per_wg` planes along the remaining axis (gx strips by gy plane groups).  `tile_cells` is what a workgroup's LDS
// tile holds.
struct PassGrid {
  unsigned gx, gy;
  int per_wg;
};
inline PassGrid axisPassGrid(int axis, int nx, int ny, int nz, int tile_cells, int strip) {
  if (axis == 0) {
    const int per_wg = std::max(1, tile_cells / nx);
    const long long lines = static_cast<long long>(ny) * nz;
    return {static_cast<unsigned>((lines + per_wg - 1) / per_wg), 1u, per_wg};
  }
  const int len = axis == 1 ? ny : nz, other = axis == 1 ? nz : ny;
  const int per_wg = std::max(1, tile_cells / (len * strip));
  return {static_cast<unsigned>((nx + strip - 1) / strip), static_cast<unsigned>((other + per_wg - 1) / per_wg), per_wg};
}

}  // namespace khr
