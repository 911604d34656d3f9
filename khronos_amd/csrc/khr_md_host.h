// khr_md_host.h — the host's share of the motion detector's frame finish (free_space_motion_detector.cpp:205-399): cluster order,
// merge groups, size filter and ids from the device's component records, and the seed-graph walk for the frames the records cannot
// answer.  Plain C++17 on pointers and sizes, no HIP: motionFinish (khronos_amd.hip) hands it views of page-locked memory,
// tests/md_host_selftest.cpp the same lists from a file (tests/test_cpu_md_host.py holds both paths to the oracle).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

namespace khr {

// One component of the seed graph as the device reduces it (k_md_comp_reduce): the length of the cluster's pixel list (seed pixels
// + the pixels of every adjacent boundary voxel once per adjacent seed, :255-265), the first seed in the canonical (x, y, z) order
// (= the cluster's position in the reference's visiting order, ASSUMPTIONS.md C.1) and the voxel bounding box (merge pre-test).
struct CompAcc {
  unsigned long long n_pixels;
  unsigned long long min_key;  // canonical-order key of the first seed
  int32_t lo[3], hi[3];
  uint32_t root, pad;  // in the downloaded records: the component's 64-bit overlap row, (pad << 32) | root (k_md_comp_overlap)
};

namespace mdh {

struct Vox { int64_t v[3]; };        // global voxel index (x, y, z)
inline Vox voxelOf(uint64_t key) {  // (unpackKey of khr_device.h)
  return Vox{{static_cast<int64_t>(key & 0x1fffffu) - (1 << 20), static_cast<int64_t>((key >> 21) & 0x1fffffu) - (1 << 20),
              static_cast<int64_t>((key >> 42) & 0x1fffffu) - (1 << 20)}};
}
// checkClusterOverlap (:333-343): (p1 - p2).norm() on int64 vectors truncates to an integer (ASSUMPTIONS.md C.2)
inline bool closerThan(int64_t n2, float sep) { return static_cast<float>(static_cast<int64_t>(std::sqrt(static_cast<double>(n2)))) < sep; }
// the gap between two boxes (anything with lo[3] / hi[3]) is a lower bound of every pairwise voxel distance: the merge pre-test
template <class A, class B>
inline bool boxesCloserThan(const A& a, const B& b, float sep) {
  int64_t gap2 = 0;
  for (int d = 0; d < 3; ++d) {
    const int64_t gp = std::max<int64_t>(0, std::max(static_cast<int64_t>(a.lo[d]) - b.hi[d], static_cast<int64_t>(b.lo[d]) - a.hi[d]));
    gap2 += gp * gp;
  }
  return closerThan(gap2, sep);
}

// cluster order = order in which the walk meets the first seed of each component (ASSUMPTIONS.md C.1)
inline std::vector<uint32_t> clusterOrder(const CompAcc* comp, uint32_t R) {
  std::vector<uint32_t> order(R);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return comp[a].min_key < comp[b].min_key; });
  return order;
}

// mergeClusters (:274-355) can only join clusters whose boxes come closer than the separation: false = the clusters are the components
inline bool mayMerge(const CompAcc* comp, uint32_t R, float sep) {
  for (uint32_t i = 0; i < R; ++i)
    for (uint32_t j = i + 1; j < R; ++j)
      if (boxesCloserThan(comp[i], comp[j], sep)) return true;
  return false;
}

// disjoint sets whose representative is the smallest member
struct Groups {
  std::vector<uint32_t> rep;
  explicit Groups(uint32_t n) : rep(n) { std::iota(rep.begin(), rep.end(), 0u); }
  uint32_t find(uint32_t x) {
    while (rep[x] != x) x = rep[x] = rep[rep[x]];
    return x;
  }
  void unite(uint32_t a, uint32_t b) {
    a = find(a), b = find(b);
    if (a != b) rep[std::max(a, b)] = std::min(a, b);
  }
  std::vector<uint32_t> labels() {
    for (uint32_t i = 0; i < rep.size(); ++i) rep[i] = find(i);
    return rep;
  }
};

// mergeClusters from the device's overlap rows (R <= 64; bits at or above R are ignored): the clusters that end up together are
// the connected components of the overlap graph (getConnectedClusters recurses).  Returns each component's group label.
inline std::vector<uint32_t> groupsFromRows(const CompAcc* comp, uint32_t R) {
  Groups g(R);
  for (uint32_t i = 0; i < R && i < 64; ++i) {
    unsigned long long row = ((static_cast<unsigned long long>(comp[i].pad) << 32) | comp[i].root) & ~(1ull << i);
    for (; row; row &= row - 1ull) {
      const uint32_t j = static_cast<uint32_t>(__builtin_ctzll(row));
      if (j < R) g.unite(i, j);
    }
  }
  return g.labels();
}

// applyClusterLevelFilters (:365-379) + the ids of writeClustersToData (:381-399).  `order` lists the R components in cluster
// order, group[r] labels r's merge group, px(r) is the length of r's pixel list.  A merged cluster stands at the position of its
// first member (`current` only ever absorbs later clusters) and lists its members' pixels; it is filtered by that length; ids
// start at 1 and saturate at 255.  id[r]: 0 = r's cluster was filtered out, otherwise its id.
using Kept = std::vector<std::pair<int, uint64_t>>;  // the kept clusters in cluster order: (id, pixel list length incl. duplicates)
template <class Px>
inline Kept numberClusters(const uint32_t* order, const uint32_t* group, uint32_t R, Px px, int min_size, int max_size, std::vector<int32_t>* id_out) {
  Kept kept;
  id_out->assign(R, 0);
  std::vector<uint64_t> gpx(R, 0);
  std::vector<int32_t> gid(R, -1);  // per group label: -1 not met yet, 0 filtered out, > 0 the cluster's id
  for (uint32_t r = 0; r < R; ++r) gpx[group[r]] += px(r);
  int id = 1;
  for (uint32_t k = 0; k < R; ++k) {
    const uint32_t r = order[k], g = group[r];
    if (gid[g] < 0) {  // the group's first member in cluster order: its position is the merged cluster's
      const int size = static_cast<int>(gpx[g]);
      gid[g] = size < min_size || size > max_size ? 0 : id;
      if (gid[g]) kept.emplace_back(id, gpx[g]);
      if (gid[g] && id < 255) ++id;
    }
    (*id_out)[r] = gid[g];
  }
  return kept;
}

// the compact lists of a seed frame (k_md_compact, k_md_adjacency)
struct WalkLists {
  const uint64_t *seed_keys, *bnd_keys;
  const uint32_t *seed_counts, *bnd_counts, *adj;  // adj[s * nn + j]: 0xffffffff = none, bit 31 set = seed id, otherwise a boundary id
  uint32_t S, B;
  int nn;
};

// The whole clustering on the host, sequential as in the reference: clusterDynamicVoxels (:205-272), mergeClusters, filter, ids.
// Writes seed_final[S] and bnd_final[B] (cluster id per listed voxel, 0 = none) and bnd_deg[B] (per boundary voxel: how many
// seeds of kept clusters list it, :255-265); returns the kept clusters.  The outputs may not alias the lists.
inline Kept walkClusters(const WalkLists& l, float sep, int min_size, int max_size, int32_t* seed_final, int32_t* bnd_final, int32_t* bnd_deg) {
  const uint32_t S = l.S, B = l.B;
  const int nn = l.nn;
  // canonical seed order: ascending (x, y, z) (ASSUMPTIONS.md C.1)
  std::vector<uint32_t> order(S);
  std::vector<Vox> sg(S);
  std::iota(order.begin(), order.end(), 0u);
  for (uint32_t i = 0; i < S; ++i) sg[i] = voxelOf(l.seed_keys[i]);
  std::sort(order.begin(), order.end(),
            [&](uint32_t a, uint32_t b) { return std::lexicographical_compare(sg[a].v, sg[a].v + 3, sg[b].v, sg[b].v + 3); });
  struct Cluster {
    uint64_t n_pixels = 0;        // with the duplicates the reference produces (:255-265)
    std::vector<uint32_t> seeds, bnds;  // seed ids, boundary ids (unique)
    std::vector<Vox> vox;               // the listed voxels
    int64_t lo[3], hi[3];
  };
  std::vector<Cluster> clusters;
  std::vector<uint8_t> closed(S, 0);
  std::vector<uint32_t> stack;
  for (uint32_t s0 : order) {
    if (closed[s0]) continue;
    stack.assign(1, s0);
    Cluster cl;
    while (!stack.empty()) {
      const uint32_t r = stack.back();
      stack.pop_back();
      if (closed[r]) continue;
      closed[r] = 1;
      cl.n_pixels += l.seed_counts[r];
      cl.seeds.push_back(r);
      for (int k = 0; k < nn; ++k) {
        const uint32_t a = l.adj[static_cast<size_t>(r) * nn + k];
        if (a == 0xffffffffu) continue;
        if (a & 0x80000000u) {
          stack.push_back(a & 0x7fffffffu);
        } else {
          cl.n_pixels += l.bnd_counts[a];  // appended once per adjacent expanded seed
          cl.bnds.push_back(a);
        }
      }
    }
    std::sort(cl.bnds.begin(), cl.bnds.end());
    cl.bnds.erase(std::unique(cl.bnds.begin(), cl.bnds.end()), cl.bnds.end());
    for (int d = 0; d < 3; ++d) { cl.lo[d] = INT64_MAX; cl.hi[d] = INT64_MIN; }
    for (uint32_t r : cl.seeds) cl.vox.push_back(sg[r]);
    for (uint32_t r : cl.bnds) cl.vox.push_back(voxelOf(l.bnd_keys[r]));
    for (const Vox& g : cl.vox)
      for (int d = 0; d < 3; ++d) { cl.lo[d] = std::min(cl.lo[d], g.v[d]); cl.hi[d] = std::max(cl.hi[d], g.v[d]); }
    clusters.push_back(std::move(cl));
  }
  // mergeClusters (:274-355): the merged clusters are the connected components of the overlap relation between the ORIGINAL clusters
  const uint32_t nc = static_cast<uint32_t>(clusters.size());
  auto overlap = [&](const Cluster& a, const Cluster& b) {
    if (!boxesCloserThan(a, b, sep)) return false;
    for (const Vox& p : a.vox)
      for (const Vox& q : b.vox) {
        const int64_t dx = p.v[0] - q.v[0], dy = p.v[1] - q.v[1], dz = p.v[2] - q.v[2];
        if (closerThan(dx * dx + dy * dy + dz * dz, sep)) return true;
      }
    return false;
  };
  Groups groups(nc);
  for (uint32_t i = 0; i < nc; ++i)
    for (uint32_t j = i + 1; j < nc; ++j)
      if (overlap(clusters[i], clusters[j])) groups.unite(i, j);
  const std::vector<uint32_t> group = groups.labels();
  // Filter and ids by the function the records path uses.  Why it gives what the reference's loop over its merged clusters gives:
  // `clusters` is in cluster order already (order = identity); a label is its group's smallest index, i.e. the first member, at
  // whose position the reference keeps the merged cluster; the merged pixel list is the members' lists concatenated, so its length
  // is the sum numberClusters forms.
  std::vector<uint32_t> identity(nc);
  std::vector<int32_t> ids;
  std::iota(identity.begin(), identity.end(), 0u);
  Kept kept = numberClusters(identity.data(), group.data(), nc, [&](uint32_t i) { return clusters[i].n_pixels; }, min_size, max_size, &ids);
  // writeClustersToData (:381-399): later clusters overwrite earlier ones.  Ids never decrease from one kept cluster to the next,
  // so a boundary voxel that several clusters list ends with the largest of their ids (k_md_comp_finals takes the same maximum).
  std::fill(seed_final, seed_final + S, 0);
  std::fill(bnd_final, bnd_final + B, 0);
  std::fill(bnd_deg, bnd_deg + B, 0);
  for (uint32_t ci = 0; ci < nc; ++ci) {
    const int32_t id = ids[ci];
    if (!id) continue;
    for (uint32_t r : clusters[ci].seeds) {
      seed_final[r] = id;
      for (int k = 0; k < nn; ++k) {
        const uint32_t a = l.adj[static_cast<size_t>(r) * nn + k];
        if (a != 0xffffffffu && !(a & 0x80000000u)) ++bnd_deg[a];
      }
    }
    for (uint32_t r : clusters[ci].bnds) bnd_final[r] = std::max(bnd_final[r], id);
  }
  return kept;
}

}  // namespace mdh
}  // namespace khr
