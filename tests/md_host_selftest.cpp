// The motion detector's host stages (khronos_amd/csrc/khr_md_host.h) on one case from standard input, results on standard output;
// tests/test_cpu_md_host.py writes the cases and compares with the oracle.  All numbers are unsigned decimal integers:
//   nn  sep (bits of the float)  min_size  max_size  S  B
//   S seed keys, S seed counts, S * nn adjacency entries, B boundary keys, B boundary counts
//   R (0 = no component records), then per record: n_pixels min_key lo[3] hi[3] (biased by 2^20) row
//   with_rows (1 = the rows are the device's overlap rows)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../khronos_amd/csrc/khr_md_host.h"

using namespace khr;

static uint64_t next() {
  unsigned long long v = 0;
  if (std::scanf("%llu", &v) != 1) {
    std::fprintf(stderr, "md_host_selftest: input ends early\n");
    std::exit(2);
  }
  return v;
}
template <class T>
static std::vector<T> list(size_t n) {
  std::vector<T> v(n);
  for (T& x : v) x = static_cast<T>(next());
  return v;
}
template <class T>
static void print(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (const T& x : v) std::printf(" %lld", static_cast<long long>(x));
  std::printf("\n");
}
static void printKept(const char* name, const std::vector<std::pair<int, uint64_t>>& kept) {
  std::printf("%s", name);
  for (const auto& k : kept) std::printf(" %d %" PRIu64, k.first, k.second);
  std::printf("\n");
}

int main() {
  const int nn = static_cast<int>(next());
  const uint32_t sep_bits = static_cast<uint32_t>(next());
  float sep;
  std::memcpy(&sep, &sep_bits, sizeof(sep));
  const int min_size = static_cast<int>(next()), max_size = static_cast<int>(next());
  const uint32_t S = static_cast<uint32_t>(next()), B = static_cast<uint32_t>(next());
  const std::vector<uint64_t> sk = list<uint64_t>(S);
  const std::vector<uint32_t> sc = list<uint32_t>(S), adj = list<uint32_t>(static_cast<size_t>(S) * nn);
  const std::vector<uint64_t> bk = list<uint64_t>(B);
  const std::vector<uint32_t> bc = list<uint32_t>(B);

  std::vector<int32_t> seed_final(S, -1), bnd_final(B, -1), bnd_deg(B, -1);
  const mdh::WalkLists lists{sk.data(), bk.data(), sc.data(), bc.data(), adj.data(), S, B, nn};
  const auto kept = mdh::walkClusters(lists, sep, min_size, max_size, seed_final.data(), bnd_final.data(), bnd_deg.data());
  std::printf("walk %zu\n", kept.size());
  printKept("kept", kept);
  print("seed_final", seed_final);
  print("bnd_final", bnd_final);
  print("bnd_deg", bnd_deg);

  const uint32_t R = static_cast<uint32_t>(next());
  if (R == 0) return 0;
  std::vector<CompAcc> comp(R);
  for (CompAcc& a : comp) {
    a.n_pixels = next();
    a.min_key = next();
    for (int d = 0; d < 3; ++d) a.lo[d] = static_cast<int32_t>(static_cast<int64_t>(next()) - (1 << 20));
    for (int d = 0; d < 3; ++d) a.hi[d] = static_cast<int32_t>(static_cast<int64_t>(next()) - (1 << 20));
    const uint64_t row = next();
    a.root = static_cast<uint32_t>(row);
    a.pad = static_cast<uint32_t>(row >> 32);
  }
  const bool with_rows = next() != 0;
  // the choice motionFinish makes: components as they are when nothing can merge, groups from the rows when there are rows
  const bool may_merge = mdh::mayMerge(comp.data(), R, sep);
  std::printf("may_merge %d\n", may_merge ? 1 : 0);
  if (may_merge && !with_rows) return 0;
  const std::vector<uint32_t> order = mdh::clusterOrder(comp.data(), R);
  const std::vector<uint32_t> group = may_merge ? mdh::groupsFromRows(comp.data(), R) : mdh::Groups(R).labels();
  std::vector<int32_t> ids;
  const mdh::Kept rkept = mdh::numberClusters(order.data(), group.data(), R, [&](uint32_t r) { return comp[r].n_pixels; }, min_size, max_size, &ids);
  std::printf("records %zu\n", rkept.size());
  printKept("rkept", rkept);
  print("comp_id", ids);
  return 0;
}
