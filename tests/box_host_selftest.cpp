// box_host_selftest.cpp — prints what khronos_amd/csrc/khr_box_host.h computes for the requests on standard input, one line each;
// tests/test_cpu_box_host.py writes the requests and holds the answers to their definitions.  Built with the address and
// undefined-behaviour sanitizers, so an overflow in the box check ends the run.
//   layout NAME A B          -> NAME A B : field offset ... bytes N      (fields in the order they lie in memory)
//   box OX OY OZ NX NY NZ R  -> box RULE AXIS CELLS                      (RULE 0 ok, 1 dim, 2 range, 3 cells; CELLS 0 unless written)
//   grid AXIS NX NY NZ T S   -> grid GX GY PER_WG
//   result OX OY OZ NX NY NZ -> result VALID CELLS ox oy oz nx ny nz     (BoxResult::set, then boxOut)
#include <cstdio>
#include <iostream>
#include <string>

#include "../khronos_amd/csrc/khr_box_host.h"

using namespace khr;

namespace {

struct Field {
  const char* name;
  size_t at;
};

template <size_t N>
void show(const std::string& name, size_t a, size_t b, const Field (&f)[N], size_t bytes) {
  std::printf("%s %zu %zu :", name.c_str(), a, b);
  for (const Field& x : f) std::printf(" %s %zu", x.name, x.at);
  std::printf(" bytes %zu\n", bytes);
}

bool layout(const std::string& name, size_t a, size_t b) {
  if (name == "vorDense") {
    const VorDense L = vorDense(a);
    show(name, a, b, {{"distance", L.distance}, {"d2", L.d2}, {"site", L.site}, {"status", L.status}, {"basis", L.basis}, {"wg_count", L.wg_count}}, L.bytes);
  } else if (name == "vorList") {
    const VorList L = vorList(a);
    show(name, a, b, {{"cells", L.cells}, {"distance", L.distance}, {"basis", L.basis}, {"sites", L.sites}}, L.bytes);
  } else if (name == "plIn") {
    const PlIn L = plIn(a);
    show(name, a, b, {{"distance", L.distance}, {"d2", L.d2}, {"basis", L.basis}, {"site", L.site}}, L.bytes);
  } else if (name == "plDense") {
    const PlDense L = plDense(a);
    show(name, a, b, {{"rec_key", L.rec_key}, {"rec_acc", L.rec_acc}, {"label", L.label}, {"number", L.number}, {"pair_count", L.pair_count}, {"place", L.place}}, L.bytes);
  } else if (name == "plWork") {
    const PlWork L = plWork(a, b);
    show(name, a, b, {{"keys", L.keys}, {"keys_sorted", L.keys_sorted}, {"vals", L.vals}, {"vals_sorted", L.vals_sorted}, {"head", L.head}, {"n_unique", L.n_unique},
                      {"edge_a", L.edge_a}, {"edge_b", L.edge_b}, {"edge_clear", L.edge_clear}, {"edge_contacts", L.edge_contacts}, {"edge_new", L.edge_new},
                      {"parent", L.parent}, {"root", L.root}, {"size", L.size}, {"place_new", L.place_new}, {"comp_new", L.comp_new}}, L.bytes);
  } else if (name == "plOut") {
    const PlOut L = plOut(a, b);
    show(name, a, b, {{"sum", L.sum}, {"centre", L.centre}, {"centre_d2", L.centre_d2}, {"radius", L.radius}, {"basis", L.basis}, {"site", L.site}, {"n_cells", L.n_cells},
                      {"degree", L.degree}, {"component", L.component}, {"edge_a", L.edge_a}, {"edge_b", L.edge_b}, {"edge_clear", L.edge_clear},
                      {"edge_contacts", L.edge_contacts}}, L.bytes);
  } else if (name == "tfIn") {
    const TfIn L = tfIn(a, b);
    show(name, a, b, {{"distance", L.distance}, {"status", L.status}, {"goals", L.goals}}, L.bytes);
  } else if (name == "tfDense") {
    const TfDense L = tfDense(a, b);
    show(name, a, b, {{"keys", L.keys}, {"cost", L.cost}, {"goal", L.goal}, {"parent", L.parent}, {"mask", L.mask}, {"flags", L.flags}, {"go_on", L.go_on}}, L.bytes);
  } else if (name == "tfStarts") {
    const TfStarts L = tfStarts(a);
    show(name, a, b, {{"offsets", L.offsets}, {"starts", L.starts}, {"path_cost", L.path_cost}, {"path_goal", L.path_goal}}, L.bytes);
  } else {
    return false;
  }
  return true;
}

}  // namespace

int main() {
  std::string what;
  while (std::cin >> what) {
    if (what == "layout") {
      std::string name;
      size_t a = 0, b = 0;
      if (!(std::cin >> name >> a >> b) || !layout(name, a, b)) return 2;
    } else if (what == "box") {
      int32_t o[3], d[3];
      int ratio = 0, axis = -2;
      size_t cells = 0;
      if (!(std::cin >> o[0] >> o[1] >> o[2] >> d[0] >> d[1] >> d[2] >> ratio)) return 2;
      const BoxCheck rule = checkCellBox(o, d, ratio, &cells, &axis);
      std::printf("box %d %d %zu\n", static_cast<int>(rule), axis, cells);
    } else if (what == "grid") {
      int axis = 0, nx = 0, ny = 0, nz = 0, tile = 0, strip = 0;
      if (!(std::cin >> axis >> nx >> ny >> nz >> tile >> strip)) return 2;
      const PassGrid g = axisPassGrid(axis, nx, ny, nz, tile, strip);
      std::printf("grid %u %u %d\n", g.gx, g.gy, g.per_wg);
    } else if (what == "result") {
      int32_t o[3], d[3], oo[3] = {0, 0, 0}, dd[3] = {0, 0, 0};
      if (!(std::cin >> o[0] >> o[1] >> o[2] >> d[0] >> d[1] >> d[2])) return 2;
      BoxResult r;
      if (r.valid || r.cells != 0) return 3;
      r.set(o, d, static_cast<size_t>(d[0]) * d[1] * d[2]);
      r.boxOut(nullptr, nullptr);
      r.boxOut(oo, nullptr);
      r.boxOut(nullptr, dd);
      std::printf("result %d %zu %d %d %d %d %d %d\n", r.valid ? 1 : 0, r.cells, oo[0], oo[1], oo[2], dd[0], dd[1], dd[2]);
    } else {
      return 2;
    }
  }
  return 0;
}
