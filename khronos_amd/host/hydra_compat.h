// hydra_compat.h — minimal stand-ins for the Hydra / spark_dsg types that appear in the signature of
// khronos::ActiveWindow (khronos/include/khronos/active_window/active_window.h:67-193).  Hydra is an
// un-vendored dependency of the reference (install/https.rosinstall:5-8) and is not available offline; in
// a real integration these are the genuine Hydra types and this header disappears.
#pragma once
#include <chrono>
#include <cmath>
#include <fstream>
#include <functional>
#include <map>
#include <mutex>
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/khronos_amd.h"
#include "mini_yaml.h"

namespace hydra {

using TimeStamp = uint64_t;
inline double toSeconds(TimeStamp t) { return static_cast<double>(t) / 1e9; }
inline TimeStamp fromSeconds(double s) { return static_cast<TimeStamp>(s * 1e9); }

using BlockIndex = std::array<int32_t, 3>;
using BlockIndices = std::vector<BlockIndex>;

struct Sensor {
  int width = 0, height = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0;
  float min_range = 0.1f, max_range = 5.f;
};

// hydra::InputPacket role: raw sensor frame + pose.  Row-major 4x4 doubles (Eigen::Isometry3d role).
struct InputPacket {
  TimeStamp timestamp_ns = 0;
  double world_T_body[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double body_T_sensor[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  Sensor sensor;
  const float* depth = nullptr;     // H*W metres
  const uint8_t* color = nullptr;   // H*W*3
  const int32_t* labels = nullptr;  // H*W
  bool on_device = false;           // buffers are HBM-resident on the context's device
  bool buffers_complete = false;    // on_device: no stream is still writing the buffers when the packet is handed over (KHR_PF_INPUT_READY:
                                    // the conversion may then run on the context's second stream, beside the previous frame's tail)
  // open-set features of the instance ids of `labels` (InputData::label_features, used at instance_forwarding.cpp:96,141)
  std::map<int, std::vector<float>> label_features;
};

inline void mul4(const double* a, const double* b, double* o) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += a[4 * r + k] * b[4 * k + c];
      o[4 * r + c] = s;
    }
}

// hydra::InputData role (fields SURVEY.md A.2).  The normalised images live in a device frame slot of the
// fusion context; host copies are fetched on demand.
struct InputData {
  TimeStamp timestamp_ns = 0;
  double world_T_body[16];
  double world_T_sensor[16];
  Sensor sensor;
  khr_ctx* ctx = nullptr;
  int slot = -1;  // device frame slot
  std::map<int, std::vector<float>> label_features;  // InputData::label_features
  // keeps the slot out of the ring for as long as any copy of this InputData lives (the shared_ptr<FrameData> ownership of
  // the reference: buffer entries and extraction workers keep frames alive, active_window.cpp:261-263)
  std::shared_ptr<void> slot_lease;
  void retainSlot() {
    if (!ctx || slot < 0 || khr_retain_slot(ctx, slot) < 0) return;
    khr_ctx* c = ctx;
    const int s = slot;
    slot_lease = std::shared_ptr<void>(nullptr, [c, s](void*) { khr_release_slot(c, s); });
  }
  // ActiveWindowOutput::sensor_data (active_window.cpp:165): the output's copy does not lease the ring slot -- outputs wait in a
  // consumer's queue for an unbounded time -- it owns a device-side copy of the frame's images instead (khr_frame_copy, taken in
  // stream order when the output is built) and fetches from that
  std::shared_ptr<khr_frame_copy> images;
  void detachFromRing() {
    if (ctx && slot >= 0) {
      khr_frame_copy* fc = nullptr;
      if (khr_frame_copy_create(ctx, slot, &fc) == 0 && fc) images = std::shared_ptr<khr_frame_copy>(fc, [](khr_frame_copy* p) { khr_frame_copy_release(p); });
    }
    slot_lease.reset();
    slot = -1;
    ctx = nullptr;
  }
  const Sensor& getSensor() const { return sensor; }
  const double* getSensorPose() const { return world_T_sensor; }
  size_t numPixels() const { return static_cast<size_t>(sensor.width) * sensor.height; }
  // host copies of the normalised images (InputData::range_image, ::vertex_map, ::depth_image, ::color_image, ::label_image); empty
  // when neither a slot nor a copy is held
  std::vector<float> rangeImage() const {
    std::vector<float> r(numPixels());
    if (ctx && slot >= 0) khr_download_frame(ctx, slot, r.data(), nullptr, nullptr);
    else if (!images || khr_frame_copy_download(images.get(), nullptr, r.data(), nullptr, nullptr, nullptr) != 0) r.clear();
    return r;
  }
  std::vector<float> vertexMap() const {
    std::vector<float> v(numPixels() * 3);
    if (ctx && slot >= 0) khr_download_frame(ctx, slot, nullptr, v.data(), nullptr);
    else if (!images || khr_frame_copy_download(images.get(), nullptr, nullptr, nullptr, nullptr, v.data()) != 0) v.clear();
    return v;
  }
  std::vector<float> depthImage() const {
    std::vector<float> d(numPixels());
    if (!images || khr_frame_copy_download(images.get(), d.data(), nullptr, nullptr, nullptr, nullptr) != 0) d.clear();
    return d;
  }
  std::vector<uint8_t> colorImage() const {  // rgb8
    std::vector<uint8_t> c(numPixels() * 3);
    if (!images || khr_frame_copy_download(images.get(), nullptr, nullptr, c.data(), nullptr, nullptr) != 0) c.clear();
    return c;
  }
  std::vector<int32_t> labelImage() const {
    std::vector<int32_t> l(numPixels());
    if (!images || khr_frame_copy_download(images.get(), nullptr, nullptr, nullptr, l.data(), nullptr) != 0) l.clear();
    return l;
  }
};

// a voxel block copied to the host (VolumetricMap::cloneUpdated role, active_window.cpp:229)
struct BlockCopy {
  BlockIndex index;
  std::vector<float> distance, weight;
  std::vector<uint8_t> color;  // rgba
  std::vector<uint64_t> last_observed, last_occupied;
  std::vector<uint8_t> flags;
  std::vector<uint32_t> semantic_label;
  uint8_t block_flags = 0;
};

// ---- map slices (ActiveWindowVisualizer::visualize{EverFree,Tracking,Tsdf}Slice, active_window_visualizer.cpp:345-520) ----
// getVoxelKey((0, 0, height)).z as a global voxel index (ASSUMPTIONS.md A.10): the block floor, then the voxel floor inside the
// block (A.1), in float.  A local index of -1 / vps that rounding produces is kept: bz * vps + v then names the edge voxel of the
// neighbouring layer, the voxel the height lies in to within that rounding.  Same rule as khr_slice_voxel_z and
// khronos_amd.capi.slice_voxel_z.
inline int64_t sliceVoxelZ(float height, float voxel_size, int voxels_per_side) {
  const float bs = voxel_size * static_cast<float>(voxels_per_side), bs_inv = 1.f / bs, vs_inv = 1.f / voxel_size;
  const int64_t bz = static_cast<int64_t>(std::floor(height * bs_inv));
  const float origin = static_cast<float>(bz) * bs;
  const int64_t v = static_cast<int64_t>(std::floor((height - origin) * vs_inv));
  return bz * voxels_per_side + v;
}

// The visualizer's slice height: slice_height, plus world_T_body.z when slice_height_is_relative (:114, :364-367; config keys :71-73)
struct SliceConfig {
  float slice_height = -0.5f;  // (khronos_ros/config/mapper/uHumans2.yaml)
  bool slice_height_is_relative = true;
  bool show_unknown_voxels = false;
  float height(const double* world_T_body) const {
    float h = slice_height;
    if (slice_height_is_relative) h += static_cast<float>(world_T_body[11]);
    return h;
  }
};

// One z-plane of the live map (VolumetricMap::slice): every live block on the layer, sorted by (bx, by), its vps x vps voxels at
// the plane x-outer / y-inner (voxel i of block k is entry k * vps^2 + x * vps + y).
struct MapSlice {
  int64_t voxel_z = 0;
  int voxels_per_side = 0;
  std::vector<int32_t> block_xy;     // 2 per block
  std::vector<float> positions;      // voxel centres, 3 per voxel
  std::vector<float> distance, weight;
  std::vector<uint64_t> last_observed;
  std::vector<uint8_t> flags;        // KHR_VOX_* bits
  size_t size() const { return distance.size(); }
  size_t numBlocks() const { return block_xy.size() / 2; }
};

// What the visualizer draws for a slice, as scalars (the colormaps are Hydra's): the slice voxels it keeps, in its order, with
// their class and value.
enum class SliceClass : uint8_t {
  kUnknown = 0,   // gray
  kFree = 1,      // ever-free slice: green
  kOccupied = 2,  // ever-free slice: red
  kTooOld = 3,    // tracking slice: age above max_age (black)
  kValue = 4,     // tracking slice: age; TSDF slice: 0.5 + 0.5 * distance / truncation (colormap input)
};
struct SlicePoints {
  std::vector<uint32_t> voxel;  // entry of the MapSlice (its position: MapSlice::positions[3 * voxel])
  std::vector<SliceClass> cls;
  std::vector<float> value;     // kValue only (0 otherwise)
  void add(uint32_t v, SliceClass c, float x = 0.f) {
    voxel.push_back(v);
    cls.push_back(c);
    value.push_back(x);
  }
  bool operator==(const SlicePoints& o) const {
    return voxel == o.voxel && cls == o.cls && value.size() == o.value.size() &&
           (value.empty() || std::memcmp(value.data(), o.value.data(), value.size() * sizeof(float)) == 0);
  }
};
// visualizeEverFreeSlice (:382-397): unknown iff last_observed == 0 (drawn only with show_unknown_voxels), else free / occupied by
// the ever-free bit
inline SlicePoints everFreeSlice(const MapSlice& s, bool show_unknown_voxels) {
  SlicePoints r;
  for (size_t i = 0; i < s.size(); ++i) {
    const bool unknown = s.last_observed[i] == 0u;
    if (unknown && !show_unknown_voxels) continue;
    r.add(static_cast<uint32_t>(i), unknown ? SliceClass::kUnknown : ((s.flags[i] & KHR_VOX_EVER_FREE) ? SliceClass::kFree : SliceClass::kOccupied));
  }
  return r;
}
// visualizeTrackingSlice (:443-459): age = stamp_s - toSeconds(last_observed) in double, then float (:453); above max_age = 3 its own class
inline SlicePoints trackingSlice(const MapSlice& s, TimeStamp stamp_ns, bool show_unknown_voxels) {
  SlicePoints r;
  const double stamp_s = toSeconds(stamp_ns);
  constexpr float max_age = 3;
  for (size_t i = 0; i < s.size(); ++i) {
    const bool unknown = s.last_observed[i] == 0u;
    if (unknown && !show_unknown_voxels) continue;
    if (unknown) {
      r.add(static_cast<uint32_t>(i), SliceClass::kUnknown);
      continue;
    }
    const float age = static_cast<float>(stamp_s - toSeconds(s.last_observed[i]));
    if (age > max_age) r.add(static_cast<uint32_t>(i), SliceClass::kTooOld);
    else r.add(static_cast<uint32_t>(i), SliceClass::kValue, age);
  }
  return r;
}
// visualizeTsdfSlice (:500-512): every voxel; unknown iff weight < 1e-6, else value = 0.5 + 0.5 * d / truncation in double (:508-511)
inline SlicePoints tsdfSlice(const MapSlice& s, float truncation_distance) {
  SlicePoints r;
  for (size_t i = 0; i < s.size(); ++i) {
    if (s.weight[i] < 1e-6) r.add(static_cast<uint32_t>(i), SliceClass::kUnknown);
    else r.add(static_cast<uint32_t>(i), SliceClass::kValue, static_cast<float>(0.5 + 0.5 * s.distance[i] / truncation_distance));
  }
  return r;
}

// The live map seen from a pose (VolumetricMap::render, khr_render_view; ASSUMPTIONS.md A.12): W x H row-major images.  A pixel
// whose status is not kHit is zero in every image.
struct RenderedView {
  enum Status : uint8_t { kNone = 0, kHit = 1, kBlocked = 2 };
  int width = 0, height = 0;
  std::vector<float> depth;      // z-depth of the hit, metres
  std::vector<float> normal;     // 3 per pixel, world frame
  std::vector<uint8_t> color;    // rgba per pixel
  std::vector<uint32_t> label;   // 0 without semantics
  std::vector<uint8_t> flags;    // KHR_VOX_* bits of the voxel the hit lies in
  std::vector<uint8_t> status;
  khr_render_stats stats{};
  size_t numPixels() const { return status.size(); }
};

// The live map at world points (VolumetricMap::query, khr_query_points; ASSUMPTIONS.md A.13): one entry per point.  Every value
// of a point whose status bit is clear is zero.
struct PointSamples {
  enum Status : uint8_t { kValue = KHR_QP_VALUE, kGradient = KHR_QP_GRADIENT, kVoxel = KHR_QP_VOXEL };
  std::vector<float> distance;          // trilinear signed distance, metres (kValue)
  std::vector<float> gradient;          // 3 per point: d(distance) / d(metres), not normalised (kGradient)
  std::vector<float> weight;            // of the voxel the point lies in, not interpolated (kVoxel, as the four below)
  std::vector<uint8_t> color;           // rgba per point
  std::vector<uint32_t> label;          // 0 without semantics
  std::vector<uint8_t> flags;           // KHR_VOX_* bits
  std::vector<uint64_t> last_observed;  // 0 without tracking
  std::vector<uint8_t> status;
  khr_query_stats stats{};
  size_t size() const { return status.size(); }
  bool hasValue(size_t i) const { return (status[i] & kValue) != 0; }
  bool hasGradient(size_t i) const { return (status[i] & kGradient) != 0; }
  bool hasVoxel(size_t i) const { return (status[i] & kVoxel) != 0; }
};

// A frame or a point set registered against the live map (VolumetricMap::align, khr_align_frame; ASSUMPTIONS.md A.14).  `found`
// false: the map did not constrain the pose (too few inliers or a singular system) and world_T_source is the prior -- keep it.
struct AlignOptions {
  int stride = 4;            // depth form: every stride-th pixel of every stride-th row
  float gate = 0.f;          // largest |distance| of an inlier, metres; 0 = the truncation distance
  float huber_delta = 0.f;   // metres; 0 = no robust factor
  float min_weight = 0.f;    // 0 = the mesh's minimum weight
  khr_align_options solver{10, 64, 1e-4, 1e-5, 1e-5};  // max_iterations, min_inliers, lambda, eps_rot, eps_trans
};
struct Alignment {
  double world_T_source[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  bool found = false;
  int iterations = 0;  // updates applied
  bool converged = false;
  uint64_t n_inlier_first = 0, n_inlier_last = 0;
  double rmse_first = 0, rmse_last = 0;  // sqrt(sum w rho d^2 / sum w rho) over the inliers of the first / last linearisation
  double H[21] = {}, b[6] = {};          // the last linearisation's normal equations: H's upper triangle row by row, undamped
  // H as a full 6 x 6 row-major matrix, twist order (omega, v): the information matrix of the pose up to the residual's variance
  std::array<double, 36> information() const {
    std::array<double, 36> m{};
    int k = 0;
    for (int r = 0; r < 6; ++r)
      for (int c = r; c < 6; ++c, ++k) m[6 * r + c] = m[6 * c + r] = H[k];
    return m;
  }
};

// The distance-field stage of the reference's mapper configuration (freespace_places of khronos_ros/config/mapper/*.yaml: the
// active window's TSDF, downsampled by `ratio`, goes into a distance transform with these parameters; the stage itself is
// un-vendored Hydra).  fromYaml takes the mapper file's root node (freespace_places under `frontend`), or the node that holds
// freespace_places itself.
struct DistanceFieldConfig {
  float max_distance_m = 1.f;
  float min_weight = 0.f;  // 0 = the mesh's minimum weight
  bool positive_distance_only = false;
  int ratio = 1;
  static DistanceFieldConfig fromYaml(const khronos_amd::YamlNode& root) {
    DistanceFieldConfig c;
    const khronos_amd::YamlNode* fp = root.find("freespace_places");
    if (!fp)
      if (const khronos_amd::YamlNode* fe = root.find("frontend")) fp = fe->find("freespace_places");
    if (!fp) return c;
    if (const khronos_amd::YamlNode* gvd = fp->find("gvd")) {
      if (gvd->has("max_distance_m")) gvd->read("max_distance_m", c.max_distance_m);
      if (gvd->has("min_weight")) gvd->read("min_weight", c.min_weight);
      if (gvd->has("positive_distance_only")) gvd->read("positive_distance_only", c.positive_distance_only);
    }
    if (const khronos_amd::YamlNode* ti = fp->find("tsdf_interpolator"))
      if (ti->has("ratio")) ti->read("ratio", c.ratio);
    return c;
  }
};

// What to compute (VolumetricMap::distanceField): the box in cells of `ratio` voxels, first cell and cells per axis.
struct DistanceFieldRequest {
  std::array<int32_t, 3> origin{0, 0, 0}, dims{1, 1, 1};
  int ratio = 1;
  float min_weight = 0.f;        // 0 = the mesh's minimum weight
  float max_distance = 1.f;      // metres
  float surface_distance = 0.f;  // a cell is an obstacle iff its least observed distance is <= this
  bool unknown_is_obstacle = false;
  bool positive_only = false;
  DistanceFieldRequest() = default;
  DistanceFieldRequest(const DistanceFieldConfig& c)
      : ratio(c.ratio), min_weight(c.min_weight), max_distance(c.max_distance_m), positive_only(c.positive_distance_only) {}
};

// The exact Euclidean distance field of a box of the live map (khr_distance_field; ASSUMPTIONS.md A.15): one entry per cell in
// the order x + nx * (y + ny * z).  Only the cells of the box take part.
struct DistanceField {
  enum Status : uint8_t { kObserved = KHR_DF_OBSERVED, kObstacle = KHR_DF_OBSTACLE, kInRange = KHR_DF_IN_RANGE };
  std::array<int32_t, 3> origin{0, 0, 0}, dims{0, 0, 0};
  float cell_size = 0.f;
  std::vector<float> distance;  // metres; negative inside obstacles unless positive_only; +-max_distance out of range
  std::vector<int32_t> d2;      // squared cell units; +-KHR_DF_FAR out of range
  std::vector<uint8_t> status;
  khr_df_stats stats{};
  size_t size() const { return status.size(); }
  size_t index(int x, int y, int z) const { return static_cast<size_t>(x) + static_cast<size_t>(dims[0]) * (static_cast<size_t>(y) + static_cast<size_t>(dims[1]) * static_cast<size_t>(z)); }
  // the cell a world point lies in, relative to the box's first cell (may lie outside [0, dims))
  std::array<int32_t, 3> cellOf(float x, float y, float z) const {
    return {static_cast<int32_t>(std::floor(x / cell_size)) - origin[0], static_cast<int32_t>(std::floor(y / cell_size)) - origin[1],
            static_cast<int32_t>(std::floor(z / cell_size)) - origin[2]};
  }
  bool contains(const std::array<int32_t, 3>& c) const { return c[0] >= 0 && c[0] < dims[0] && c[1] >= 0 && c[1] < dims[1] && c[2] >= 0 && c[2] < dims[2]; }
  // world position of the centre of the box's cell (x, y, z)
  std::array<float, 3> centre(int x, int y, int z) const {
    return {(static_cast<float>(origin[0] + x) + 0.5f) * cell_size, (static_cast<float>(origin[1] + y) + 0.5f) * cell_size,
            (static_cast<float>(origin[2] + z) + 0.5f) * cell_size};
  }
};

// The Voronoi parameters of the same stage (freespace_places.gvd.voronoi_config and gvd.min_basis_for_extraction of the mapper
// files): when two neighbouring cells' nearest obstacles count as apart, and how many such obstacles a cell needs to be extracted.
// min_basis is min_basis_for_extraction + 1 (the cell's own obstacle counts here), clamped to 2 .. KHR_VOR_MAX_BASIS.  fromYaml
// takes what DistanceFieldConfig::fromYaml takes; an unknown mode string throws.
struct VoronoiConfig {
  int mode = KHR_VOR_L1_THEN_ANGLE;
  float min_distance_m = 0.f;
  int parent_l1_separation = 20;
  float parent_cos_angle_separation = 0.2f;
  int min_basis_for_extraction = 1;
  int min_basis = 2;
  static int modeFromString(const std::string& name) {
    if (name == "L1") return KHR_VOR_L1;
    if (name == "ANGLE") return KHR_VOR_ANGLE;
    if (name == "L1_THEN_ANGLE") return KHR_VOR_L1_THEN_ANGLE;
    throw std::runtime_error("voronoi_config: unknown mode '" + name + "' (L1, ANGLE, L1_THEN_ANGLE)");
  }
  static int minBasisFor(int min_basis_for_extraction) { return std::min<int>(KHR_VOR_MAX_BASIS, std::max(2, min_basis_for_extraction + 1)); }
  static VoronoiConfig fromYaml(const khronos_amd::YamlNode& root) {
    VoronoiConfig c;
    const khronos_amd::YamlNode* fp = root.find("freespace_places");
    if (!fp)
      if (const khronos_amd::YamlNode* fe = root.find("frontend")) fp = fe->find("freespace_places");
    const khronos_amd::YamlNode* gvd = fp ? fp->find("gvd") : nullptr;
    if (!gvd) return c;
    if (gvd->has("min_basis_for_extraction")) gvd->read("min_basis_for_extraction", c.min_basis_for_extraction);
    c.min_basis = minBasisFor(c.min_basis_for_extraction);
    if (const khronos_amd::YamlNode* vc = gvd->find("voronoi_config")) {
      if (const khronos_amd::YamlNode* m = vc->find("mode")) c.mode = modeFromString(khronos_amd::detail::unquote(khronos_amd::detail::trim(m->scalar)));
      if (vc->has("min_distance_m")) vc->read("min_distance_m", c.min_distance_m);
      if (vc->has("parent_l1_separation")) vc->read("parent_l1_separation", c.parent_l1_separation);
      if (vc->has("parent_cos_angle_separation")) vc->read("parent_cos_angle_separation", c.parent_cos_angle_separation);
    }
    return c;
  }
};

// What to compute (VolumetricMap::voronoiField): DistanceFieldRequest's box and cell classes (positive_only plays no part: only
// the outer transform exists) plus the Voronoi parameters.
struct VoronoiRequest {
  std::array<int32_t, 3> origin{0, 0, 0}, dims{1, 1, 1};
  int ratio = 1;
  float min_weight = 0.f;        // 0 = the mesh's minimum weight
  float max_distance = 1.f;      // metres
  float surface_distance = 0.f;
  bool unknown_is_obstacle = false;
  float min_distance = 0.f;      // metres: nearer cells are no Voronoi cells
  int mode = KHR_VOR_L1_THEN_ANGLE;
  int parent_l1_separation = 20;
  float parent_cos_angle_separation = 0.2f;
  int min_basis = 2;
  VoronoiRequest() = default;
  VoronoiRequest(const DistanceFieldConfig& d, const VoronoiConfig& v)
      : ratio(d.ratio), min_weight(d.min_weight), max_distance(d.max_distance_m), min_distance(v.min_distance_m), mode(v.mode),
        parent_l1_separation(v.parent_l1_separation), parent_cos_angle_separation(v.parent_cos_angle_separation), min_basis(v.min_basis) {}
};

// Nearest obstacle cell and generalized Voronoi cells of a box of the live map (khr_voronoi_field; ASSUMPTIONS.md A.20).  The dense
// arrays hold one entry per cell in the order x + nx * (y + ny * z); the list holds the cells with basis >= min_basis in that order.
struct VoronoiField {
  std::array<int32_t, 3> origin{0, 0, 0}, dims{0, 0, 0};
  float cell_size = 0.f;
  std::vector<float> distance;  // metres; max_distance out of range, 0 in the obstacle set
  std::vector<int32_t> d2;      // squared cell units; KHR_DF_FAR out of range
  std::vector<uint8_t> status;  // DistanceField::Status bits
  std::vector<int32_t> site;    // linear index in the box of the nearest obstacle cell; -1 without one
  std::vector<uint8_t> basis;   // 0 = not eligible, else 1 .. KHR_VOR_MAX_BASIS; a Voronoi cell has >= 2
  std::vector<int32_t> cells;          // 3 per listed cell: its global cell index
  std::vector<float> cell_distance;
  std::vector<uint8_t> cell_basis;
  std::vector<int32_t> cell_sites;     // 3 * KHR_VOR_MAX_BASIS per listed cell: global cell indices, unused entries zero
  khr_voronoi_stats stats{};
  size_t size() const { return status.size(); }
  size_t numListed() const { return cell_basis.size(); }
  size_t index(int x, int y, int z) const { return static_cast<size_t>(x) + static_cast<size_t>(dims[0]) * (static_cast<size_t>(y) + static_cast<size_t>(dims[1]) * static_cast<size_t>(z)); }
  // the box-local cell of a linear index (a site)
  std::array<int32_t, 3> cellAt(int32_t linear) const { return {linear % dims[0], (linear / dims[0]) % dims[1], linear / (dims[0] * dims[1])}; }
};

// The graph parameters of the same stage (freespace_places.graph, filter_places and min_places_component_size of the mapper files):
// how far a place reaches, how near an obstacle it may lie, and which islands of places are dropped.  compressionFor turns
// compression_distance_m into cells of the field: floor(distance / cell size), clamped to 1 .. KHR_PL_MAX_COMPRESSION (the
// reference's 1.5 m over cells of 0.2 m gives 7).  Without filter_places every component is kept.
struct PlacesConfig {
  float compression_distance_m = 1.0f;
  float min_node_distance_m = 0.f;
  bool filter_places = false;
  int min_places_component_size = 1;
  static PlacesConfig fromYaml(const khronos_amd::YamlNode& root) {
    PlacesConfig c;
    const khronos_amd::YamlNode* fp = root.find("freespace_places");
    if (!fp)
      if (const khronos_amd::YamlNode* fe = root.find("frontend")) fp = fe->find("freespace_places");
    if (!fp) return c;
    if (fp->has("filter_places")) fp->read("filter_places", c.filter_places);
    if (fp->has("min_places_component_size")) fp->read("min_places_component_size", c.min_places_component_size);
    if (const khronos_amd::YamlNode* g = fp->find("graph")) {
      if (g->has("compression_distance_m")) g->read("compression_distance_m", c.compression_distance_m);
      if (g->has("min_node_distance_m")) g->read("min_node_distance_m", c.min_node_distance_m);
    }
    return c;
  }
  int compressionFor(float cell_size) const {
    return std::min<int>(KHR_PL_MAX_COMPRESSION, std::max(1, static_cast<int>(std::floor(compression_distance_m / cell_size))));
  }
  int minComponentSize() const { return filter_places ? std::max(1, min_places_component_size) : 1; }
  // the request for a field of `cell_size` metres per cell; min_basis as VoronoiConfig gives it
  khr_places_request request(float cell_size, int min_basis = 0) const {
    khr_places_request rq{};
    rq.min_basis = min_basis, rq.min_node_distance = min_node_distance_m, rq.compression = compressionFor(cell_size), rq.min_component_size = minComponentSize();
    return rq;
  }
};

// Places and their links from the Voronoi cells of the last voronoiField (khr_places_graph; ASSUMPTIONS.md A.21): one row per kept
// place and per kept edge, and the kept place of every cell of that field's box (-1 for none).
struct PlacesGraph {
  std::vector<int32_t> place;       // per cell of the box, x + nx * (y + ny * z)
  std::vector<int32_t> centre;      // 3 per place: global cell
  std::vector<int32_t> centre_d2;
  std::vector<float> radius;        // metres: the centre's distance
  std::vector<uint8_t> basis;
  std::vector<int32_t> site;        // 3 per place: the centre's nearest obstacle cell, global
  std::vector<uint32_t> n_cells;
  std::vector<int64_t> sum;         // 3 per place: the members' global cells summed
  std::vector<uint32_t> degree, component;
  std::vector<uint32_t> edge_a, edge_b;
  std::vector<int32_t> edge_clearance_d2;
  std::vector<uint32_t> edge_n_contacts;
  khr_places_stats stats{};
  size_t numPlaces() const { return n_cells.size(); }
  size_t numEdges() const { return edge_a.size(); }
  // the mean of a place's member cells, in cells
  std::array<double, 3> centroid(size_t p) const {
    const double n = static_cast<double>(n_cells[p]);
    return {static_cast<double>(sum[3 * p]) / n, static_cast<double>(sum[3 * p + 1]) / n, static_cast<double>(sum[3 * p + 2]) / n};
  }
};

// What a body needs to move through the free space of the same stage (freespace_places.travel; this library's keys, the reference
// has no counterpart): clearance_m, the body's radius; connectivity 6, 18 or 26 (anything else throws); allow_unknown, whether
// unobserved cells may be crossed; max_distance_m, how far to look (0 = everywhere), which maxCostFor turns into move cost: 10 per
// cell along an axis.
struct TravelConfig {
  float clearance_m = 0.f;
  int connectivity = 26;
  bool allow_unknown = false;
  float max_distance_m = 0.f;
  static TravelConfig fromYaml(const khronos_amd::YamlNode& root) {
    TravelConfig c;
    const khronos_amd::YamlNode* fp = root.find("freespace_places");
    if (!fp)
      if (const khronos_amd::YamlNode* fe = root.find("frontend")) fp = fe->find("freespace_places");
    const khronos_amd::YamlNode* t = fp ? fp->find("travel") : nullptr;
    if (!t) return c;
    if (t->has("clearance_m")) t->read("clearance_m", c.clearance_m);
    if (t->has("connectivity")) t->read("connectivity", c.connectivity);
    if (t->has("allow_unknown")) t->read("allow_unknown", c.allow_unknown);
    if (t->has("max_distance_m")) t->read("max_distance_m", c.max_distance_m);
    if (c.connectivity != 6 && c.connectivity != 18 && c.connectivity != 26)
      throw std::runtime_error("freespace_places.travel.connectivity is " + std::to_string(c.connectivity) + ": 6, 18 or 26");
    return c;
  }
  uint32_t maxCostFor(float cell_size) const {
    return max_distance_m > 0.f ? static_cast<uint32_t>(std::max(1.0, std::round(10.0 * static_cast<double>(max_distance_m) / static_cast<double>(cell_size)))) : 0u;
  }
  // the request for a field of `cell_size` metres per cell
  khr_travel_request request(float cell_size) const {
    khr_travel_request rq{};
    rq.clearance = clearance_m, rq.connectivity = connectivity, rq.allow_unknown = allow_unknown ? 1 : 0, rq.max_cost = maxCostFor(cell_size);
    return rq;
  }
};

// Travel cost, nearest goal by travel and the step towards it for every cell of the last voronoiField's box (khr_travel_field;
// ASSUMPTIONS.md A.22), in the order x + nx * (y + ny * z).
struct TravelField {
  std::array<int32_t, 3> origin{0, 0, 0}, dims{0, 0, 0};
  std::vector<uint32_t> cost;   // KHR_TF_UNREACHED where no goal reaches
  std::vector<int32_t> goal;    // index into the goals given; -1 unreached
  std::vector<uint8_t> parent;  // (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of the next cell towards the goal; 13 at a goal, 255 unreached
  khr_travel_stats stats{};
  size_t size() const { return cost.size(); }
  bool contains(const std::array<int32_t, 3>& cell) const {
    for (int a = 0; a < 3; ++a)
      if (cell[a] < origin[a] || cell[a] >= origin[a] + dims[a]) return false;
    return true;
  }
  size_t index(const std::array<int32_t, 3>& cell) const {
    return static_cast<size_t>(cell[0] - origin[0]) + static_cast<size_t>(dims[0]) * (static_cast<size_t>(cell[1] - origin[1]) + static_cast<size_t>(dims[1]) * static_cast<size_t>(cell[2] - origin[2]));
  }
  bool reached(const std::array<int32_t, 3>& cell) const { return contains(cell) && cost[index(cell)] != KHR_TF_UNREACHED; }
};

// The paths of VolumetricMap::travelPaths: path i is cells[3 * offsets[i] .. 3 * offsets[i + 1]), global cells from the start to its
// goal, both included; empty, with cost KHR_TF_UNREACHED and goal -1, for a start outside the box or unreached.
struct TravelPaths {
  std::vector<int64_t> offsets;
  std::vector<int32_t> cells;
  std::vector<uint32_t> path_cost;
  std::vector<int32_t> path_goal;
  size_t numPaths() const { return path_cost.size(); }
  size_t length(size_t i) const { return static_cast<size_t>(offsets[i + 1] - offsets[i]); }
};

// What changed between the live map and another map (VolumetricMap::diff; khr_diff_map, ASSUMPTIONS.md A.18): the changed blocks
// in (x, y, z) order, the changed voxels of a block in ascending linear index.  Per voxel: x, y, z of its global voxel index in
// this map's frame, kind, the two distances, the label of the occupied side and last_observed of either side; per block: its
// index, its two counts and the index of its first entry in the voxel arrays.
struct MapDiff {
  enum Kind : uint8_t { kAppeared = KHR_DIFF_APPEARED, kDisappeared = KHR_DIFF_DISAPPEARED };
  khr_diff_stats stats{};
  std::vector<int32_t> voxels;  // 3 per changed voxel
  std::vector<uint8_t> kind;
  std::vector<float> d_now, d_then;
  std::vector<uint32_t> label;
  std::vector<uint64_t> stamp_now, stamp_then;
  std::vector<int32_t> blocks;  // 3 per changed block
  std::vector<uint32_t> block_appeared, block_disappeared, block_first;
  size_t numVoxels() const { return kind.size(); }
  size_t numBlocks() const { return block_first.size(); }
};

// The connected pieces of matter in the live map (VolumetricMap::segment; khr_segment_map, ASSUMPTIONS.md A.19): the kept
// components in ascending order of their representatives (ids 1, 2, ...: component i has id i + 1) and, where asked for, the
// voxel list grouped by component in ascending id, ascending voxel order inside a component.  Indices are global voxel indices.
struct MapSegments {
  khr_segment_stats stats{};
  std::vector<int32_t> label;
  std::vector<uint64_t> n_voxels;
  std::vector<int32_t> bbox_min, bbox_max;  // 3 per component, inclusive
  std::vector<int64_t> sum;                 // 3 per component
  std::vector<int32_t> representative;      // 3 per component
  std::vector<uint64_t> last_observed_max, first;
  std::vector<int32_t> voxels;  // 3 per listed voxel (empty without the list)
  std::vector<uint32_t> voxel_component;
  size_t numComponents() const { return label.size(); }
  size_t numVoxels() const { return voxel_component.size(); }
  // centre of mass of component i in metres, in double from the exact sums
  std::array<double, 3> centroid(size_t i, double voxel_size) const {
    const double n = static_cast<double>(n_voxels[i]);
    return {(static_cast<double>(sum[3 * i]) / n + 0.5) * voxel_size, (static_cast<double>(sum[3 * i + 1]) / n + 0.5) * voxel_size,
            (static_cast<double>(sum[3 * i + 2]) / n + 0.5) * voxel_size};
  }
};

struct IndexedMesh;  // (below, behind Mesh)

// hydra::VolumetricMap role: here a handle on the HBM-resident map of a fusion context.
class VolumetricMap {
 public:
  struct Config {
    float voxel_size = 0.1f;
    int voxels_per_side = 16;
    float truncation_distance = 0.3f;
    bool with_semantics = false;
    bool with_tracking = true;
  } config;

  VolumetricMap() = default;
  VolumetricMap(const Config& cfg, khr_ctx* ctx) : config(cfg), ctx_(ctx) {}
  bool hasSemantics() const { return config.with_semantics; }
  float blockSize() const { return config.voxel_size * static_cast<float>(config.voxels_per_side); }
  khr_ctx* ctx() const { return ctx_; }
  size_t numBlocks() const { return static_cast<size_t>(khr_num_blocks(ctx_)); }
  // TsdfLayer::allocatedBlockIndices / blockIndicesWithCondition(updated) role (sorted)
  BlockIndices allocatedBlockIndices(bool only_updated = false) const {
    const int64_t n = khr_block_indices(ctx_, nullptr, 0, only_updated);
    BlockIndices out(static_cast<size_t>(n > 0 ? n : 0));
    if (n > 0) khr_block_indices(ctx_, out[0].data(), n, only_updated);
    return out;
  }
  // deep copy of one block of the LIVE map (visualiser / tests; the output's snapshot is ActiveWindowOutput::cloneUpdated)
  BlockCopy cloneBlock(const BlockIndex& idx) const {
    BlockCopy b;
    b.index = idx;
    const size_t n = static_cast<size_t>(config.voxels_per_side) * config.voxels_per_side * config.voxels_per_side;
    b.distance.resize(n); b.weight.resize(n); b.color.resize(4 * n); b.last_observed.resize(n);
    b.last_occupied.resize(n); b.flags.resize(n); b.semantic_label.resize(n);
    khr_download_block(ctx_, idx[0], idx[1], idx[2], b.distance.data(), b.weight.data(), b.color.data(),
                       b.last_observed.data(), b.last_occupied.data(), b.flags.data(), b.semantic_label.data(), nullptr,
                       &b.block_flags);
    return b;
  }
  // one z-plane of the live map, gathered and ordered on the device (khr_map_slice): for sinks that read planes (the
  // visualizer's slices); cloneBlock is for whole blocks
  MapSlice slice(float height) const {
    MapSlice s;
    s.voxel_z = sliceVoxelZ(height, config.voxel_size, config.voxels_per_side);
    s.voxels_per_side = config.voxels_per_side;
    const size_t np = static_cast<size_t>(config.voxels_per_side) * config.voxels_per_side;
    int64_t n = 0;
    for (size_t cap = slice_hint_;; cap = static_cast<size_t>(n)) {
      s.block_xy.resize(2 * (cap / np)); s.positions.resize(3 * cap); s.distance.resize(cap); s.weight.resize(cap);
      s.last_observed.resize(cap); s.flags.resize(cap);
      const int rc = khr_map_slice(ctx_, s.voxel_z, static_cast<int64_t>(cap), s.block_xy.data(), s.positions.data(), s.distance.data(),
                                   s.weight.data(), s.last_observed.data(), s.flags.data(), &n);
      if (rc == KHR_ENOMEM && static_cast<size_t>(n) > cap) continue;
      if (rc != KHR_OK) throw std::runtime_error(std::string("khr_map_slice: ") + khr_last_error());
      break;
    }
    const size_t nv = static_cast<size_t>(n);
    slice_hint_ = nv;
    s.block_xy.resize(2 * (nv / np)); s.positions.resize(3 * nv); s.distance.resize(nv); s.weight.resize(nv);
    s.last_observed.resize(nv); s.flags.resize(nv);
    return s;
  }
  // The map rendered on the device from any pose (khr_render_view): depth, normal, colour, label, voxel flags and hit status per
  // pixel of `sensor` (its min_range / max_range bound the march in z-depth).  step_voxels 0 = half a voxel, min_weight 0 = the
  // mesh's minimum weight.  One call, one host wait.
  RenderedView render(const Sensor& sensor, const double* world_T_sensor, float step_voxels = 0.f, float min_weight = 0.f) const {
    khr_render_request rq{};
    rq.sensor = {sensor.width, sensor.height, sensor.fx, sensor.fy, sensor.cx, sensor.cy, sensor.min_range, sensor.max_range};
    for (int i = 0; i < 16; ++i) rq.world_T_sensor[i] = world_T_sensor[i];
    rq.step_voxels = step_voxels;
    rq.min_weight = min_weight;
    RenderedView v;
    v.width = sensor.width;
    v.height = sensor.height;
    const size_t n = sensor.width > 0 && sensor.height > 0 ? static_cast<size_t>(sensor.width) * sensor.height : 0;
    v.depth.resize(n); v.normal.resize(3 * n); v.color.resize(4 * n); v.label.resize(n); v.flags.resize(n); v.status.resize(n);
    if (khr_render_view(ctx_, &rq, 0, v.depth.data(), v.normal.data(), v.color.data(), v.label.data(), v.flags.data(), v.status.data(),
                        &v.stats) != KHR_OK)
      throw std::runtime_error(std::string("khr_render_view: ") + khr_last_error());
    return v;
  }
  // what the map predicts for a frame: the view from the frame's own pose through its own sensor (a sink's model-to-frame check)
  RenderedView render(const InputData& frame, float step_voxels = 0.f, float min_weight = 0.f) const {
    return render(frame.sensor, frame.world_T_sensor, step_voxels, min_weight);
  }
  // What the map says at world points (khr_query_points): `points` holds x, y, z per point.  min_weight 0 = the mesh's minimum
  // weight.  One call, one host wait, no block copies; cloneBlock is for whole blocks.
  PointSamples query(const std::vector<float>& points, float min_weight = 0.f) const {
    if (points.size() % 3 != 0) throw std::runtime_error("VolumetricMap::query: points must hold 3 floats per point");
    const size_t n = points.size() / 3;
    PointSamples s;
    s.distance.resize(n); s.gradient.resize(3 * n); s.weight.resize(n); s.color.resize(4 * n); s.label.resize(n); s.flags.resize(n);
    s.last_observed.resize(n); s.status.resize(n);
    if (khr_query_points(ctx_, static_cast<int64_t>(n), points.data(), min_weight, 0, s.distance.data(), s.gradient.data(), s.weight.data(),
                         s.color.data(), s.label.data(), s.flags.data(), s.last_observed.data(), s.status.data(), &s.stats) != KHR_OK)
      throw std::runtime_error(std::string("khr_query_points: ") + khr_last_error());
    return s;
  }
  PointSamples query(float x, float y, float z, float min_weight = 0.f) const { return query(std::vector<float>{x, y, z}, min_weight); }
  // Registers a depth image (host memory, sensor.width x sensor.height metres) against the map, starting from `prior`
  // (world_T_sensor, row-major 4 x 4): Gauss-Newton over khr_align_linearize, one host wait per iteration, the map only read.  Call
  // it with the odometry prior before the frame is fused, and fuse with the returned pose.  Throws on a bad request.
  Alignment align(const Sensor& sensor, const float* depth, const double* prior, const AlignOptions& opt = AlignOptions(),
                  const float* weights = nullptr) const {
    khr_align_request rq = alignRequest(prior, opt);
    rq.depth = depth;
    rq.sensor = {sensor.width, sensor.height, sensor.fx, sensor.fy, sensor.cx, sensor.cy, sensor.min_range, sensor.max_range};
    rq.stride = opt.stride;
    rq.weights = weights;
    return alignRun(rq, opt);
  }
  // the same for a converted frame: its depth image is the one the frame slot (or the output's copy) holds
  Alignment align(const InputData& frame, const double* prior, const AlignOptions& opt = AlignOptions()) const {
    std::vector<float> depth = frame.depthImage();
    if (depth.empty() && frame.ctx && frame.slot >= 0) {
      khr_frame_copy* fc = nullptr;
      if (khr_frame_copy_create(frame.ctx, frame.slot, &fc) != 0 || !fc) throw std::runtime_error(std::string("khr_frame_copy_create: ") + khr_last_error());
      depth.resize(frame.numPixels());
      const int rc = khr_frame_copy_download(fc, depth.data(), nullptr, nullptr, nullptr, nullptr);
      khr_frame_copy_release(fc);
      if (rc != 0) throw std::runtime_error(std::string("khr_frame_copy_download: ") + khr_last_error());
    }
    if (depth.empty()) throw std::runtime_error("VolumetricMap::align: the frame's depth image is not available");
    return align(frame.sensor, depth.data(), prior, opt);
  }
  // the same for a point list: x, y, z per point in the source frame, `weights` one per point or empty
  Alignment align(const std::vector<float>& points, const double* prior, const AlignOptions& opt = AlignOptions(),
                  const std::vector<float>& weights = {}) const {
    if (points.size() % 3 != 0) throw std::runtime_error("VolumetricMap::align: points must hold 3 floats per point");
    if (!weights.empty() && weights.size() != points.size() / 3) throw std::runtime_error("VolumetricMap::align: one weight per point");
    khr_align_request rq = alignRequest(prior, opt);
    rq.n = static_cast<int64_t>(points.size() / 3);
    rq.points = points.data();
    rq.weights = weights.empty() ? nullptr : weights.data();
    return alignRun(rq, opt);
  }
  // How far every cell of a box is from the nearest obstacle (khr_distance_field): gathered from the hashed blocks and transformed on
  // the device, exact.  One call, one host wait, no block copies.  Throws on a bad request.
  DistanceField distanceField(const DistanceFieldRequest& request) const {
    khr_df_request rq{};
    for (int a = 0; a < 3; ++a) rq.origin[a] = request.origin[a], rq.dims[a] = request.dims[a];
    rq.ratio = request.ratio;
    rq.min_weight = request.min_weight, rq.max_distance = request.max_distance, rq.surface_distance = request.surface_distance;
    rq.unknown_is_obstacle = request.unknown_is_obstacle ? 1 : 0, rq.positive_only = request.positive_only ? 1 : 0;
    DistanceField f;
    f.origin = request.origin, f.dims = request.dims;
    f.cell_size = config.voxel_size * static_cast<float>(request.ratio);
    size_t n = 1;
    for (int a = 0; a < 3; ++a) n *= request.dims[a] > 0 && request.dims[a] <= KHR_DF_MAX_DIM ? static_cast<size_t>(request.dims[a]) : 0;
    f.distance.resize(n); f.d2.resize(n); f.status.resize(n);
    if (khr_distance_field(ctx_, &rq, 0, f.distance.data(), f.d2.data(), f.status.data(), &f.stats) != KHR_OK)
      throw std::runtime_error(std::string("khr_distance_field: ") + khr_last_error());
    return f;
  }
  // Where the nearest obstacle of every cell of a box is, and which cells lie between obstacles that are apart (khr_voronoi_field):
  // the generalized Voronoi diagram the places graph is extracted from.  Computed on the device; one host wait for the counters, then
  // the arrays are copied.  Throws on a bad request.
  VoronoiField voronoiField(const VoronoiRequest& request) const {
    khr_voronoi_request rq{};
    for (int a = 0; a < 3; ++a) rq.origin[a] = request.origin[a], rq.dims[a] = request.dims[a];
    rq.ratio = request.ratio;
    rq.min_weight = request.min_weight, rq.max_distance = request.max_distance, rq.surface_distance = request.surface_distance;
    rq.unknown_is_obstacle = request.unknown_is_obstacle ? 1 : 0;
    rq.min_distance = request.min_distance, rq.mode = request.mode, rq.parent_l1_separation = request.parent_l1_separation;
    rq.parent_cos_angle_separation = request.parent_cos_angle_separation, rq.min_basis = request.min_basis;
    VoronoiField f;
    f.origin = request.origin, f.dims = request.dims;
    f.cell_size = config.voxel_size * static_cast<float>(request.ratio);
    if (khr_voronoi_field(ctx_, &rq, &f.stats) != KHR_OK) throw std::runtime_error(std::string("khr_voronoi_field: ") + khr_last_error());
    const size_t n = static_cast<size_t>(request.dims[0]) * request.dims[1] * request.dims[2], m = static_cast<size_t>(f.stats.n_listed);
    f.distance.resize(n); f.d2.resize(n); f.status.resize(n); f.site.resize(n); f.basis.resize(n);
    f.cells.resize(3 * m); f.cell_distance.resize(m); f.cell_basis.resize(m); f.cell_sites.resize(3 * KHR_VOR_MAX_BASIS * m);
    if (khr_voronoi_field_into(ctx_, 0, f.distance.data(), f.d2.data(), f.status.data(), f.site.data(), f.basis.data(), f.cells.data(), f.cell_distance.data(),
                               f.cell_basis.data(), f.cell_sites.data()) != KHR_OK)
      throw std::runtime_error(std::string("khr_voronoi_field_into: ") + khr_last_error());
    return f;
  }

  // The places graph of the last voronoiField `field` of this map (khr_places_graph): computed on the device, two host waits for the
  // counts, then the lists are copied.  Throws on a bad request or without a Voronoi field.
  PlacesGraph placesGraph(const VoronoiField& field, const khr_places_request& request) const {
    PlacesGraph g;
    if (khr_places_graph(ctx_, &request, &g.stats) != KHR_OK) throw std::runtime_error(std::string("khr_places_graph: ") + khr_last_error());
    const size_t p = static_cast<size_t>(g.stats.n_places), e = static_cast<size_t>(g.stats.n_edges);
    g.place.resize(field.size());
    g.centre.resize(3 * p); g.centre_d2.resize(p); g.radius.resize(p); g.basis.resize(p); g.site.resize(3 * p); g.n_cells.resize(p); g.sum.resize(3 * p);
    g.degree.resize(p); g.component.resize(p);
    g.edge_a.resize(e); g.edge_b.resize(e); g.edge_clearance_d2.resize(e); g.edge_n_contacts.resize(e);
    if (khr_places_graph_into(ctx_, 0, g.place.data(), g.centre.data(), g.centre_d2.data(), g.radius.data(), g.basis.data(), g.site.data(), g.n_cells.data(),
                              g.sum.data(), g.degree.data(), g.component.data(), g.edge_a.data(), g.edge_b.data(), g.edge_clearance_d2.data(),
                              g.edge_n_contacts.data()) != KHR_OK)
      throw std::runtime_error(std::string("khr_places_graph_into: ") + khr_last_error());
    return g;
  }
  PlacesGraph placesGraph(const VoronoiField& field, const PlacesConfig& config, int min_basis = 0) const {
    return placesGraph(field, config.request(field.cell_size, min_basis));
  }
  // Travel cost from `goals` (3 int32 each, global cells) over the box of the last voronoiField `field` of this map
  // (khr_travel_field): relaxed on the device in rounds, then copied.  Throws on a bad request or without a Voronoi field.
  TravelField travelField(const VoronoiField& field, const std::vector<int32_t>& goals, const khr_travel_request& request) const {
    TravelField t;
    if (khr_travel_field(ctx_, &request, goals.data(), goals.size() / 3, 0, &t.stats) != KHR_OK) throw std::runtime_error(std::string("khr_travel_field: ") + khr_last_error());
    t.origin = field.origin, t.dims = field.dims;
    t.cost.resize(field.size()); t.goal.resize(field.size()); t.parent.resize(field.size());
    if (khr_travel_field_into(ctx_, 0, t.cost.data(), t.goal.data(), t.parent.data()) != KHR_OK)
      throw std::runtime_error(std::string("khr_travel_field_into: ") + khr_last_error());
    return t;
  }
  TravelField travelField(const VoronoiField& field, const std::vector<int32_t>& goals, const TravelConfig& config) const {
    return travelField(field, goals, config.request(field.cell_size));
  }
  // The paths from `starts` (3 int32 each, global cells) to their goals through the last travelField (khr_travel_paths).
  TravelPaths travelPaths(const std::vector<int32_t>& starts) const {
    TravelPaths p;
    uint64_t total = 0;
    const size_t n = starts.size() / 3;
    if (khr_travel_paths(ctx_, n, starts.data(), 0, &total) != KHR_OK) throw std::runtime_error(std::string("khr_travel_paths: ") + khr_last_error());
    p.offsets.resize(n + 1); p.cells.resize(3 * static_cast<size_t>(total)); p.path_cost.resize(n); p.path_goal.resize(n);
    if (khr_travel_paths_into(ctx_, 0, p.offsets.data(), p.cells.data(), p.path_cost.data(), p.path_goal.data()) != KHR_OK)
      throw std::runtime_error(std::string("khr_travel_paths_into: ") + khr_last_error());
    return p;
  }
  // The map save / load role of hydra::VolumetricMap (un-vendored upstream; the reference's own tree has no counterpart): the live
  // map as one checkpoint file (khr_checkpoint_save: the format is in include/khronos_amd.h) and back into an EMPTY map of the
  // same configuration (khr_checkpoint_load; sharded contexts keep their own blocks).  File I/O around the two calls through a
  // page-locked bounce buffer (pageable when that cannot be had).  save returns the file's bytes, load the blocks kept; both
  // throw std::runtime_error with khr_last_error's text.  The mesh layer, the frame ring and the trackers are not part of a
  // checkpoint.  (Defined in active_window.cpp.)
  size_t save(const std::string& path) const;
  size_t load(const std::string& path);
  // The mesh of the last meshing as an indexed mesh: one vertex per cell of a grid of `resolution` metres, the role of the
  // frontend's voxel-grid mesh compression (khr_weld_mesh, ASSUMPTIONS.md A.16).  Welded on the device; the indexed mesh alone
  // crosses to the host.  Throws std::runtime_error with khr_last_error's text.  (Defined below, behind IndexedMesh.)
  IndexedMesh weldedMesh(float resolution) const;
  // Another map fused into this one on the device (voxblox's mergeLayerAintoLayerB role; khr_merge_map, ASSUMPTIONS.md A.17):
  // voxel to voxel under an integer voxel offset, or resampled under a rigid dst_T_src.  `other` is only read.  Returns the
  // statistics; throws std::runtime_error with khr_last_error's text, the map then is as it was.
  struct MergeRequest {
    bool resample = false;
    int32_t voxel_offset[3] = {0, 0, 0};
    double dst_T_src[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float min_weight = 0.f;  // 0 = this map's mesh_min_weight
  };
  khr_merge_stats merge(const VolumetricMap& other, const MergeRequest& request) {
    khr_merge_request rq{};
    rq.mode = request.resample ? KHR_MERGE_RESAMPLE : KHR_MERGE_ALIGNED;
    for (int i = 0; i < 3; ++i) rq.voxel_offset[i] = request.voxel_offset[i];
    for (int i = 0; i < 16; ++i) rq.dst_T_src[i] = request.dst_T_src[i];
    rq.min_weight = request.min_weight;
    khr_merge_stats st{};
    if (khr_merge_map(ctx_, other.ctx_, &rq, &st) != KHR_OK) throw std::runtime_error(std::string("khr_merge_map: ") + khr_last_error());
    return st;
  }
  // This map ("now") compared with another ("then") on the device (khr_diff_map, ASSUMPTIONS.md A.18): the voxels that appeared
  // or vanished, `then` sampled as merge() samples its source.  Neither map is written.  free_distance < 0 = this map's
  // voxel_size; occupied_distance defaults to 0.  Throws std::runtime_error with khr_last_error's text.
  struct DiffRequest {
    bool resample = false;
    int32_t voxel_offset[3] = {0, 0, 0};
    double ctx_T_ref[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float min_weight = 0.f;  // 0 = this map's mesh_min_weight
    float occupied_distance = 0.f;
    float free_distance = -1.f;
  };
  MapDiff diff(const VolumetricMap& then, const DiffRequest& request) const {
    khr_diff_request rq{};
    rq.mode = request.resample ? KHR_MERGE_RESAMPLE : KHR_MERGE_ALIGNED;
    for (int i = 0; i < 3; ++i) rq.voxel_offset[i] = request.voxel_offset[i];
    for (int i = 0; i < 16; ++i) rq.ctx_T_ref[i] = request.ctx_T_ref[i];
    rq.min_weight = request.min_weight;
    rq.occupied_distance = request.occupied_distance;
    rq.free_distance = request.free_distance < 0.f ? config.voxel_size : request.free_distance;
    MapDiff d;
    if (khr_diff_map(ctx_, then.ctx_, &rq, &d.stats) != KHR_OK) throw std::runtime_error(std::string("khr_diff_map: ") + khr_last_error());
    const size_t n = static_cast<size_t>(d.stats.n_appeared + d.stats.n_disappeared), m = static_cast<size_t>(d.stats.n_changed_blocks);
    d.voxels.resize(3 * n); d.kind.resize(n); d.d_now.resize(n); d.d_then.resize(n); d.label.resize(n); d.stamp_now.resize(n);
    d.stamp_then.resize(n); d.blocks.resize(3 * m); d.block_appeared.resize(m); d.block_disappeared.resize(m); d.block_first.resize(m);
    if (khr_diff_map_into(ctx_, 0, d.voxels.data(), d.kind.data(), d.d_now.data(), d.d_then.data(), d.label.data(), d.stamp_now.data(),
                          d.stamp_then.data(), d.blocks.data(), d.block_appeared.data(), d.block_disappeared.data(), d.block_first.data()) != KHR_OK)
      throw std::runtime_error(std::string("khr_diff_map_into: ") + khr_last_error());
    return d;
  }
  // The connected components of this map's occupied voxels on the device (khr_segment_map, ASSUMPTIONS.md A.19).  The map is not
  // written.  by_label < 0 = by label where the map has semantics.  Throws std::runtime_error with khr_last_error's text.
  struct SegmentRequest {
    float min_weight = 0.f;  // 0 = this map's mesh_min_weight
    float surface_distance = 0.f;
    int connectivity = 26;
    int by_label = -1;
    std::vector<int32_t> labels;  // at most 64; empty = every label
    uint32_t flags_require = 0, flags_exclude = 0;
    int64_t min_voxels = 1, max_voxels = 0;  // max_voxels <= 0 = unlimited
    bool want_voxels = true;
  };
  MapSegments segment(const SegmentRequest& request) const {
    khr_segment_request rq{};
    rq.min_weight = request.min_weight;
    rq.surface_distance = request.surface_distance;
    rq.connectivity = request.connectivity;
    khr_config kc{};
    if (request.by_label < 0 && khr_get_config(ctx_, &kc) != KHR_OK) throw std::runtime_error(std::string("khr_get_config: ") + khr_last_error());
    rq.by_label = request.by_label < 0 ? (kc.with_semantics != 0) : request.by_label;
    rq.labels = request.labels.empty() ? nullptr : request.labels.data();
    rq.n_labels = static_cast<int32_t>(request.labels.size());
    rq.flags_require = request.flags_require, rq.flags_exclude = request.flags_exclude;
    rq.min_voxels = request.min_voxels, rq.max_voxels = request.max_voxels;
    rq.want_voxels = request.want_voxels;
    MapSegments s;
    if (khr_segment_map(ctx_, &rq, &s.stats) != KHR_OK) throw std::runtime_error(std::string("khr_segment_map: ") + khr_last_error());
    const size_t m = static_cast<size_t>(s.stats.n_components), n = request.want_voxels ? static_cast<size_t>(s.stats.n_voxels) : 0;
    s.label.resize(m); s.n_voxels.resize(m); s.bbox_min.resize(3 * m); s.bbox_max.resize(3 * m); s.sum.resize(3 * m); s.representative.resize(3 * m);
    s.last_observed_max.resize(m); s.first.resize(m); s.voxels.resize(3 * n); s.voxel_component.resize(n);
    if (khr_segment_map_into(ctx_, 0, s.label.data(), s.n_voxels.data(), s.bbox_min.data(), s.bbox_max.data(), s.sum.data(), s.representative.data(),
                             s.last_observed_max.data(), s.first.data(), request.want_voxels ? s.voxels.data() : nullptr,
                             request.want_voxels ? s.voxel_component.data() : nullptr) != KHR_OK)
      throw std::runtime_error(std::string("khr_segment_map_into: ") + khr_last_error());
    return s;
  }

 private:
  static khr_align_request alignRequest(const double* prior, const AlignOptions& opt) {
    khr_align_request rq{};
    for (int i = 0; i < 16; ++i) rq.world_T_source[i] = prior[i];
    rq.stride = 1;
    rq.min_weight = opt.min_weight;
    rq.gate = opt.gate;
    rq.huber_delta = opt.huber_delta;
    return rq;
  }
  Alignment alignRun(const khr_align_request& rq, const AlignOptions& opt) const {
    Alignment a;
    khr_align_result res{};
    const int rc = khr_align_frame(ctx_, &rq, 0, &opt.solver, a.world_T_source, &res);
    if (rc != KHR_OK && rc != KHR_ENOTFOUND) throw std::runtime_error(std::string("khr_align_frame: ") + khr_last_error());
    a.found = rc == KHR_OK;
    a.iterations = res.iterations;
    a.converged = res.converged != 0;
    a.n_inlier_first = res.n_inlier_first;
    a.n_inlier_last = res.n_inlier_last;
    a.rmse_first = res.rmse_first;
    a.rmse_last = res.rmse_last;
    for (int i = 0; i < 21; ++i) a.H[i] = res.H[i];
    for (int i = 0; i < 6; ++i) a.b[i] = res.b[i];
    return a;
  }
  khr_ctx* ctx_ = nullptr;
  mutable size_t slice_hint_ = 0;  // voxels of the last slice: the first guess of the next call's buffers
};

struct Mesh {
  std::vector<float> points;    // 3 per vertex
  std::vector<uint8_t> colors;  // rgba per vertex
  std::vector<uint32_t> labels;
  std::vector<uint64_t> first_seen_stamps, stamps;
  size_t numVertices() const { return labels.size(); }
};

// a Mesh with explicit faces (VolumetricMap::weldedMesh): 3 vertex indices per face; soup_to_vertex maps every vertex of the
// triangle soup the mesh was welded from to its welded vertex
struct IndexedMesh : Mesh {
  std::vector<uint32_t> faces;
  std::vector<uint32_t> soup_to_vertex;
  khr_weld_stats stats{};
  size_t numFaces() const { return faces.size() / 3; }
};

inline IndexedMesh VolumetricMap::weldedMesh(float resolution) const {
  IndexedMesh m;
  if (khr_weld_mesh(ctx_, resolution, &m.stats) != KHR_OK) throw std::runtime_error(std::string("khr_weld_mesh: ") + khr_last_error());
  const size_t nv = m.stats.n_vertices;
  m.points.resize(3 * nv); m.colors.resize(4 * nv); m.labels.resize(nv); m.first_seen_stamps.resize(nv); m.stamps.resize(nv);
  m.faces.resize(3 * m.stats.n_faces);
  m.soup_to_vertex.resize(m.stats.n_soup_vertices);
  if (khr_weld_mesh_into(ctx_, 0, m.points.data(), m.colors.data(), m.labels.data(), m.first_seen_stamps.data(), m.stamps.data(), m.faces.data(),
                         m.soup_to_vertex.data()) != KHR_OK)
    throw std::runtime_error(std::string("khr_weld_mesh_into: ") + khr_last_error());
  return m;
}

struct BoundingBox {
  float min[3] = {0, 0, 0}, max[3] = {0, 0, 0};
  bool valid = false;
  void merge(const BoundingBox& o) {
    if (!o.valid) return;
    if (!valid) { *this = o; return; }
    for (int i = 0; i < 3; ++i) { min[i] = o.min[i] < min[i] ? o.min[i] : min[i]; max[i] = o.max[i] > max[i] ? o.max[i] : max[i]; }
  }
  void include(const float* p) {
    if (!valid) { for (int i = 0; i < 3; ++i) min[i] = max[i] = p[i]; valid = true; return; }
    for (int i = 0; i < 3; ++i) { if (p[i] < min[i]) min[i] = p[i]; if (p[i] > max[i]) max[i] = p[i]; }
  }
  float dimension(int i) const { return max[i] - min[i]; }
  float center(int i) const { return 0.5f * (min[i] + max[i]); }
  float volume() const { return valid ? dimension(0) * dimension(1) * dimension(2) : 0.f; }
  float maxDimension() const { float m = dimension(0); for (int i = 1; i < 3; ++i) if (dimension(i) > m) m = dimension(i); return m; }
};

// spark_dsg::KhronosObjectAttributes role (fields set at mesh_object_extractor.cpp:81-118,268-302)
struct KhronosObjectAttributes {
  Mesh mesh;
  BoundingBox bounding_box;
  int semantic_label = -1;
  std::vector<float> semantic_feature;
  std::vector<TimeStamp> first_observed_ns, last_observed_ns;
  double position[3] = {0, 0, 0};
  // dynamic objects (mesh_object_extractor.cpp:120-172)
  std::vector<std::array<float, 3>> trajectory_positions;
  std::vector<TimeStamp> trajectory_timestamps;
};

// hydra::ActiveWindowOutput role (fields set at active_window.cpp:225-247)
struct ActiveWindowOutput {
  using Ptr = std::shared_ptr<ActiveWindowOutput>;
  TimeStamp timestamp_ns = 0;
  double world_t_body[3] = {0, 0, 0};
  double world_R_body[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  BlockIndices archived_mesh_indices;
  // setMap(map.cloneUpdated()) (active_window.cpp:229): a device-side SNAPSHOT of the blocks flagged updated, taken between
  // meshing and archival (khr_snapshot_updated).  It keeps its contents whatever later frames do to the map -- the hydra
  // frontend takes outputs from a queue -- and costs no host round trip at output time; indices and voxels come to the
  // host when a consumer asks.  Released with the last copy of the output.
  std::shared_ptr<khr_snapshot> map;
  khr_ctx* map_ctx = nullptr;  // the live map the snapshot was taken from (voxels_per_side etc. via khr_get_config)
  std::shared_ptr<InputData> sensor_data;
  std::vector<std::shared_ptr<KhronosObjectAttributes>> graph_update;  // LayerUpdate(2) role

  void setMap(khr_snapshot* snap) { map = std::shared_ptr<khr_snapshot>(snap, [](khr_snapshot* s) { khr_snapshot_release(s); }); }
  // indices of the snapshot's blocks, sorted (TsdfLayer::allocatedBlockIndices of the cloned map)
  const BlockIndices& updatedBlocks() const {
    if (!indices_valid_) {
      const int64_t n = map ? khr_snapshot_num_blocks(map.get()) : 0;
      if (n < 0) throw std::runtime_error(std::string("ActiveWindowOutput: the map snapshot was never produced: ") + khr_last_error());
      updated_blocks_.assign(static_cast<size_t>(n > 0 ? n : 0), BlockIndex{0, 0, 0});
      // (fails when more blocks were updated than the snapshot holds -- max_snapshot_blocks: the clone is incomplete and says so)
      if (n > 0 && khr_snapshot_download(map.get(), updated_blocks_[0].data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n) < 0) {
        updated_blocks_.clear();
        throw std::runtime_error(std::string("ActiveWindowOutput::updatedBlocks: ") + khr_last_error());
      }
      std::sort(updated_blocks_.begin(), updated_blocks_.end());
      indices_valid_ = true;
    }
    return updated_blocks_;
  }
  // the cloned blocks (all snapshotted layers, or distance / weight only) in ONE packed transfer
  std::vector<BlockCopy> cloneUpdated(bool tsdf_only = false) const {
    std::vector<BlockCopy> out;
    const int64_t n = map ? khr_snapshot_num_blocks(map.get()) : 0;
    if (n <= 0) return out;
    khr_config cfg{};
    khr_get_config(map_ctx, &cfg);
    const size_t nv = static_cast<size_t>(cfg.voxels_per_side) * cfg.voxels_per_side * cfg.voxels_per_side, N = static_cast<size_t>(n);
    std::vector<int32_t> idx(3 * N);
    std::vector<float> d(N * nv), w(N * nv);
    std::vector<uint8_t> col, fl;
    std::vector<uint64_t> lo;
    std::vector<uint32_t> lab;
    if (!tsdf_only) { col.resize(4 * N * nv); fl.resize(N * nv); lo.resize(N * nv); lab.resize(N * nv); }
    const int64_t k = khr_snapshot_download(map.get(), idx.data(), d.data(), w.data(), tsdf_only ? nullptr : col.data(),
                                            tsdf_only ? nullptr : lo.data(), tsdf_only ? nullptr : fl.data(),
                                            tsdf_only ? nullptr : lab.data(), n);
    if (k < 0) throw std::runtime_error(std::string("ActiveWindowOutput::cloneUpdated: ") + khr_last_error());
    for (int64_t i = 0; i < k; ++i) {
      BlockCopy b;
      b.index = {idx[3 * i], idx[3 * i + 1], idx[3 * i + 2]};
      b.distance.assign(d.begin() + i * nv, d.begin() + (i + 1) * nv);
      b.weight.assign(w.begin() + i * nv, w.begin() + (i + 1) * nv);
      if (!tsdf_only) {
        b.color.assign(col.begin() + 4 * i * nv, col.begin() + 4 * (i + 1) * nv);
        b.last_observed.assign(lo.begin() + i * nv, lo.begin() + (i + 1) * nv);
        b.flags.assign(fl.begin() + i * nv, fl.begin() + (i + 1) * nv);
        b.semantic_label.assign(lab.begin() + i * nv, lab.begin() + (i + 1) * nv);
      }
      b.block_flags = 1;  // KHR_BLK_UPDATED: what made it part of the clone
      out.push_back(std::move(b));
    }
    std::sort(out.begin(), out.end(), [](const BlockCopy& a, const BlockCopy& b) { return a.index < b.index; });
    return out;
  }
  std::vector<BlockCopy> cloneUpdatedTsdf() const { return cloneUpdated(true); }
  // true when the output updated more blocks than its snapshot could hold (config max_snapshot_blocks): updatedBlocks() /
  // cloneUpdated() of such an output throw instead of handing out a partial clone
  bool mapOverflowed() const {
    if (!map) return false;
    khr_config cfg{};
    if (khr_get_config(map_ctx, &cfg) < 0) return false;
    const int64_t n = khr_snapshot_num_blocks(map.get());
    const int64_t cap = snapshot_capacity > 0 ? snapshot_capacity : (cfg.max_snapshot_blocks ? cfg.max_snapshot_blocks : 8192);
    return n > cap;
  }
  int64_t snapshot_capacity = 0;  // set by the producer (ActiveWindow::extractOutputData)

 private:
  mutable BlockIndices updated_blocks_;
  mutable bool indices_valid_ = false;
};


// ---- hydra::ActiveWindowModule role (the base class of khronos::ActiveWindow, active_window.h:67) ---------------------------
// The Hydra module owns the output queue and the module thread: the thread takes an InputPacket, calls the protected
// virtual spinOnce and pushes a non-null result to the queue (the hydra frontend pops it later: hence the snapshot in
// ActiveWindowOutput::map).  The stand-in keeps exactly that surface: constructor (config, output queue), virtual
// printInfo, protected pure-virtual spinOnce, and `step` as the body of the module thread's loop.
template <typename T>
struct InputQueue {  // hydra::InputQueue role (a mutex-guarded deque)
  using Ptr = std::shared_ptr<InputQueue<T>>;
  void push(const T& v) {
    std::lock_guard<std::mutex> lock(mutex);
    queue.push_back(v);
  }
  bool pop(T* out) {
    std::lock_guard<std::mutex> lock(mutex);
    if (queue.empty()) return false;
    *out = queue.front();
    queue.erase(queue.begin());
    return true;
  }
  size_t size() const {
    std::lock_guard<std::mutex> lock(mutex);
    return queue.size();
  }
  mutable std::mutex mutex;
  std::vector<T> queue;
};

class ActiveWindowModule {
 public:
  using OutputQueue = InputQueue<ActiveWindowOutput::Ptr>;
  ActiveWindowModule(const OutputQueue::Ptr& output_queue) : output_queue_(output_queue) {}
  virtual ~ActiveWindowModule() = default;
  virtual std::string printInfo() const { return ""; }
  // one iteration of the module thread (hydra: ActiveWindowModule::spin): process a packet, queue the output if there is one
  ActiveWindowOutput::Ptr step(const InputPacket& input) {
    ActiveWindowOutput::Ptr out = spinOnce(input);
    if (out && output_queue_) output_queue_->push(out);
    return out;
  }
  const OutputQueue::Ptr& outputQueue() const { return output_queue_; }

 protected:
  virtual ActiveWindowOutput::Ptr spinOnce(const InputPacket& input) = 0;
  OutputQueue::Ptr output_queue_;
};

// config_utilities string factory role (config::RegistrationWithConfig<Base, Derived, Config, Args...>(name) /
// config::createFromYaml): the pipeline selects the active window by `active_window: {type: "<name>", ...}`
// (uHumans2.yaml:35-36; registration at active_window.h:190-192).  The creator receives the text of the `active_window:`
// mapping's document and the output queue.
class ActiveWindowFactory {
 public:
  using Creator = std::function<std::unique_ptr<ActiveWindowModule>(const std::string& yaml_text, const ActiveWindowModule::OutputQueue::Ptr&)>;
  static bool add(const std::string& type, Creator c) {
    registry()[type] = std::move(c);
    return true;
  }
  static bool has(const std::string& type) { return registry().count(type) != 0; }
  static std::unique_ptr<ActiveWindowModule> create(const std::string& type, const std::string& yaml_text,
                                                    const ActiveWindowModule::OutputQueue::Ptr& queue) {
    auto it = registry().find(type);
    return it == registry().end() ? nullptr : it->second(yaml_text, queue);
  }

 private:
  static std::map<std::string, Creator>& registry() {
    static std::map<std::string, Creator> r;
    return r;
  }
};
// config::RegistrationWithConfig<ActiveWindowModule, Derived, Derived::Config, OutputQueue::Ptr>(name) role: a static
// member of this type inside Derived registers it (the creator is only instantiated once Derived is complete)
template <typename Derived>
struct ActiveWindowRegistration {
  explicit ActiveWindowRegistration(const std::string& name) {
    ActiveWindowFactory::add(name, [](const std::string& yaml_text, const ActiveWindowModule::OutputQueue::Ptr& queue) {
      return std::unique_ptr<ActiveWindowModule>(new Derived(Derived::Config::fromYamlString(yaml_text), queue));
    });
  }
};


// ---- hydra::timing (ElapsedTimeRecorder / ScopedTimer role) ------------------------------------------------------------
// The reference brackets its stages with `Timer timer("<scope>", stamp)` (active_window.cpp:121,152,204,220,269;
// tracking_integrator.cpp:72; free_space_motion_detector.cpp:75; connected_semantics.cpp:61; max_iou_tracker.cpp:200,217)
// and dumps `timing/stats.csv` at shutdown (khronos_ros/src/experiments/experiment_manager.cpp:251-258).  Same scope
// names here, so that a CPU-vs-GPU comparison reads the same rows.  The device work of a scope is asynchronous: with
// `ElapsedTimeRecorder::instance().sync_device = fn` set (the ActiveWindow sets it when config.timing_sync_device is on)
// a scope's end first waits for the device, which makes "active_window/all" the per-frame latency the reference measures.
namespace timing {
struct TimerStats {
  uint64_t count = 0;
  double sum = 0.0, sum_sq = 0.0, min = 0.0, max = 0.0, last = 0.0;
};
class ElapsedTimeRecorder {
 public:
  static ElapsedTimeRecorder& instance() {
    static ElapsedTimeRecorder r;
    return r;
  }
  void record(const std::string& name, double seconds) {
    std::lock_guard<std::mutex> lock(mutex_);
    TimerStats& t = stats_[name];
    if (t.count == 0) t.min = t.max = seconds;
    t.min = std::min(t.min, seconds);
    t.max = std::max(t.max, seconds);
    t.sum += seconds;
    t.sum_sq += seconds * seconds;
    t.last = seconds;
    ++t.count;
  }
  std::map<std::string, TimerStats> stats() const {
    std::lock_guard<std::mutex> lock(mutex_);
    return stats_;
  }
  void reset() {
    std::lock_guard<std::mutex> lock(mutex_);
    stats_.clear();
  }
  // "name,mean[s],min[s],max[s],std-dev[s]" rows (ElapsedTimeRecorder::logStats; column set recalled, ASSUMPTIONS.md D.1),
  // plus the sample count as a last column
  bool logStats(const std::string& path) const {
    std::ofstream out(path);
    if (!out) return false;
    out << "name,mean[s],min[s],max[s],std-dev[s],count\n";
    for (const auto& kv : stats()) {
      const TimerStats& t = kv.second;
      const double mean = t.count ? t.sum / static_cast<double>(t.count) : 0.0;
      const double var = t.count > 1 ? std::max(0.0, (t.sum_sq - t.sum * mean) / static_cast<double>(t.count - 1)) : 0.0;
      out << kv.first << ',' << mean << ',' << t.min << ',' << t.max << ',' << std::sqrt(var) << ',' << t.count << "\n";
    }
    return true;
  }
  std::function<void()> sync_device;  // optional: called when a timer with `sync` set stops
  bool disabled = false;

 private:
  mutable std::mutex mutex_;
  std::map<std::string, TimerStats> stats_;
};

class ScopedTimer {
 public:
  ScopedTimer(std::string name, uint64_t /*timestamp_ns*/, bool sync = false)
      : name_(std::move(name)), sync_(sync), start_(std::chrono::steady_clock::now()) {}
  ~ScopedTimer() { stop(); }
  void stop() {
    if (done_) return;
    done_ = true;
    ElapsedTimeRecorder& r = ElapsedTimeRecorder::instance();
    if (r.disabled) return;
    if (sync_ && r.sync_device) r.sync_device();
    r.record(name_, std::chrono::duration<double>(std::chrono::steady_clock::now() - start_).count());
  }

 private:
  std::string name_;
  bool sync_, done_ = false;
  std::chrono::steady_clock::time_point start_;
};
}  // namespace timing

}  // namespace hydra
