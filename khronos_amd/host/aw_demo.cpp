// aw_demo.cpp — drives khronos::ActiveWindow (host mirror) over a synthetic stream, the way the Hydra module
// thread drives the reference (spinOnce per InputPacket, finishMapping at shutdown), and prints a JSON
// summary that tests/test_gpu_host.py compares with the step-wise C-ABI path and the oracle.
// usage: aw_demo <config.yaml> <width> <height> <frames> [object_label]
//        aw_demo --slices | --render | --query | --distance | --voronoi | --places | --travel | --align | --weld | --merge | --diff | --segment | --checkpoint | --bench | --rayver ... (below)
//   object_label >= 0: the stand-in detector / tracker below; otherwise the plugins named in the config
#include <execinfo.h>
#include <csignal>
#include <unistd.h>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <queue>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <unordered_map>

#include <chrono>

#include <hip/hip_runtime_api.h>

#include "active_window.h"
#include "ray_verificator.h"

extern "C" {
void* synth_create(uint32_t seed, int num_static, int with_mover);
void synth_destroy(void* s);
void synth_render(void* sp, int W, int H, float fx, float fy, float cx, float cy, const double* T, double t_sec,
                  float max_depth, float noise_sigma_rel, uint32_t noise_seed, float* depth, uint8_t* rgb, int32_t* label,
                  int num_threads);
}

using namespace khronos;

// test stand-in for the instance-forwarding object detector + id tracker (the real
// ConnectedSemantics / MaxIoUTracker are host plugins that are not part of the device path): pixels carrying
// `label` become semantic cluster 1 of the frame (object_image = 1 there), with the bounding box of their
// world-frame vertices, and one track collects them.
struct LabelObjectDetector : ObjectDetector {
  int label;
  const int32_t* current_labels = nullptr;
  explicit LabelObjectDetector(int l) : label(l) {}
  void processInput(const VolumetricMap& map, FrameData& data) override {
    const size_t n = static_cast<size_t>(data.input.sensor.width) * data.input.sensor.height;
    std::vector<int32_t> obj(n, 0);
    const std::vector<float> vm = data.input.vertexMap();
    const std::vector<float> range = data.input.rangeImage();
    MeasurementCluster cl;
    cl.id = 1;
    for (size_t i = 0; i < n; ++i)
      if (current_labels[i] == label && range[i] > 0.f) {
        obj[i] = 1;
        cl.bounding_box.include(&vm[3 * i]);
        ++cl.num_pixels;
      }
    khr_set_frame_image(map.ctx(), data.input.slot, /*object image*/ 1, obj.data(), 0);
    if (cl.num_pixels > 0) data.semantic_clusters.push_back(cl);
  }
};

struct SingleTrackTracker : Tracker {
  void processInput(FrameData& data) override {
    if (data.semantic_clusters.empty()) return;
    if (tracks_.empty()) {
      Track t;
      t.id = 0;
      t.first_seen = data.input.timestamp_ns;
      t.semantics = SemanticClusterInfo(1);
      tracks_.push_back(t);
    }
    Track& t = tracks_[0];
    t.last_seen = data.input.timestamp_ns;
    t.observations.push_back({data.input.timestamp_ns, 1, -1});
    t.confidence = std::min(1.f, static_cast<float>(t.observations.size()) / 4.f);
  }
};

static void circlePose(double t, double* T) {
  const double th = 2.0 * M_PI * t / 10.0, yaw = th + M_PI / 2;
  const double f[3] = {std::cos(yaw), std::sin(yaw), 0}, r[3] = {f[1], -f[0], 0}, d[3] = {0, 0, -1};
  const double p[3] = {1.5 * std::cos(th), 1.5 * std::sin(th), 1.5};
  for (int i = 0; i < 3; ++i) {
    T[4 * i + 0] = r[i];
    T[4 * i + 1] = d[i];
    T[4 * i + 2] = f[i];
    T[4 * i + 3] = p[i];
  }
  T[12] = T[13] = T[14] = 0;
  T[15] = 1;
}

// aw_demo --rayver <policy>: drives khronos::RayVerificator (host mirror over the device index) with a scenario from
// stdin and prints the check results as JSON lines (tests/test_gpu_host.py compares them with the oracle).
//   P <n> then n lines "<stamp> x y z"          agent poses (sorted by time)
//   V <n> then n lines "<first> <last> x y z"   mesh vertices; every P / V block is followed by an update
//   Q <n> then n lines "<earliest> <latest> x y z"
static int rayverDemo(const char* policy) {
  RayVerificator::Config cfg;
  const char* names[] = {"First", "Last", "FirstAndLast", "Middle", "All"};
  for (int i = 0; i < 5; ++i)
    if (std::string(policy) == names[i]) cfg.ray_policy = static_cast<RayVerificator::Config::RayPolicy>(i);
  std::cin >> cfg.block_size >> cfg.radial_tolerance >> cfg.depth_tolerance >> cfg.active_window_duration;
  RayVerificator rv(cfg);
  std::vector<uint64_t> pose_stamps, first_seen, last_seen;
  std::vector<float> pose_pos, vertices;
  std::string tok;
  while (std::cin >> tok) {
    size_t n = 0;
    std::cin >> n;
    if (tok == "P") {
      for (size_t i = 0; i < n; ++i) {
        uint64_t t; float x, y, z;
        std::cin >> t >> x >> y >> z;
        pose_stamps.push_back(t);
        pose_pos.insert(pose_pos.end(), {x, y, z});
      }
    } else if (tok == "V") {
      for (size_t i = 0; i < n; ++i) {
        uint64_t a, b; float x, y, z;
        std::cin >> a >> b >> x >> y >> z;
        first_seen.push_back(a);
        last_seen.push_back(b);
        vertices.insert(vertices.end(), {x, y, z});
      }
      rv.updateData(pose_stamps, pose_pos, vertices, first_seen, last_seen);
    } else if (tok == "Q") {
      std::vector<float> pts;
      std::vector<uint64_t> t0, t1;
      for (size_t i = 0; i < n; ++i) {
        uint64_t a, b; float x, y, z;
        std::cin >> a >> b >> x >> y >> z;
        t0.push_back(a);
        t1.push_back(b);
        pts.insert(pts.end(), {x, y, z});
      }
      const auto res = rv.checkMany(pts, t0, t1);
      std::printf("{\"rays\": %zu, \"results\": [", rv.numRays());
      for (size_t i = 0; i < res.size(); ++i) {
        std::printf("%s{\"present\": [", i ? ", " : "");
        for (size_t k = 0; k < res[i].present.size(); ++k) std::printf("%s%" PRIu64, k ? ", " : "", res[i].present[k]);
        std::printf("], \"absent\": [");
        for (size_t k = 0; k < res[i].absent.size(); ++k) std::printf("%s%" PRIu64, k ? ", " : "", res[i].absent[k]);
        std::printf("]}");
      }
      std::printf("]}\n");
    } else if (tok == "C") {  // C <n> <resolution> <window> <relative> <absence> <presence>, then n lines "<forward> <earliest> <latest> x y z"
      RayChangeDetector::Config dc;
      int rel = 1;
      std::cin >> dc.temporal_resolution >> dc.window_size >> rel >> dc.absence_confidence >> dc.presence_confidence;
      dc.use_relative_confidence = rel != 0;
      const RayChangeDetector det(dc);
      std::vector<float> pts;
      std::vector<uint64_t> t0, t1;
      std::vector<uint8_t> fwd;
      for (size_t i = 0; i < n; ++i) {
        int f; uint64_t a, b; float x, y, z;
        std::cin >> f >> a >> b >> x >> y >> z;
        fwd.push_back(static_cast<uint8_t>(f));
        t0.push_back(a);
        t1.push_back(b);
        pts.insert(pts.end(), {x, y, z});
      }
      const auto res = det.detectChangesMany(rv, pts, t0, t1, fwd);
      std::printf("{\"changes\": [");
      for (size_t i = 0; i < res.size(); ++i)
        std::printf("%s[%lld, %lld]", i ? ", " : "", res[i].closest_absent ? static_cast<long long>(*res[i].closest_absent) : -1ll,
                    res[i].furthest_persistent ? static_cast<long long>(*res[i].furthest_persistent) : -1ll);
      std::printf("]}\n");
    }
  }
  return 0;
}

// aw_demo --bench <config.yaml> <width> <height> <preroll> <warmup> <steps>: khronos::ActiveWindow::spinOnce itself, timed the way
// bench.py times the step-wise C ABI: every frame of the stream is rendered and put into HBM BEFORE the timed
// region (InputPacket::on_device), preroll + warmup untimed steps, then `steps` calls of step() back to back; the clock stops when
// the device has drained and the extraction workers have been joined.  One JSON line.
static int benchDemo(int argc, char** argv) {
  if (argc < 8) {
    std::fprintf(stderr, "usage: aw_demo --bench <config.yaml> <width> <height> <preroll> <warmup> <steps>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), pre = std::atoi(argv[5]), warm = std::atoi(argv[6]), steps = std::atoi(argv[7]);
  const int N = pre + warm + steps;
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  std::vector<hydra::InputPacket> pkts(static_cast<size_t>(N));
  std::vector<void*> dev;
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket& pkt = pkts[static_cast<size_t>(i)];
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    void *d = nullptr, *c = nullptr, *l = nullptr;
    if (hipMalloc(&d, n * 4) != hipSuccess || hipMalloc(&c, n * 3) != hipSuccess || hipMalloc(&l, n * 4) != hipSuccess ||
        hipMemcpy(d, depth.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(c, rgb.data(), n * 3, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(l, label.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) {
      std::fprintf(stderr, "aw_demo --bench: device frames\n");
      return 1;
    }
    dev.insert(dev.end(), {d, c, l});
    pkt.depth = static_cast<const float*>(d);
    pkt.color = static_cast<const uint8_t*>(c);
    pkt.labels = static_cast<const int32_t*>(l);
    pkt.on_device = true;
    pkt.buffers_complete = true;  // (rendered and synchronised before the timed region)
  }
  int n_out = 0;
  size_t dyn_frames = 0;
  auto run = [&](int a, int b, bool count) {
    for (int i = a; i < b; ++i) {
      khr_host_trace("step_begin");
      auto out = aw.step(pkts[static_cast<size_t>(i)]);
      hydra::ActiveWindowOutput::Ptr popped;
      while (out_queue->pop(&popped)) {}
      if (count) {
        n_out += out ? 1 : 0;
        dyn_frames += aw.numDynamicClustersOfLastFrame() > 0 ? 1 : 0;  // (not getLatestFrameData(): that completes the deferred tracker step)
      }
    }
  };
  run(0, pre + warm, false);
  khr_sync(aw.getMap().ctx());
  khr_host_trace("timed_begin");
  const auto t0 = std::chrono::steady_clock::now();
  run(pre + warm, N, true);
  khr_host_trace("join_begin");
  const auto t1 = std::chrono::steady_clock::now();
  aw.joinExtractions();
  khr_sync(aw.getMap().ctx());
  const auto t2 = std::chrono::steady_clock::now();
  const double ms_steps = std::chrono::duration<double, std::milli>(t1 - t0).count(), ms_all = std::chrono::duration<double, std::milli>(t2 - t0).count();
  std::printf("{\"what\": \"khronos::ActiveWindow::spinOnce (libkhronos_amd_host.so), frames resident in HBM, %dx%d\", \"preroll\": %d, \"warmup\": %d, "
              "\"steps\": %d, \"frames_per_s\": %.2f, \"ms_per_step\": %.5f, \"steps_ms\": %.4f, \"drain_and_join_ms\": %.4f, \"outputs\": %d, "
              "\"frames_with_dynamic_clusters\": %zu, \"tracks\": %zu}\n",
              W, H, pre, warm, steps, 1e3 * steps / ms_all, ms_all / steps, ms_steps, ms_all - ms_steps, n_out, dyn_frames, aw.getTracks().size());
  if (std::getenv("AW_BENCH_TIMERS"))  // (host view of the reference's timer scopes over the whole run: where spinOnce spends its time)
    for (const auto& kv : hydra::timing::ElapsedTimeRecorder::instance().stats())
      std::fprintf(stderr, "%-44s count %6llu  mean %8.4f ms\n", kv.first.c_str(), static_cast<unsigned long long>(kv.second.count),
                   1e3 * kv.second.sum / static_cast<double>(kv.second.count));
  aw.finishMapping();
  for (void* p : dev) hipFree(p);
  synth_destroy(scene);
  return 0;
}

// The visualizer's three map slices restated over a cloneBlock loop (the path INTEGRATION.md section 3 used to give sinks): every
// allocated block on the layer, in allocatedBlockIndices' sorted order, copied whole, its plane read x-outer / y-inner.
static hydra::MapSlice sliceByBlockCopies(const VolumetricMap& map, float height) {
  hydra::MapSlice s;
  const int vps = map.config.voxels_per_side;
  s.voxel_z = hydra::sliceVoxelZ(height, map.config.voxel_size, vps);
  s.voxels_per_side = vps;
  const int64_t bz = (s.voxel_z >= 0 ? s.voxel_z : s.voxel_z - (vps - 1)) / vps, lz = s.voxel_z - bz * vps;
  const float bs = map.blockSize(), vs = map.config.voxel_size;
  for (const auto& idx : map.allocatedBlockIndices()) {
    if (idx[2] != bz) continue;
    const hydra::BlockCopy b = map.cloneBlock(idx);
    s.block_xy.insert(s.block_xy.end(), {idx[0], idx[1]});
    for (int x = 0; x < vps; ++x)
      for (int y = 0; y < vps; ++y) {
        const size_t lin = static_cast<size_t>(x + vps * (y + vps * lz));
        s.positions.insert(s.positions.end(), {static_cast<float>(idx[0]) * bs + (static_cast<float>(x) + 0.5f) * vs,
                                               static_cast<float>(idx[1]) * bs + (static_cast<float>(y) + 0.5f) * vs,
                                               static_cast<float>(idx[2]) * bs + (static_cast<float>(lz) + 0.5f) * vs});
        s.distance.push_back(b.distance[lin]);
        s.weight.push_back(b.weight[lin]);
        s.last_observed.push_back(b.last_observed[lin]);
        s.flags.push_back(b.flags[lin]);
      }
  }
  return s;
}

template <typename T>
static bool sameBits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// aw_demo --slices <config.yaml> <width> <height> <frames> [slice_height] [relative] [show_unknown]: a Khronos sink builds the
// visualizer's three slices every frame twice, through VolumetricMap::slice (khr_map_slice) and through a cloneBlock loop, checks
// that they agree and times both (the device is drained before each, so neither pays for the frame's own kernels).  One JSON line:
// per-frame means after kWarm frames -- device_slice_ms (VolumetricMap::slice + the three classifications), device_fetch_ms (the
// slice call alone), block_copy_ms (the cloneBlock loop + the same classifications).
static int slicesDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --slices <config.yaml> <width> <height> <frames> [slice_height] [relative] [show_unknown]\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  hydra::SliceConfig sc;
  if (argc > 6) sc.slice_height = static_cast<float>(std::atof(argv[6]));
  if (argc > 7) sc.slice_height_is_relative = std::atoi(argv[7]) != 0;
  if (argc > 8) sc.show_unknown_voxels = std::atoi(argv[8]) != 0;
  constexpr int kWarm = 3;  // frames before the averages (the slice staging grows on the first calls)
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  int frames = 0, agree = 0, timed = 0;
  double ms_dev = 0, ms_fetch = 0, ms_copy = 0, blocks = 0;
  size_t blocks_max = 0, points = 0;
  std::string first_mismatch;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    const float h = sc.height(data.input.world_T_body);
    const uint64_t stamp = data.input.timestamp_ns;
    const float trunc = map.config.truncation_distance;
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    const hydra::MapSlice a = map.slice(h);
    const auto t_fetch = clk::now();
    const hydra::SlicePoints ea = hydra::everFreeSlice(a, sc.show_unknown_voxels), ta = hydra::trackingSlice(a, stamp, sc.show_unknown_voxels),
                             da = hydra::tsdfSlice(a, trunc);
    const auto t1 = clk::now();
    const hydra::MapSlice b = sliceByBlockCopies(map, h);
    const hydra::SlicePoints eb = hydra::everFreeSlice(b, sc.show_unknown_voxels), tb = hydra::trackingSlice(b, stamp, sc.show_unknown_voxels),
                             db = hydra::tsdfSlice(b, trunc);
    const auto t2 = clk::now();
    const bool same_slice = a.voxel_z == b.voxel_z && a.block_xy == b.block_xy && sameBits(a.positions, b.positions) &&
                            sameBits(a.distance, b.distance) && sameBits(a.weight, b.weight) && a.last_observed == b.last_observed &&
                            a.flags == b.flags;
    const bool ok = same_slice && ea == eb && ta == tb && da == db;
    if (ok) ++agree;
    else if (first_mismatch.empty())
      first_mismatch = "frame " + std::to_string(frames) + (same_slice ? ": classifications differ" : ": slices differ") + " (" +
                       std::to_string(a.numBlocks()) + " / " + std::to_string(b.numBlocks()) + " blocks)";
    if (frames >= kWarm) {
      ms_dev += std::chrono::duration<double, std::milli>(t1 - t0).count();
      ms_fetch += std::chrono::duration<double, std::milli>(t_fetch - t0).count();
      ms_copy += std::chrono::duration<double, std::milli>(t2 - t1).count();
      blocks += static_cast<double>(a.numBlocks());
      ++timed;
    }
    blocks_max = std::max(blocks_max, a.numBlocks());
    points += ea.voxel.size() + ta.voxel.size() + da.voxel.size();
    ++frames;
  });
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  const double d = timed ? static_cast<double>(timed) : 1.0;
  std::printf("{\"what\": \"ActiveWindowVisualizer map slices (ever-free, tracking, TSDF) per frame, %dx%d, voxel %.4g m\", \"frames\": %d, "
              "\"agree_frames\": %d, \"first_mismatch\": \"%s\", \"timed_frames\": %d, \"device_slice_ms\": %.4f, \"device_fetch_ms\": %.4f, \"block_copy_ms\": %.4f, "
              "\"blocks_on_layer_mean\": %.1f, \"blocks_on_layer_max\": %zu, \"points\": %zu, \"slice_height\": %.4g, \"relative\": %d}\n",
              W, H, static_cast<double>(cfg.volumetric_map.voxel_size), frames, agree, first_mismatch.c_str(), timed, ms_dev / d, ms_fetch / d, ms_copy / d,
              blocks / d, blocks_max, points, static_cast<double>(sc.slice_height), int(sc.slice_height_is_relative));
  return agree == frames ? 0 : 3;
}

// ASSUMPTIONS.md A.13 restated on the host over a cloneBlock loop (the only way a sink could ask "what does the map say at this
// point" before khr_query_points): every block a tap falls into is copied whole, once per call, then each point's seven samples
// are interpolated tap by tap.
struct QueryByBlockCopies {
  const VolumetricMap& map;
  int vps, sh;
  float vs_inv, min_weight;
  bool with_semantics, with_tracking;
  std::unordered_map<uint64_t, std::unique_ptr<hydra::BlockCopy>> blocks;  // allocated blocks; copied when first touched
  uint64_t last_key = ~0ull;
  const hydra::BlockCopy* last = nullptr;

  static uint64_t key(int64_t bx, int64_t by, int64_t bz) {
    return static_cast<uint64_t>(bx + (1 << 20)) | (static_cast<uint64_t>(by + (1 << 20)) << 21) | (static_cast<uint64_t>(bz + (1 << 20)) << 42);
  }
  explicit QueryByBlockCopies(const VolumetricMap& m) : map(m) {
    khr_config kc;
    if (khr_get_config(map.ctx(), &kc) != KHR_OK) throw std::runtime_error(khr_last_error());
    vps = kc.voxels_per_side;
    sh = vps == 16 ? 4 : 3;
    vs_inv = 1.f / kc.voxel_size;
    min_weight = kc.mesh_min_weight;
    with_semantics = kc.with_semantics != 0;
    with_tracking = kc.with_tracking != 0;
    for (const auto& idx : map.allocatedBlockIndices()) blocks.emplace(key(idx[0], idx[1], idx[2]), nullptr);
  }
  // the block of global voxel (x, y, z), null when it is not allocated; *lin = the voxel's place in it
  const hydra::BlockCopy* voxel(int64_t x, int64_t y, int64_t z, size_t* lin) {
    const int64_t bx = x >> sh, by = y >> sh, bz = z >> sh, R = 1 << 20;
    if (bx < -R || bx >= R || by < -R || by >= R || bz < -R || bz >= R) return nullptr;
    *lin = static_cast<size_t>((x & (vps - 1)) + vps * ((y & (vps - 1)) + vps * (z & (vps - 1))));
    const uint64_t k = key(bx, by, bz);
    if (k == last_key) return last;
    auto it = blocks.find(k);
    const hydra::BlockCopy* b = nullptr;
    if (it != blocks.end()) {
      if (!it->second)
        it->second = std::make_unique<hydra::BlockCopy>(map.cloneBlock({static_cast<int32_t>(bx), static_cast<int32_t>(by), static_cast<int32_t>(bz)}));
      b = it->second.get();
    }
    last_key = k;
    last = b;
    return b;
  }
  bool sample(const int64_t* j, const float* f, float* d) {
    float v[8];
    bool valid = true;
    for (int t = 0; t < 8; ++t) {
      size_t lin = 0;
      const hydra::BlockCopy* b = voxel(j[0] + (t & 1), j[1] + ((t >> 1) & 1), j[2] + (t >> 2), &lin);
      valid = valid && b && b->weight[lin] >= min_weight;
      v[t] = b ? b->distance[lin] : 0.f;
    }
    const float c00 = v[0] + f[0] * (v[1] - v[0]), c10 = v[2] + f[0] * (v[3] - v[2]);
    const float c01 = v[4] + f[0] * (v[5] - v[4]), c11 = v[6] + f[0] * (v[7] - v[6]);
    const float c0 = c00 + f[1] * (c10 - c00), c1 = c01 + f[1] * (c11 - c01);
    *d = c0 + f[2] * (c1 - c0);
    return valid;
  }
  hydra::PointSamples run(const std::vector<float>& points) {
    const size_t n = points.size() / 3;
    hydra::PointSamples s;
    s.distance.assign(n, 0.f); s.gradient.assign(3 * n, 0.f); s.weight.assign(n, 0.f); s.color.assign(4 * n, 0); s.label.assign(n, 0u);
    s.flags.assign(n, 0); s.last_observed.assign(n, 0ull); s.status.assign(n, 0);
    constexpr float kLimit = 1073741824.f;
    for (size_t i = 0; i < n; ++i) {
      const float* p = &points[3 * i];
      float g[3], f[3];
      int64_t i0[3];
      bool in_range = true;
      for (int a = 0; a < 3; ++a) {
        g[a] = p[a] * vs_inv - 0.5f;
        in_range = in_range && std::fabs(g[a]) < kLimit;
      }
      if (!in_range) continue;
      for (int a = 0; a < 3; ++a) {
        const float fl = std::floor(g[a]);
        i0[a] = static_cast<int64_t>(fl);
        f[a] = g[a] - fl;
      }
      uint8_t status = 0;
      float d = 0.f;
      if (sample(i0, f, &d)) {
        status |= KHR_QP_VALUE;
        s.distance[i] = d;
      }
      float grad[3];
      bool all = true;
      for (int a = 0; a < 3; ++a) {
        int64_t jp[3] = {i0[0], i0[1], i0[2]}, jm[3] = {i0[0], i0[1], i0[2]};
        jp[a] += 1;
        jm[a] -= 1;
        float dp = 0.f, dm = 0.f;
        all = sample(jp, f, &dp) && all;
        all = sample(jm, f, &dm) && all;
        grad[a] = (dp - dm) * (0.5f * vs_inv);
      }
      if (all) {
        status |= KHR_QP_GRADIENT;
        for (int a = 0; a < 3; ++a) s.gradient[3 * i + a] = grad[a];
      }
      float gi[3];
      bool ok = true;
      for (int a = 0; a < 3; ++a) {
        gi[a] = std::floor(p[a] * vs_inv);
        ok = ok && std::fabs(gi[a]) < kLimit;
      }
      size_t lin = 0;
      const hydra::BlockCopy* b = ok ? voxel(static_cast<int64_t>(gi[0]), static_cast<int64_t>(gi[1]), static_cast<int64_t>(gi[2]), &lin) : nullptr;
      if (b) {
        status |= KHR_QP_VOXEL;
        s.weight[i] = b->weight[lin];
        std::memcpy(&s.color[4 * i], &b->color[4 * lin], 4);
        if (with_semantics) s.label[i] = b->semantic_label[lin];
        s.flags[i] = b->flags[lin];
        if (with_tracking) s.last_observed[i] = b->last_observed[lin];
      }
      s.status[i] = status;
      s.stats.n_value += (status & KHR_QP_VALUE) != 0;
      s.stats.n_gradient += (status & KHR_QP_GRADIENT) != 0;
      s.stats.n_voxel += (status & KHR_QP_VOXEL) != 0;
    }
    return s;
  }
};

static const char* queryDifference(const hydra::PointSamples& a, const hydra::PointSamples& b) {
  if (!(a.status == b.status)) return "status";
  if (!sameBits(a.distance, b.distance)) return "distance";
  if (!sameBits(a.gradient, b.gradient)) return "gradient";
  if (!sameBits(a.weight, b.weight)) return "weight";
  if (!(a.color == b.color)) return "color";
  if (!(a.label == b.label)) return "label";
  if (!(a.flags == b.flags)) return "flags";
  if (!(a.last_observed == b.last_observed)) return "last_observed";
  if (a.stats.n_value != b.stats.n_value || a.stats.n_gradient != b.stats.n_gradient || a.stats.n_voxel != b.stats.n_voxel) return "stats";
  return nullptr;
}

// aw_demo --query <config.yaml> <width> <height> <frames> [points]: a Khronos sink asks the map about the frame's own back-projected
// depth pixels (at most `points` of them; 0 = all), in image order and shuffled with a fixed seed, every frame twice: through
// VolumetricMap::query (khr_query_points) and through the cloneBlock loop above, checks the two bit for bit and times both (the
// device is drained before each).  One JSON line: per-frame means after kWarm frames.
static int queryDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --query <config.yaml> <width> <height> <frames> [points]\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  const size_t max_points = argc > 6 ? static_cast<size_t>(std::atoll(argv[6])) : 0;
  constexpr int kWarm = 3;  // frames before the averages (the query staging grows on the first calls)
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  int frames = 0, agree = 0, timed = 0;
  double ms[4] = {0, 0, 0, 0}, n_points = 0;  // device ordered, copies ordered, device shuffled, copies shuffled
  khr_query_stats last_stats{};
  std::string first_mismatch;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    const std::vector<float> vm = data.input.vertexMap(), range = data.input.rangeImage();
    if (range.empty() || vm.size() != 3 * range.size()) throw std::runtime_error("aw_demo --query: the frame's range image / vertex map are not available");
    std::vector<float> ordered;
    for (size_t i = 0; i < range.size() && (max_points == 0 || ordered.size() < 3 * max_points); ++i)
      if (range[i] > 0.f) ordered.insert(ordered.end(), {vm[3 * i], vm[3 * i + 1], vm[3 * i + 2]});
    const size_t np = ordered.size() / 3;
    std::vector<float> shuffled = ordered;
    uint64_t rng = 0x9E3779B97F4A7C15ull;  // splitmix64, Fisher-Yates
    for (size_t i = np; i > 1; --i) {
      uint64_t x = (rng += 0x9E3779B97F4A7C15ull);
      x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
      x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
      const size_t j = static_cast<size_t>((x ^ (x >> 31)) % i);
      for (int a = 0; a < 3; ++a) std::swap(shuffled[3 * (i - 1) + a], shuffled[3 * j + a]);
    }
    bool ok = true;
    double t_ms[4];
    for (int pass = 0; pass < 2; ++pass) {
      const std::vector<float>& pts = pass ? shuffled : ordered;
      khr_sync(map.ctx());
      const auto t0 = clk::now();
      const hydra::PointSamples a = map.query(pts);
      const auto t1 = clk::now();
      QueryByBlockCopies host(map);
      const hydra::PointSamples b = host.run(pts);
      const auto t2 = clk::now();
      t_ms[2 * pass] = std::chrono::duration<double, std::milli>(t1 - t0).count();
      t_ms[2 * pass + 1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
      const char* diff = queryDifference(a, b);
      if (diff) {
        ok = false;
        if (first_mismatch.empty())
          first_mismatch = "frame " + std::to_string(frames) + (pass ? " shuffled: " : " ordered: ") + diff + " differs";
      }
      if (!pass) last_stats = a.stats;
    }
    if (ok) ++agree;
    if (frames >= kWarm) {
      for (int k = 0; k < 4; ++k) ms[k] += t_ms[k];
      n_points += static_cast<double>(np);
      ++timed;
    }
    ++frames;
  });
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  const double d = timed ? static_cast<double>(timed) : 1.0, pts = n_points / d;
  auto rate = [&](double total_ms) { return total_ms > 0 ? pts / (total_ms / d * 1e-3) : 0.0; };
  std::printf("{\"what\": \"the live map at the frame's back-projected depth pixels (VolumetricMap::query vs a cloneBlock loop), %dx%d, voxel %.4g m\", "
              "\"frames\": %d, \"agree_frames\": %d, \"first_mismatch\": \"%s\", \"timed_frames\": %d, \"points_mean\": %.1f, "
              "\"device_query_ms\": %.4f, \"block_copy_ms\": %.4f, \"device_points_per_s\": %.4g, \"block_copy_points_per_s\": %.4g, "
              "\"device_query_shuffled_ms\": %.4f, \"block_copy_shuffled_ms\": %.4f, \"device_shuffled_points_per_s\": %.4g, "
              "\"block_copy_shuffled_points_per_s\": %.4g, \"last_stats\": {\"n_value\": %llu, \"n_gradient\": %llu, \"n_voxel\": %llu}}\n",
              W, H, static_cast<double>(cfg.volumetric_map.voxel_size), frames, agree, first_mismatch.c_str(), timed, pts, ms[0] / d, ms[1] / d,
              rate(ms[0]), rate(ms[1]), ms[2] / d, ms[3] / d, rate(ms[2]), rate(ms[3]), static_cast<unsigned long long>(last_stats.n_value),
              static_cast<unsigned long long>(last_stats.n_gradient), static_cast<unsigned long long>(last_stats.n_voxel));
  return agree == frames && frames == N ? 0 : 3;
}

// ASSUMPTIONS.md A.15 restated on the host over cloneBlock copies (what a planner had to do before khr_distance_field): every
// allocated block the box overlaps is copied whole, the cells are classified voxel by voxel, and the three windowed passes run
// line by line.
static hydra::DistanceField distanceByBlockCopies(const VolumetricMap& map, const hydra::DistanceFieldRequest& rq) {
  khr_config kc;
  if (khr_get_config(map.ctx(), &kc) != KHR_OK) throw std::runtime_error(khr_last_error());
  const int vps = kc.voxels_per_side, sh = vps == 16 ? 4 : 3, ratio = rq.ratio;
  const float min_weight = rq.min_weight == 0.f ? kc.mesh_min_weight : rq.min_weight;
  hydra::DistanceField f;
  f.origin = rq.origin, f.dims = rq.dims;
  f.cell_size = kc.voxel_size * static_cast<float>(ratio);
  const int nx = rq.dims[0], ny = rq.dims[1], nz = rq.dims[2];
  const size_t n = static_cast<size_t>(nx) * ny * nz;
  constexpr int32_t kFar = KHR_DF_FAR;
  std::unordered_map<uint64_t, std::unique_ptr<hydra::BlockCopy>> blocks;
  for (const auto& idx : map.allocatedBlockIndices()) blocks.emplace(QueryByBlockCopies::key(idx[0], idx[1], idx[2]), nullptr);
  std::vector<int32_t> outer(n), inner(n);
  f.status.assign(n, 0);
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        bool observed = false;
        float value = 0.f;
        for (int dz = 0; dz < ratio; ++dz)
          for (int dy = 0; dy < ratio; ++dy)
            for (int dx = 0; dx < ratio; ++dx) {
              const int64_t vx = static_cast<int64_t>(rq.origin[0] + x) * ratio + dx, vy = static_cast<int64_t>(rq.origin[1] + y) * ratio + dy,
                            vz = static_cast<int64_t>(rq.origin[2] + z) * ratio + dz;
              const int64_t bx = vx >> sh, by = vy >> sh, bz = vz >> sh, K = 1 << 20;
              if (bx < -K || bx >= K || by < -K || by >= K || bz < -K || bz >= K) continue;
              auto it = blocks.find(QueryByBlockCopies::key(bx, by, bz));
              if (it == blocks.end()) continue;
              if (!it->second)
                it->second = std::make_unique<hydra::BlockCopy>(map.cloneBlock({static_cast<int32_t>(bx), static_cast<int32_t>(by), static_cast<int32_t>(bz)}));
              const size_t lin = static_cast<size_t>((vx & (vps - 1)) + vps * ((vy & (vps - 1)) + vps * (vz & (vps - 1))));
              if (!(it->second->weight[lin] >= min_weight)) continue;
              const float d = it->second->distance[lin];
              value = observed ? std::fmin(value, d) : d;
              observed = true;
            }
        const bool obstacle = observed && value <= rq.surface_distance;
        const size_t at = f.index(x, y, z);
        outer[at] = (obstacle || (!observed && rq.unknown_is_obstacle)) ? 0 : kFar;
        inner[at] = (observed && !obstacle) ? 0 : kFar;
        f.status[at] = static_cast<uint8_t>((observed ? KHR_DF_OBSERVED : 0) | (obstacle ? KHR_DF_OBSTACLE : 0));
        f.stats.n_observed += observed, f.stats.n_obstacle += obstacle, f.stats.n_free += observed && !obstacle;
      }
  const int R = static_cast<int>(std::floor(rq.max_distance / f.cell_size));
  auto transform = [&](std::vector<int32_t>& g) {
    std::vector<int64_t> line, res;
    const size_t stride[3] = {1, static_cast<size_t>(nx), static_cast<size_t>(nx) * ny};
    const int len[3] = {nx, ny, nz};
    for (int axis = 0; axis < 3; ++axis) {
      const int L = len[axis], a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
      line.resize(L), res.resize(L);
      for (int p = 0; p < len[a1]; ++p)
        for (int q = 0; q < len[a2]; ++q) {
          const size_t base = stride[a1] * p + stride[a2] * q;
          for (int i = 0; i < L; ++i) line[i] = g[base + stride[axis] * i];
          for (int i = 0; i < L; ++i) {
            int64_t best = line[i];
            for (int j = std::max(0, i - R); j <= std::min(L - 1, i + R); ++j) best = std::min(best, line[j] + static_cast<int64_t>(i - j) * (i - j));
            res[i] = std::min<int64_t>(best, kFar);
          }
          for (int i = 0; i < L; ++i) g[base + stride[axis] * i] = static_cast<int32_t>(res[i]);
        }
    }
  };
  transform(outer);
  if (!rq.positive_only) transform(inner);
  f.distance.resize(n), f.d2.resize(n);
  const int64_t r2 = static_cast<int64_t>(R) * R;
  for (size_t i = 0; i < n; ++i) {
    const bool in_set = outer[i] == 0, neg = in_set && !rq.positive_only;
    int32_t mag = in_set ? (rq.positive_only ? 0 : inner[i]) : outer[i];
    float dist;
    if (mag <= r2) {
      dist = f.cell_size * std::sqrt(static_cast<float>(mag));
      f.status[i] |= KHR_DF_IN_RANGE;
      ++f.stats.n_in_range;
    } else {
      mag = kFar;
      dist = rq.max_distance;
    }
    f.distance[i] = neg ? -dist : dist;
    f.d2[i] = neg ? -mag : mag;
  }
  return f;
}

// aw_demo --distance <config.yaml> <width> <height> <frames>: a Khronos sink asks, per output, for the distance field of a box around
// the sensor -- hydra::DistanceFieldConfig from the file's freespace_places -- through VolumetricMap::distanceField
// (khr_distance_field) and through the cloneBlock loop above, checks the two bit for bit and times both (the device is drained
// before each).  One JSON line: per-frame means after kWarm frames.
static int distanceDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --distance <config.yaml> <width> <height> <frames>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  constexpr int kWarm = 3;  // frames before the averages (the work grids and the staging grow on the first call)
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  const hydra::DistanceFieldConfig dfc = hydra::DistanceFieldConfig::fromYaml(khronos_amd::parseYaml(ss.str()));
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  int frames = 0, agree = 0, timed = 0;
  double ms_dev = 0, ms_copy = 0;
  size_t cells = 0;
  khr_df_stats last_stats{};
  std::string first_mismatch;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    hydra::DistanceFieldRequest rq(dfc);
    const float cell = map.config.voxel_size * static_cast<float>(rq.ratio);
    // the sensor's cell in the middle of a box that reaches the range plus a margin on x and y, half of that on z
    const int half = std::min(KHR_DF_MAX_DIM / 2, static_cast<int>(std::floor(rq.max_distance / cell)) + 12);
    const int hd[3] = {half, half, std::max(1, half / 2)};
    for (int a = 0; a < 3; ++a) {
      rq.origin[a] = static_cast<int32_t>(std::floor(data.input.world_T_sensor[4 * a + 3] / static_cast<double>(cell))) - hd[a];
      rq.dims[a] = 2 * hd[a];
    }
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    const hydra::DistanceField a = map.distanceField(rq);
    const auto t1 = clk::now();
    const hydra::DistanceField b = distanceByBlockCopies(map, rq);
    const auto t2 = clk::now();
    const char* diff = nullptr;
    if (!(a.status == b.status)) diff = "status";
    else if (!(a.d2 == b.d2)) diff = "d2";
    else if (!sameBits(a.distance, b.distance)) diff = "distance";
    else if (a.stats.n_observed != b.stats.n_observed || a.stats.n_obstacle != b.stats.n_obstacle || a.stats.n_free != b.stats.n_free ||
             a.stats.n_in_range != b.stats.n_in_range) diff = "stats";
    if (!diff) ++agree;
    else if (first_mismatch.empty()) first_mismatch = "frame " + std::to_string(frames) + ": " + diff + " differs";
    last_stats = a.stats;
    cells = a.size();
    if (frames >= kWarm) {
      ms_dev += std::chrono::duration<double, std::milli>(t1 - t0).count();
      ms_copy += std::chrono::duration<double, std::milli>(t2 - t1).count();
      ++timed;
    }
    ++frames;
  });
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  const double d = timed ? static_cast<double>(timed) : 1.0;
  std::printf("{\"what\": \"the distance field of a box around the sensor (VolumetricMap::distanceField vs a cloneBlock loop), %dx%d, voxel %.4g m, "
              "ratio %d, max_distance %.4g m, positive_only %d\", \"frames\": %d, \"agree_frames\": %d, \"first_mismatch\": \"%s\", \"timed_frames\": %d, "
              "\"cells\": %zu, \"last_stats\": {\"n_observed\": %llu, \"n_obstacle\": %llu, \"n_free\": %llu, \"n_in_range\": %llu}, "
              "\"device_ms\": %.4f, \"block_copy_ms\": %.4f}\n",
              W, H, static_cast<double>(cfg.volumetric_map.voxel_size), dfc.ratio, static_cast<double>(dfc.max_distance_m), int(dfc.positive_distance_only),
              frames, agree, first_mismatch.c_str(), timed, cells, static_cast<unsigned long long>(last_stats.n_observed),
              static_cast<unsigned long long>(last_stats.n_obstacle), static_cast<unsigned long long>(last_stats.n_free),
              static_cast<unsigned long long>(last_stats.n_in_range), ms_dev / d, ms_copy / d);
  return agree == frames && frames == N ? 0 : 3;
}

// ASSUMPTIONS.md A.20 checked on the host from the arrays VolumetricMap::voronoiField returned, and from nothing else: every site is
// a cell of the obstacle set (by status and unknown_is_obstacle) at the squared distance d2 says; the basis rule applied to the
// site array gives the basis array; the list is the ascending run of the cells with basis >= min_basis.  Returns what differs first,
// or nullptr.
static const char* voronoiCheck(const hydra::VoronoiField& f, const hydra::VoronoiRequest& rq) {
  const int nx = f.dims[0], ny = f.dims[1], nz = f.dims[2];
  const size_t n = static_cast<size_t>(nx) * ny * nz;
  if (f.distance.size() != n || f.d2.size() != n || f.status.size() != n || f.site.size() != n || f.basis.size() != n) return "array sizes";
  auto separated = [&](const std::array<int32_t, 3>& c, const std::array<int32_t, 3>& p, const std::array<int32_t, 3>& q) {
    if (p == q) return false;
    const int l1 = std::abs(p[0] - q[0]) + std::abs(p[1] - q[1]) + std::abs(p[2] - q[2]);
    if (rq.mode != KHR_VOR_ANGLE && l1 >= rq.parent_l1_separation) return true;
    if (rq.mode == KHR_VOR_L1) return false;
    int64_t dot = 0, aa = 0, bb = 0;
    for (int k = 0; k < 3; ++k) {
      const int64_t a = p[k] - c[k], b = q[k] - c[k];
      dot += a * b, aa += a * a, bb += b * b;
    }
    return static_cast<double>(dot) <= static_cast<double>(rq.parent_cos_angle_separation) * std::sqrt(static_cast<double>(aa) * static_cast<double>(bb));
  };
  const int min_basis = rq.min_basis == 0 ? 2 : rq.min_basis;
  size_t listed = 0;
  uint64_t n_eligible = 0, n_basis[KHR_VOR_MAX_BASIS + 1] = {0, 0, 0, 0, 0};
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        const size_t i = f.index(x, y, z);
        const int32_t s = f.site[i];
        const bool in_set = (f.status[i] & KHR_DF_OBSTACLE) != 0 || (rq.unknown_is_obstacle && !(f.status[i] & KHR_DF_OBSERVED));
        if ((s >= 0) != (!in_set && (f.status[i] & KHR_DF_IN_RANGE) != 0)) return "which cells have a site";
        int nb = 0;
        std::array<int32_t, 3> B[KHR_VOR_MAX_BASIS] = {};
        if (s >= 0) {
          if (static_cast<size_t>(s) >= n) return "a site outside the box";
          const uint8_t st = f.status[s];
          if (!((st & KHR_DF_OBSTACLE) != 0 || (rq.unknown_is_obstacle && !(st & KHR_DF_OBSERVED)))) return "a site outside the obstacle set";
          const std::array<int32_t, 3> p = f.cellAt(s);
          const int64_t dx = x - p[0], dy = y - p[1], dz = z - p[2];
          if (dx * dx + dy * dy + dz * dz != f.d2[i]) return "the distance to the site";
          if (f.distance[i] >= rq.min_distance) {
            ++n_eligible;
            B[nb++] = p;
            for (int oz = -1; oz <= 1; ++oz)
              for (int oy = -1; oy <= 1; ++oy)
                for (int ox = -1; ox <= 1; ++ox) {
                  const int X = x + ox, Y = y + oy, Z = z + oz;
                  if ((ox == 0 && oy == 0 && oz == 0) || X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz || nb == KHR_VOR_MAX_BASIS) continue;
                  const int32_t t = f.site[f.index(X, Y, Z)];
                  if (t < 0) continue;
                  const std::array<int32_t, 3> q = f.cellAt(t);
                  bool apart = true;
                  for (int j = 0; j < nb && apart; ++j) apart = separated({x, y, z}, B[j], q);
                  if (apart) B[nb++] = q;
                }
          }
        }
        if (nb != f.basis[i]) return "basis";
        ++n_basis[nb];
        if (nb < min_basis) continue;
        if (listed >= f.numListed() || f.cells.size() != 3 * f.numListed() || f.cell_sites.size() != 3 * KHR_VOR_MAX_BASIS * f.numListed() ||
            f.cell_distance.size() != f.numListed())
          return "the length of the list";
        if (f.cells[3 * listed] != f.origin[0] + x || f.cells[3 * listed + 1] != f.origin[1] + y || f.cells[3 * listed + 2] != f.origin[2] + z) return "the listed cells";
        if (f.cell_basis[listed] != nb || std::memcmp(&f.cell_distance[listed], &f.distance[i], sizeof(float)) != 0) return "the listed basis or distance";
        for (int j = 0; j < KHR_VOR_MAX_BASIS; ++j)
          for (int k = 0; k < 3; ++k)
            if (f.cell_sites[(listed * KHR_VOR_MAX_BASIS + j) * 3 + k] != (j < nb ? f.origin[k] + B[j][k] : 0)) return "the listed sites";
        ++listed;
      }
  if (listed != f.numListed() || listed != f.stats.n_listed) return "the length of the list";
  if (n_eligible != f.stats.n_eligible || n_basis[2] != f.stats.n_basis2 || n_basis[3] != f.stats.n_basis3 || n_basis[4] != f.stats.n_basis4) return "stats";
  return nullptr;
}

// aw_demo --voronoi <config.yaml> <width> <height> <frames>: a Khronos sink asks, per output, for the Voronoi field of a box around
// the sensor -- hydra::DistanceFieldConfig and hydra::VoronoiConfig from the file's freespace_places -- through
// VolumetricMap::voronoiField (khr_voronoi_field) and checks the returned arrays against A.20 on the host.  One JSON line.
static int voronoiDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --voronoi <config.yaml> <width> <height> <frames>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  constexpr int kWarm = 3;  // frames before the average (the buffers grow on the first call)
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  const khronos_amd::YamlNode root = khronos_amd::parseYaml(ss.str());
  const hydra::DistanceFieldConfig dfc = hydra::DistanceFieldConfig::fromYaml(root);
  const hydra::VoronoiConfig vc = hydra::VoronoiConfig::fromYaml(root);
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  int frames = 0, agree = 0, timed = 0;
  double ms_dev = 0;
  size_t cells = 0;
  khr_voronoi_stats last_stats{};
  std::string first_mismatch;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    hydra::VoronoiRequest rq(dfc, vc);
    const float cell = map.config.voxel_size * static_cast<float>(rq.ratio);
    // the sensor's cell in the middle of a box that reaches the range plus a margin on x and y, half of that on z
    const int half = std::min(KHR_DF_MAX_DIM / 2, static_cast<int>(std::floor(rq.max_distance / cell)) + 12);
    const int hd[3] = {half, half, std::max(1, half / 2)};
    for (int a = 0; a < 3; ++a) {
      rq.origin[a] = static_cast<int32_t>(std::floor(data.input.world_T_sensor[4 * a + 3] / static_cast<double>(cell))) - hd[a];
      rq.dims[a] = 2 * hd[a];
    }
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    const hydra::VoronoiField f = map.voronoiField(rq);
    const auto t1 = clk::now();
    const char* diff = voronoiCheck(f, rq);
    if (!diff) ++agree;
    else if (first_mismatch.empty()) first_mismatch = "frame " + std::to_string(frames) + ": " + diff + " differs";
    last_stats = f.stats;
    cells = f.size();
    if (frames >= kWarm) {
      ms_dev += std::chrono::duration<double, std::milli>(t1 - t0).count();
      ++timed;
    }
    ++frames;
  });
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  const double d = timed ? static_cast<double>(timed) : 1.0;
  auto u = [](uint64_t v) { return static_cast<unsigned long long>(v); };
  std::printf("{\"what\": \"the Voronoi field of a box around the sensor (VolumetricMap::voronoiField, checked on the host from its own arrays), %dx%d, "
              "voxel %.4g m, ratio %d, max_distance %.4g m, mode %d, min_basis %d\", \"frames\": %d, \"agree_frames\": %d, \"first_mismatch\": \"%s\", "
              "\"timed_frames\": %d, \"cells\": %zu, \"n_listed\": %llu, \"last_stats\": {\"n_observed\": %llu, \"n_obstacle\": %llu, \"n_free\": %llu, "
              "\"n_in_range\": %llu, \"n_eligible\": %llu, \"n_basis2\": %llu, \"n_basis3\": %llu, \"n_basis4\": %llu, \"n_listed\": %llu}, \"device_ms\": %.4f}\n",
              W, H, static_cast<double>(cfg.volumetric_map.voxel_size), dfc.ratio, static_cast<double>(dfc.max_distance_m), vc.mode, vc.min_basis, frames, agree,
              first_mismatch.c_str(), timed, cells, u(last_stats.n_listed), u(last_stats.n_observed), u(last_stats.n_obstacle), u(last_stats.n_free),
              u(last_stats.n_in_range), u(last_stats.n_eligible), u(last_stats.n_basis2), u(last_stats.n_basis3), u(last_stats.n_basis4), u(last_stats.n_listed),
              ms_dev / d);
  return agree == frames && frames == N ? 0 : 3;
}

// what VolumetricMap::placesGraph replaces: the host's flood fill over the downloaded Voronoi field and its pair search (A.21),
// held against the returned graph; nullptr when they agree, else the name of the first output that differs
static const char* placesCheck(const hydra::VoronoiField& f, const hydra::PlacesGraph& g, const khr_places_request& rq) {
  const int nx = f.dims[0], ny = f.dims[1], nz = f.dims[2];
  const size_t n = f.size();
  const int mb = rq.min_basis == 0 ? 2 : rq.min_basis, C = rq.compression;
  auto fdiv = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
  std::vector<int32_t> place(n, -1);
  std::vector<uint8_t> member(n, 0);
  for (size_t i = 0; i < n; ++i) member[i] = f.basis[i] >= mb && f.distance[i] >= rq.min_node_distance && f.d2[i] >= 0 && f.d2[i] < (1 << 30);
  struct Place { int32_t centre, d2; uint32_t cells; int64_t sum[3]; };
  std::vector<Place> places;
  std::vector<int32_t> queue;
  for (size_t s = 0; s < n; ++s) {
    if (!member[s] || place[s] >= 0) continue;
    const int32_t id = static_cast<int32_t>(places.size());
    Place p{static_cast<int32_t>(s), f.d2[s], 0, {0, 0, 0}};
    const auto c0 = f.cellAt(static_cast<int32_t>(s));
    const int b0[3] = {fdiv(f.origin[0] + c0[0], C), fdiv(f.origin[1] + c0[1], C), fdiv(f.origin[2] + c0[2], C)};
    queue.assign(1, static_cast<int32_t>(s));
    place[s] = id;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int32_t i = queue[h];
      const auto c = f.cellAt(i);
      ++p.cells;
      for (int a = 0; a < 3; ++a) p.sum[a] += f.origin[a] + c[a];
      if (f.d2[i] > p.d2 || (f.d2[i] == p.d2 && i < p.centre)) p.centre = i, p.d2 = f.d2[i];
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
            if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz) continue;
            if (fdiv(f.origin[0] + x, C) != b0[0] || fdiv(f.origin[1] + y, C) != b0[1] || fdiv(f.origin[2] + z, C) != b0[2]) continue;
            const size_t j = f.index(x, y, z);
            if (member[j] && place[j] < 0) place[j] = id, queue.push_back(static_cast<int32_t>(j));
          }
    }
    places.push_back(p);
  }
  // the pair search: every unordered adjacent pair once, from its lower cell
  std::map<std::pair<int32_t, int32_t>, std::pair<int32_t, uint32_t>> pairs;
  for (size_t i = 0; i < n; ++i) {
    if (place[i] < 0) continue;
    const auto c = f.cellAt(static_cast<int32_t>(i));
    for (int dz = 0; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if (dz == 0 && (dy < 0 || (dy == 0 && dx <= 0))) continue;
          const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
          if (x < 0 || x >= nx || y < 0 || y >= ny || z >= nz) continue;
          const size_t j = f.index(x, y, z);
          if (place[j] < 0 || place[j] == place[i]) continue;
          auto& e = pairs[{std::min(place[i], place[j]), std::max(place[i], place[j])}];
          e.first = std::max(e.first, std::min(f.d2[i], f.d2[j]));
          ++e.second;
        }
  }
  // components by relaxation over the edges (the least place of each), the filter, the renumbering
  std::vector<int32_t> comp(places.size());
  for (size_t p = 0; p < places.size(); ++p) comp[p] = static_cast<int32_t>(p);
  for (bool changed = true; changed;) {
    changed = false;
    for (const auto& e : pairs) {
      const int32_t m = std::min(comp[e.first.first], comp[e.first.second]);
      if (comp[e.first.first] != m || comp[e.first.second] != m) comp[e.first.first] = comp[e.first.second] = m, changed = true;
    }
  }
  std::vector<uint32_t> size(places.size(), 0);
  for (size_t p = 0; p < places.size(); ++p) ++size[comp[p]];
  const uint32_t need = static_cast<uint32_t>(std::max(rq.min_component_size, 1));
  std::vector<int32_t> place_new(places.size(), -1), comp_new(places.size(), -1);
  uint32_t kept = 0, kept_comps = 0, comps_all = 0;
  for (size_t p = 0; p < places.size(); ++p) {
    if (comp[p] == static_cast<int32_t>(p)) ++comps_all;
    if (size[comp[p]] < need) continue;
    if (comp[p] == static_cast<int32_t>(p)) comp_new[p] = static_cast<int32_t>(kept_comps++);
    place_new[p] = static_cast<int32_t>(kept++);
  }
  if (g.stats.n_places_all != places.size() || g.stats.n_edges_all != pairs.size() || g.stats.n_components_all != comps_all || g.stats.n_places != kept ||
      g.stats.n_components != kept_comps || g.numPlaces() != kept)
    return "stats";
  for (size_t i = 0; i < n; ++i)
    if (g.place[i] != (place[i] < 0 ? -1 : place_new[place[i]])) return "place";
  std::vector<uint32_t> degree(kept, 0);
  size_t e_out = 0;
  for (const auto& e : pairs) {
    const int32_t a = place_new[e.first.first], b = place_new[e.first.second];
    if (a < 0) continue;
    if (e_out >= g.numEdges() || g.edge_a[e_out] != static_cast<uint32_t>(a) || g.edge_b[e_out] != static_cast<uint32_t>(b) ||
        g.edge_clearance_d2[e_out] != e.second.first || g.edge_n_contacts[e_out] != e.second.second)
      return "edges";
    ++degree[a], ++degree[b], ++e_out;
  }
  if (e_out != g.numEdges() || g.stats.n_edges != e_out) return "edges";
  for (size_t p = 0; p < places.size(); ++p) {
    if (place_new[p] < 0) continue;
    const size_t q = static_cast<size_t>(place_new[p]);
    const Place& P = places[p];
    const auto c = f.cellAt(P.centre);
    for (int a = 0; a < 3; ++a)
      if (g.centre[3 * q + a] != f.origin[a] + c[a] || g.sum[3 * q + a] != P.sum[a]) return "centre";
    if (g.centre_d2[q] != P.d2 || std::memcmp(&g.radius[q], &f.distance[P.centre], 4) != 0 || g.basis[q] != f.basis[P.centre] || g.n_cells[q] != P.cells) return "centre";
    const int32_t s = f.site[P.centre];
    const auto sc = s >= 0 ? f.cellAt(s) : std::array<int32_t, 3>{0, 0, 0};
    for (int a = 0; a < 3; ++a)
      if (g.site[3 * q + a] != (s >= 0 ? f.origin[a] + sc[a] : 0)) return "site";
    if (g.degree[q] != degree[q] || g.component[q] != static_cast<uint32_t>(comp_new[comp[p]])) return "component";
  }
  return nullptr;
}

// aw_demo --places <config.yaml> <width> <height> <frames>: a Khronos sink asks, per output, for the Voronoi field of a box around the
// sensor and for the places graph of that field -- hydra::PlacesConfig from the file's freespace_places -- through
// VolumetricMap::placesGraph (khr_places_graph), and sets it against the host's flood fill and pair search over the downloaded
// field, which the call replaces.  One JSON line.
static int placesDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --places <config.yaml> <width> <height> <frames>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  constexpr int kWarm = 3;  // frames before the average (the buffers grow on the first calls)
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  const khronos_amd::YamlNode root = khronos_amd::parseYaml(ss.str());
  const hydra::DistanceFieldConfig dfc = hydra::DistanceFieldConfig::fromYaml(root);
  const hydra::VoronoiConfig vc = hydra::VoronoiConfig::fromYaml(root);
  const hydra::PlacesConfig pc = hydra::PlacesConfig::fromYaml(root);
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  int frames = 0, agree = 0, timed = 0, compression = 0;
  double ms_dev = 0, ms_host = 0;
  size_t cells = 0;
  khr_places_stats last{};
  std::string first_mismatch;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    hydra::VoronoiRequest rq(dfc, vc);
    const float cell = map.config.voxel_size * static_cast<float>(rq.ratio);
    const int half = std::min(KHR_DF_MAX_DIM / 2, static_cast<int>(std::floor(rq.max_distance / cell)) + 12);
    const int hd[3] = {half, half, std::max(1, half / 2)};
    for (int a = 0; a < 3; ++a) {
      rq.origin[a] = static_cast<int32_t>(std::floor(data.input.world_T_sensor[4 * a + 3] / static_cast<double>(cell))) - hd[a];
      rq.dims[a] = 2 * hd[a];
    }
    const hydra::VoronoiField f = map.voronoiField(rq);
    const khr_places_request prq = pc.request(f.cell_size, vc.min_basis);
    compression = prq.compression;
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    const hydra::PlacesGraph g = map.placesGraph(f, prq);
    const auto t1 = clk::now();
    const char* diff = placesCheck(f, g, prq);
    const auto t2 = clk::now();
    if (!diff) ++agree;
    else if (first_mismatch.empty()) first_mismatch = "frame " + std::to_string(frames) + ": " + diff + " differs";
    last = g.stats;
    cells = f.size();
    if (frames >= kWarm) {
      ms_dev += std::chrono::duration<double, std::milli>(t1 - t0).count();
      ms_host += std::chrono::duration<double, std::milli>(t2 - t1).count();
      ++timed;
    }
    ++frames;
  });
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  const double d = timed ? static_cast<double>(timed) : 1.0;
  auto u = [](uint64_t v) { return static_cast<unsigned long long>(v); };
  std::printf("{\"what\": \"the places graph of the Voronoi field of a box around the sensor (VolumetricMap::placesGraph, against the host's flood fill and "
              "pair search over the downloaded field), %dx%d, voxel %.4g m, ratio %d, compression %d cells, min_node_distance %.4g m, min_component_size %d\", "
              "\"frames\": %d, \"agree_frames\": %d, \"first_mismatch\": \"%s\", \"timed_frames\": %d, \"cells\": %zu, \"last_stats\": {\"n_members\": %llu, "
              "\"n_places_all\": %llu, \"n_edges_all\": %llu, \"n_components_all\": %llu, \"n_places\": %llu, \"n_edges\": %llu, \"n_components\": %llu}, "
              "\"device_ms\": %.4f, \"host_ms\": %.4f}\n",
              W, H, static_cast<double>(cfg.volumetric_map.voxel_size), dfc.ratio, compression, static_cast<double>(pc.min_node_distance_m), pc.minComponentSize(),
              frames, agree, first_mismatch.c_str(), timed, cells, u(last.n_members), u(last.n_places_all), u(last.n_edges_all), u(last.n_components_all),
              u(last.n_places), u(last.n_edges), u(last.n_components), ms_dev / d, ms_host / d);
  return agree == frames && frames == N ? 0 : 3;
}

// what VolumetricMap::travelField replaces: Dijkstra on the host over the downloaded distance and status (A.22), pairs (cost, goal)
// in a binary heap.  Returns what differs first, or nullptr.
static const char* travelCheck(const hydra::VoronoiField& f, const hydra::TravelField& t, const std::vector<int32_t>& goals, const khr_travel_request& rq) {
  const int nx = f.dims[0], ny = f.dims[1], nz = f.dims[2];
  const size_t n = f.size();
  std::vector<uint8_t> trav(n);
  uint64_t n_trav = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool cls = (f.status[i] & KHR_DF_OBSERVED) ? !(f.status[i] & KHR_DF_OBSTACLE) : rq.allow_unknown != 0;
    trav[i] = cls && f.distance[i] >= rq.clearance;
    n_trav += trav[i];
  }
  const uint64_t far = ~0ull;
  std::vector<uint64_t> key(n, far);
  using Item = std::pair<uint64_t, uint32_t>;  // key, cell
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  uint64_t used = 0;
  for (size_t g = 0; g < goals.size() / 3; ++g) {
    const std::array<int32_t, 3> cell{goals[3 * g], goals[3 * g + 1], goals[3 * g + 2]};
    if (!t.contains(cell) || !trav[t.index(cell)]) continue;
    ++used;
    if (g < key[t.index(cell)]) key[t.index(cell)] = g, heap.push({g, static_cast<uint32_t>(t.index(cell))});
  }
  const int most = rq.connectivity == 6 ? 1 : rq.connectivity == 18 ? 2 : 3;
  while (!heap.empty()) {
    const Item it = heap.top();
    heap.pop();
    if (it.first != key[it.second]) continue;
    const int x = static_cast<int>(it.second % nx), y = static_cast<int>((it.second / nx) % ny), z = static_cast<int>(it.second / (static_cast<uint32_t>(nx) * ny));
    for (int c = 0; c < 27; ++c) {
      const int dx = c % 3 - 1, dy = (c / 3) % 3 - 1, dz = c / 9 - 1, nzr = (dx != 0) + (dy != 0) + (dz != 0);
      const int X = x + dx, Y = y + dy, Z = z + dz;
      if (nzr == 0 || nzr > most || X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
      const size_t q = f.index(X, Y, Z);
      const uint64_t cand = it.first + (static_cast<uint64_t>(nzr == 1 ? 10 : nzr == 2 ? 14 : 17) << 32);
      if (!trav[q] || (rq.max_cost && (cand >> 32) > rq.max_cost) || cand >= key[q]) continue;
      key[q] = cand;
      heap.push({cand, static_cast<uint32_t>(q)});
    }
  }
  uint64_t reached = 0, top = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool r = key[i] != far;
    reached += r;
    if (r) top = std::max<uint64_t>(top, key[i] >> 32);
    if (t.cost[i] != (r ? static_cast<uint32_t>(key[i] >> 32) : KHR_TF_UNREACHED)) return "cost";
    if (t.goal[i] != (r ? static_cast<int32_t>(static_cast<uint32_t>(key[i])) : -1)) return "goal";
    if ((t.parent[i] == 255) != !r || (t.parent[i] == 13) != (r && (key[i] >> 32) == 0)) return "parent";
  }
  if (t.stats.n_traversable != n_trav || t.stats.n_goals_used != used || t.stats.n_reached != reached || t.stats.max_cost != top) return "stats";
  return nullptr;
}

// aw_demo --travel <config.yaml> <width> <height> <frames>: a Khronos sink asks, per output, for the Voronoi field of a box around the
// sensor and for the travel field from the camera's cell -- hydra::TravelConfig from the file's freespace_places.travel -- through
// VolumetricMap::travelField (khr_travel_field), sets it against Dijkstra on the host over the downloaded field, which the call
// replaces, and traces the path from the reached cell furthest away (VolumetricMap::travelPaths).  One JSON line: the reach from the
// camera's cell and that path.
static int travelDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --travel <config.yaml> <width> <height> <frames>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  constexpr int kWarm = 3;  // frames before the average (the buffers grow on the first calls)
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  const khronos_amd::YamlNode root = khronos_amd::parseYaml(ss.str());
  const hydra::DistanceFieldConfig dfc = hydra::DistanceFieldConfig::fromYaml(root);
  const hydra::VoronoiConfig vc = hydra::VoronoiConfig::fromYaml(root);
  const hydra::TravelConfig tc = hydra::TravelConfig::fromYaml(root);
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  int frames = 0, agree = 0, timed = 0, paths_ok = 0;
  double ms_dev = 0, ms_host = 0;
  size_t cells = 0, path_cells = 0;
  uint32_t path_cost = 0;
  khr_travel_stats last{};
  std::string first_mismatch, path_text;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    hydra::VoronoiRequest rq(dfc, vc);
    const float cell = map.config.voxel_size * static_cast<float>(rq.ratio);
    const int half = std::min(KHR_DF_MAX_DIM / 2, static_cast<int>(std::floor(rq.max_distance / cell)) + 12);
    const int hd[3] = {half, half, std::max(1, half / 2)};
    std::vector<int32_t> camera(3);
    for (int a = 0; a < 3; ++a) {
      camera[a] = static_cast<int32_t>(std::floor(data.input.world_T_sensor[4 * a + 3] / static_cast<double>(cell)));
      rq.origin[a] = camera[a] - hd[a];
      rq.dims[a] = 2 * hd[a];
    }
    const hydra::VoronoiField f = map.voronoiField(rq);
    const khr_travel_request trq = tc.request(f.cell_size);
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    const hydra::TravelField t = map.travelField(f, camera, trq);
    const auto t1 = clk::now();
    const char* diff = travelCheck(f, t, camera, trq);
    const auto t2 = clk::now();
    if (!diff) ++agree;
    else if (first_mismatch.empty()) first_mismatch = "frame " + std::to_string(frames) + ": " + diff + " differs";
    // the path from the reached cell furthest away (the first such cell), and from a cell outside the box
    size_t far_cell = 0;
    for (size_t i = 0; i < t.size(); ++i)
      if (t.cost[i] != KHR_TF_UNREACHED && (t.cost[far_cell] == KHR_TF_UNREACHED || t.cost[i] > t.cost[far_cell])) far_cell = i;
    const std::array<int32_t, 3> fc = f.cellAt(static_cast<int32_t>(far_cell));
    const std::vector<int32_t> starts = {t.origin[0] + fc[0], t.origin[1] + fc[1], t.origin[2] + fc[2], t.origin[0] - 1, t.origin[1], t.origin[2]};
    const hydra::TravelPaths p = map.travelPaths(starts);
    bool ok = p.numPaths() == 2 && p.length(1) == 0 && p.path_cost[1] == KHR_TF_UNREACHED && p.path_goal[1] == -1;
    if (ok && t.stats.n_reached > 0) {
      const size_t len = p.length(0);
      ok = len >= 1 && p.path_cost[0] == t.cost[far_cell] && p.path_goal[0] == 0 && p.cells[0] == starts[0] && p.cells[1] == starts[1] && p.cells[2] == starts[2];
      for (int a = 0; a < 3 && ok; ++a) ok = p.cells[3 * (len - 1) + a] == camera[a];
      // every step moves to a neighbour and loses the move's weight
      for (size_t k = 0; k + 1 < len && ok; ++k) {
        const std::array<int32_t, 3> a{p.cells[3 * k], p.cells[3 * k + 1], p.cells[3 * k + 2]}, b{p.cells[3 * k + 3], p.cells[3 * k + 4], p.cells[3 * k + 5]};
        const int nzr = (a[0] != b[0]) + (a[1] != b[1]) + (a[2] != b[2]);
        ok = std::abs(a[0] - b[0]) <= 1 && std::abs(a[1] - b[1]) <= 1 && std::abs(a[2] - b[2]) <= 1 && nzr >= 1 &&
             t.cost[t.index(a)] - t.cost[t.index(b)] == (nzr == 1 ? 10u : nzr == 2 ? 14u : 17u);
      }
      path_cells = len, path_cost = p.path_cost[0];
      path_text = "[" + std::to_string(starts[0]) + ", " + std::to_string(starts[1]) + ", " + std::to_string(starts[2]) + "]";
    } else if (ok) {
      ok = p.length(0) == 0;
    }
    if (ok) ++paths_ok;
    else if (first_mismatch.empty()) first_mismatch = "frame " + std::to_string(frames) + ": the path differs";
    last = t.stats;
    cells = f.size();
    if (frames >= kWarm) {
      ms_dev += std::chrono::duration<double, std::milli>(t1 - t0).count();
      ms_host += std::chrono::duration<double, std::milli>(t2 - t1).count();
      ++timed;
    }
    ++frames;
  });
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  const double d = timed ? static_cast<double>(timed) : 1.0;
  auto u = [](uint64_t v) { return static_cast<unsigned long long>(v); };
  std::printf("{\"what\": \"the travel field from the camera's cell over the Voronoi field of a box around the sensor (VolumetricMap::travelField, against "
              "Dijkstra on the host over the downloaded field) and the path from the furthest reached cell, %dx%d, voxel %.4g m, ratio %d, clearance %.4g m, "
              "connectivity %d\", \"frames\": %d, \"agree_frames\": %d, \"path_frames\": %d, \"first_mismatch\": \"%s\", \"timed_frames\": %d, \"cells\": %zu, "
              "\"last_stats\": {\"n_traversable\": %llu, \"n_goals_used\": %llu, \"n_reached\": %llu, \"max_cost\": %llu, \"n_rounds\": %llu, \"n_waits\": %llu}, "
              "\"last_path\": {\"start\": %s, \"cells\": %zu, \"cost\": %u}, \"device_ms\": %.4f, \"host_ms\": %.4f}\n",
              W, H, static_cast<double>(cfg.volumetric_map.voxel_size), dfc.ratio, static_cast<double>(tc.clearance_m), tc.connectivity, frames, agree, paths_ok,
              first_mismatch.c_str(), timed, cells, u(last.n_traversable), u(last.n_goals_used), u(last.n_reached), u(last.max_cost), u(last.n_rounds), u(last.n_waits),
              path_text.empty() ? "null" : path_text.c_str(), path_cells, path_cost, ms_dev / d, ms_host / d);
  return agree == frames && paths_ok == frames && frames == N ? 0 : 3;
}

// 64-bit digest of an image's bytes: sum_i mix(i * L + byte_i) mod 2^64, mix = the splitmix64 step of khr_map_digest
// (tests/test_gpu_render_view.py restates it in numpy)
static uint64_t imageDigest(const void* data, size_t bytes) {
  const uint8_t* b = static_cast<const uint8_t*>(data);
  uint64_t sum = 0;
  for (size_t i = 0; i < bytes; ++i) {
    uint64_t x = static_cast<uint64_t>(i) * 0x632BE59BD9B4E019ull + b[i] + 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    sum += x ^ (x >> 31);
  }
  return sum;
}

// aw_demo --render <config.yaml> <width> <height> <frames> [step_voxels]: drives the synthetic stream through an ActiveWindow whose
// Khronos sink renders the map at the LAST frame's own pose and sensor (VolumetricMap::render(frame): one call).  One JSON line:
// the image shapes, the render counters, a 64-bit digest per image (imageDigest) and the call's wall-clock time.
static int renderDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --render <config.yaml> <width> <height> <frames> [step_voxels]\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  const float step_voxels = argc > 6 ? static_cast<float>(std::atof(argv[6])) : 0.f;
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  int frames = 0;
  hydra::RenderedView view;
  double render_ms = 0;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    if (++frames != N) return;
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    view = map.render(data.input, step_voxels);
    render_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  });
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  auto dg = [](const auto& v) { return static_cast<unsigned long long>(imageDigest(v.data(), v.size() * sizeof(v[0]))); };
  std::printf("{\"what\": \"the live map rendered at the last frame's pose (VolumetricMap::render), %d frames\", \"frames\": %d, "
              "\"shapes\": {\"depth\": [%d, %d], \"normal\": [%d, %d, 3], \"color\": [%d, %d, 4], \"label\": [%d, %d], \"flags\": [%d, %d], "
              "\"status\": [%d, %d]}, \"stats\": {\"n_hit\": %llu, \"n_blocked\": %llu, \"n_samples_total\": %llu, \"n_samples_evaluated\": %llu}, "
              "\"digests\": {\"depth\": \"%016llx\", \"normal\": \"%016llx\", \"color\": \"%016llx\", \"label\": \"%016llx\", "
              "\"flags\": \"%016llx\", \"status\": \"%016llx\"}, \"render_ms\": %.3f}\n",
              N, frames, view.height, view.width, view.height, view.width, view.height, view.width, view.height, view.width, view.height,
              view.width, view.height, view.width, static_cast<unsigned long long>(view.stats.n_hit),
              static_cast<unsigned long long>(view.stats.n_blocked), static_cast<unsigned long long>(view.stats.n_samples_total),
              static_cast<unsigned long long>(view.stats.n_samples_evaluated), dg(view.depth), dg(view.normal), dg(view.color), dg(view.label),
              dg(view.flags), dg(view.status), render_ms);
  return frames == N && view.numPixels() == n ? 0 : 3;
}

// aw_demo --align <config.yaml> <width> <height> <frames> [stride]: drives the synthetic stream through an ActiveWindow whose Khronos
// sink, at the LAST frame, perturbs the frame's own pose by about 1 degree and 3 cm and lets the map pull it back
// (VolumetricMap::align: khr_align_frame).  The frame goes in three ways -- the converted frame (InputData), the raw depth image and
// the host's back-projection of its strided pixels as a point list -- which must give the same pose bit for bit.  One JSON line: the
// true pose, the prior, the returned pose, the rotation (rad) and translation (m) errors before and after, the loop's counters and
// the call's wall-clock time.  Exit status 0 iff the pose was found, both errors shrank and the three forms agree.
static void poseError(const double* T, const double* truth, double* rot, double* trans) {
  double tr = 0, d2 = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) tr += T[4 * r + c] * truth[4 * r + c];  // trace(R truth^T)
    const double d = T[4 * r + 3] - truth[4 * r + 3];
    d2 += d * d;
  }
  const double cs = std::min(1.0, std::max(-1.0, 0.5 * (tr - 1.0)));
  *rot = std::acos(cs);
  *trans = std::sqrt(d2);
}

static int alignDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --align <config.yaml> <width> <height> <frames> [stride]\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  hydra::AlignOptions opt;
  if (argc > 6) opt.stride = std::atoi(argv[6]);
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  int frames = 0;
  double truth[16], prior[16];
  hydra::Alignment from_frame, from_depth, from_points;
  size_t n_points = 0;
  double align_ms = 0;
  using clk = std::chrono::steady_clock;
  aw.addKhronosSink([&](const FrameData& data, const VolumetricMap& map, const Tracks&) {
    if (++frames != N) return;
    std::memcpy(truth, data.input.world_T_sensor, sizeof(truth));
    // prior = exp(omega^) R, t + v with |omega| = 0.0175 rad, |v| = 0.029 m (Rodrigues)
    const double w[3] = {0.010, -0.008, 0.012}, v[3] = {0.020, -0.015, 0.015};
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), A = std::sin(th) / th, B = (1.0 - std::cos(th)) / (th * th);
    const double K[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    std::memcpy(prior, truth, sizeof(prior));
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        double s = 0;
        for (int k = 0; k < 3; ++k) {
          double e = (r == k ? 1.0 : 0.0) + A * K[r][k];
          for (int j = 0; j < 3; ++j) e += B * K[r][j] * K[j][k];
          s += e * truth[4 * k + c];
        }
        prior[4 * r + c] = s;
      }
      prior[4 * r + 3] = truth[4 * r + 3] + v[r];
    }
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    from_frame = map.align(data.input, prior, opt);
    align_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    const hydra::Sensor& sn = data.input.sensor;
    from_depth = map.align(sn, depth.data(), prior, opt);
    std::vector<float> pts;
    for (int y = 0; y < H; y += opt.stride)
      for (int x = 0; x < W; x += opt.stride) {
        const float z = depth[static_cast<size_t>(y) * W + x];
        if (!(z > 0.f) || !std::isfinite(z) || z < sn.min_range || z > sn.max_range) continue;
        const float xn = (static_cast<float>(x) - sn.cx) / sn.fx, yn = (static_cast<float>(y) - sn.cy) / sn.fy;
        const float px = xn * z, py = yn * z;
        pts.push_back(px);
        pts.push_back(py);
        pts.push_back(z);
      }
    n_points = pts.size() / 3;
    from_points = map.align(pts, prior, opt);
  });
  void* scene = synth_create(1234, 12, 1);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  aw.finishMapping();
  synth_destroy(scene);
  if (frames != N) return 3;
  auto same = [](const hydra::Alignment& a, const hydra::Alignment& b) {
    return std::memcmp(a.world_T_source, b.world_T_source, sizeof(a.world_T_source)) == 0 && a.found == b.found && a.iterations == b.iterations &&
           a.n_inlier_first == b.n_inlier_first && a.n_inlier_last == b.n_inlier_last && std::memcmp(a.H, b.H, sizeof(a.H)) == 0 &&
           std::memcmp(a.b, b.b, sizeof(a.b)) == 0;
  };
  auto mat = [](const double* T) {
    std::string s = "[";
    for (int i = 0; i < 16; ++i) {
      char b[40];
      std::snprintf(b, sizeof(b), "%s%.17g", i ? ", " : "", T[i]);
      s += b;
    }
    return s + "]";
  };
  double r0, t0, r1, t1;
  poseError(prior, truth, &r0, &t0);
  poseError(from_frame.world_T_source, truth, &r1, &t1);
  const bool depth_same = same(from_frame, from_depth), points_same = same(from_depth, from_points);
  std::printf("{\"what\": \"a perturbed pose of the last frame pulled back by the map (VolumetricMap::align), %d frames\", \"frames\": %d, "
              "\"stride\": %d, \"truth\": %s, \"prior\": %s, \"pose\": %s, \"found\": %s, \"iterations\": %d, \"converged\": %s, "
              "\"n_inlier_first\": %llu, \"n_inlier_last\": %llu, \"rmse_first\": %.17g, \"rmse_last\": %.17g, \"rot_error_prior\": %.9g, "
              "\"trans_error_prior\": %.9g, \"rot_error\": %.9g, \"trans_error\": %.9g, \"n_points\": %zu, \"depth_form_equal\": %s, "
              "\"point_form_equal\": %s, \"align_ms\": %.3f}\n",
              N, frames, opt.stride, mat(truth).c_str(), mat(prior).c_str(), mat(from_frame.world_T_source).c_str(),
              from_frame.found ? "true" : "false", from_frame.iterations, from_frame.converged ? "true" : "false",
              static_cast<unsigned long long>(from_frame.n_inlier_first), static_cast<unsigned long long>(from_frame.n_inlier_last),
              from_frame.rmse_first, from_frame.rmse_last, r0, t0, r1, t1, n_points, depth_same ? "true" : "false",
              points_same ? "true" : "false", align_ms);
  return from_frame.found && r1 < r0 && t1 < t0 && depth_same && points_same ? 0 : 3;
}

// aw_demo --checkpoint <config.yaml> <width> <height> <frames> [file]: runs the synthetic stream through an ActiveWindow, saves the live
// map through getMap().save (hydra::VolumetricMap: khr_checkpoint_save around a file), loads the file into the empty map of a second
// context of the same configuration and compares the two maps' whole-map digests.  One JSON line: both digests (12 words each),
// both block counts, the file's bytes, save_ms and load_ms (wall clock, file I/O included).  Exit status 0 iff the maps are equal.
static int checkpointDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --checkpoint <config.yaml> <width> <height> <frames> [file]\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  const std::string path = argc > 6 ? argv[6] : "aw_demo_map.chk";
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  synth_destroy(scene);
  using clk = std::chrono::steady_clock;
  hydra::VolumetricMap& map = aw.getMap();
  khr_sync(map.ctx());
  const auto t0 = clk::now();
  const size_t file_bytes = map.save(path);
  const auto t1 = clk::now();
  khr_config kc;
  if (khr_get_config(map.ctx(), &kc) != KHR_OK) throw std::runtime_error(khr_last_error());
  khr_ctx* ctx2 = nullptr;
  if (khr_create(&kc, &ctx2) != KHR_OK) throw std::runtime_error(std::string("khr_create: ") + khr_last_error());
  hydra::VolumetricMap map2(map.config, ctx2);
  const auto t2 = clk::now();
  const size_t kept = map2.load(path);
  const auto t3 = clk::now();
  uint64_t da[KHR_DIGEST_WORDS], db[KHR_DIGEST_WORDS];
  if (khr_map_digest(map.ctx(), da) != KHR_OK || khr_map_digest(ctx2, db) != KHR_OK) throw std::runtime_error(khr_last_error());
  const size_t blocks_a = map.numBlocks(), blocks_b = map2.numBlocks();
  const bool same = std::memcmp(da, db, sizeof(da)) == 0 && blocks_a == blocks_b && kept == blocks_b &&
                    map.allocatedBlockIndices() == map2.allocatedBlockIndices();
  auto words = [](const uint64_t* d) {
    std::string s = "[";
    for (int i = 0; i < KHR_DIGEST_WORDS; ++i) {
      char b[32];
      std::snprintf(b, sizeof(b), "%s\"%016llx\"", i ? ", " : "", static_cast<unsigned long long>(d[i]));
      s += b;
    }
    return s + "]";
  };
  std::printf("{\"what\": \"map checkpoint through hydra::VolumetricMap::save / load, %dx%d, %d frames\", \"digest_saved\": %s, \"digest_loaded\": %s, "
              "\"blocks_saved\": %zu, \"blocks_loaded\": %zu, \"file_bytes\": %zu, \"save_ms\": %.3f, \"load_ms\": %.3f, \"equal\": %s}\n",
              W, H, N, words(da).c_str(), words(db).c_str(), blocks_a, blocks_b, file_bytes,
              std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t3 - t2).count(),
              same ? "true" : "false");
  khr_destroy(ctx2);
  aw.finishMapping();
  return same ? 0 : 3;
}

static void onSegv(int sig) {  // a crash must not look like an empty result: print where it happened
  void* bt[48];
  const int n = backtrace(bt, 48);
  const char msg[] = "aw_demo: fatal signal, backtrace:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(bt, n, 2);
  _exit(128 + sig);
}

// the weld of ASSUMPTIONS.md A.16 on one host thread: first-come over the soup, one unordered_map of cells.  false: a vertex out of range
static bool hostWeld(const hydra::Mesh& soup, float r, hydra::IndexedMesh* out) {
  const size_t n = soup.numVertices();
  std::unordered_map<uint64_t, uint32_t> index;
  index.reserve(n / 4 + 16);
  out->soup_to_vertex.resize(n);
  for (size_t i = 0; i < n; ++i) {
    uint64_t key = 0;
    for (int a = 0; a < 3; ++a) {
      const float p = soup.points[3 * i + a], c = std::floor(p / r);
      if (!std::isfinite(p) || !(c >= -1048576.f && c < 1048576.f)) return false;
      key |= static_cast<uint64_t>(static_cast<uint32_t>(static_cast<int>(c) + (1 << 20)) & 0x1fffffu) << (21 * a);
    }
    const auto it = index.emplace(key, static_cast<uint32_t>(out->labels.size()));
    if (it.second) {
      out->points.insert(out->points.end(), &soup.points[3 * i], &soup.points[3 * i] + 3);
      out->colors.insert(out->colors.end(), &soup.colors[4 * i], &soup.colors[4 * i] + 4);
      out->labels.push_back(soup.labels[i]);
      out->first_seen_stamps.push_back(soup.first_seen_stamps[i]);
      out->stamps.push_back(soup.stamps[i]);
    }
    out->soup_to_vertex[i] = it.first->second;
  }
  for (size_t f = 0; f + 2 < n; f += 3) {
    const uint32_t a = out->soup_to_vertex[f], b = out->soup_to_vertex[f + 1], c = out->soup_to_vertex[f + 2];
    if (a != b && b != c && a != c) out->faces.insert(out->faces.end(), {a, b, c});
  }
  out->stats.n_soup_vertices = n;
  out->stats.n_vertices = out->labels.size();
  out->stats.n_faces = out->faces.size() / 3;
  out->stats.n_degenerate_faces = n / 3 - out->stats.n_faces;
  return true;
}

static double medianOf(std::vector<double> v) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

// aw_demo --weld <config.yaml> <width> <height> <frames> [resolution] [repeats]: drives the synthetic stream through an ActiveWindow and
// then takes the window's mesh (the last output's) twice: as an indexed mesh welded on the device (VolumetricMap::weldedMesh:
// khr_weld_mesh + khr_weld_mesh_into) and as the soup (khr_fetch_mesh + khr_fetch_mesh_into) welded here by the same definition.
// One JSON line: the counts, whether the two are equal array for array, the median wall-clock time of both ways over `repeats`
// (device drained before each), and the bytes that cross to the host.  resolution 0 / absent: the voxel size.
static int weldDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --weld <config.yaml> <width> <height> <frames> [resolution] [repeats]\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  float r = argc > 6 ? static_cast<float>(std::atof(argv[6])) : 0.f;
  if (!(r > 0.f)) r = cfg.volumetric_map.voxel_size;
  const int reps = std::max(1, argc > 7 ? std::atoi(argv[7]) : 5);
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  void* scene = synth_create(1234, 12, 1);
  const size_t n = static_cast<size_t>(W) * H;
  std::vector<float> depth(n);
  std::vector<uint8_t> rgb(n * 3);
  std::vector<int32_t> label(n);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  synth_destroy(scene);
  const VolumetricMap& map = aw.getMap();
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  hydra::IndexedMesh dev, host;
  hydra::Mesh soup;
  std::vector<double> t_dev, t_fetch, t_weld;
  bool in_range = true;
  for (int k = 0; k < reps + 1; ++k) {  // (the first round grows the buffers of both ways and is not timed)
    khr_sync(map.ctx());
    const auto t0 = clk::now();
    dev = map.weldedMesh(r);
    const auto t1 = clk::now();
    khr_sync(map.ctx());
    const auto t2 = clk::now();
    khr_mesh_view view{};
    const int64_t nv = khr_fetch_mesh(map.ctx(), &view);
    if (nv < 0) throw std::runtime_error(std::string("khr_fetch_mesh: ") + khr_last_error());
    soup.points.resize(3 * nv); soup.colors.resize(4 * nv); soup.labels.resize(nv); soup.first_seen_stamps.resize(nv); soup.stamps.resize(nv);
    if (nv && khr_fetch_mesh_into(map.ctx(), soup.points.data(), soup.colors.data(), soup.labels.data(), soup.first_seen_stamps.data(),
                                  soup.stamps.data()) != KHR_OK)
      throw std::runtime_error(std::string("khr_fetch_mesh_into: ") + khr_last_error());
    const auto t3 = clk::now();
    host = hydra::IndexedMesh();
    in_range = hostWeld(soup, r, &host);
    const auto t4 = clk::now();
    if (k > 0) t_dev.push_back(ms(t0, t1)), t_fetch.push_back(ms(t2, t3)), t_weld.push_back(ms(t3, t4));
  }
  aw.finishMapping();
  const char* diff = nullptr;
  if (!in_range) diff = "the host weld found a vertex out of range";
  else if (dev.stats.n_soup_vertices != host.stats.n_soup_vertices || dev.stats.n_vertices != host.stats.n_vertices ||
           dev.stats.n_faces != host.stats.n_faces || dev.stats.n_degenerate_faces != host.stats.n_degenerate_faces) diff = "stats";
  else if (!sameBits(dev.points, host.points)) diff = "points";
  else if (dev.colors != host.colors) diff = "colors";
  else if (dev.labels != host.labels) diff = "labels";
  else if (dev.first_seen_stamps != host.first_seen_stamps) diff = "first_seen";
  else if (dev.stamps != host.stamps) diff = "stamps";
  else if (dev.faces != host.faces) diff = "faces";
  else if (dev.soup_to_vertex != host.soup_to_vertex) diff = "soup_to_vertex";
  const unsigned long long ns = dev.stats.n_soup_vertices, nv = dev.stats.n_vertices, nf = dev.stats.n_faces;
  std::printf("{\"what\": \"the window's mesh as an indexed mesh: VolumetricMap::weldedMesh (device) vs khr_fetch_mesh + a one-thread host weld, %dx%d, "
              "voxel %.4g m\", \"frames\": %d, \"resolution\": %.9g, \"repeats\": %d, \"n_soup_vertices\": %llu, \"n_vertices\": %llu, \"n_faces\": %llu, "
              "\"n_degenerate_faces\": %llu, \"equal\": %s, \"first_mismatch\": \"%s\", \"device_weld_ms\": %.4f, \"fetch_ms\": %.4f, "
              "\"host_weld_ms\": %.4f, \"soup_bytes\": %llu, \"indexed_bytes\": %llu, \"soup_to_vertex_bytes\": %llu}\n",
              W, H, static_cast<double>(cfg.volumetric_map.voxel_size), N, static_cast<double>(r), reps, ns, nv, nf,
              static_cast<unsigned long long>(dev.stats.n_degenerate_faces), diff ? "false" : "true", diff ? diff : "", medianOf(t_dev),
              medianOf(t_fetch), medianOf(t_weld), 36ull * ns, 36ull * nv + 12ull * nf, 4ull * ns);
  return diff ? 3 : 0;
}

// ---- aw_demo --merge ----------------------------------------------------------------------------------------------------------
// a block of a map on the host: cloneBlock's layers plus the likelihood rows ([k][voxel], zero without a semantic entry)
struct MergeBlock {
  hydra::BlockCopy b;
  std::vector<float> lik;
};
using MergeBlocks = std::map<hydra::BlockIndex, MergeBlock>;

static MergeBlocks downloadMap(const VolumetricMap& map, int K) {
  MergeBlocks out;
  const size_t n = static_cast<size_t>(map.config.voxels_per_side) * map.config.voxels_per_side * map.config.voxels_per_side;
  for (const auto& idx : map.allocatedBlockIndices()) {
    MergeBlock& m = out[idx];
    m.b = map.cloneBlock(idx);
    m.lik.assign(n * static_cast<size_t>(K), 0.f);
    if (K > 0 && khr_download_block(map.ctx(), idx[0], idx[1], idx[2], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, m.lik.data(),
                                    nullptr) != KHR_OK)
      throw std::runtime_error(std::string("khr_download_block: ") + khr_last_error());
  }
  return out;
}

// ASSUMPTIONS.md A.17, ALIGNED with zero offset, one thread: src into dst
static khr_merge_stats hostMerge(MergeBlocks* dst, const MergeBlocks& src, size_t n, int K, float min_weight, float max_weight) {
  khr_merge_stats st{};
  st.n_src_blocks = st.n_candidate_blocks = src.size();
  for (const auto& kv : src) {
    const MergeBlock& s = kv.second;
    bool any = false;
    for (size_t v = 0; v < n && !any; ++v) any = s.b.weight[v] >= min_weight;
    if (!any) continue;
    ++st.n_touched_blocks;
    auto it = dst->find(kv.first);
    if (it == dst->end()) {
      ++st.n_new_blocks;
      MergeBlock fresh;
      fresh.b.index = kv.first;
      fresh.b.distance.assign(n, 0.f); fresh.b.weight.assign(n, 0.f); fresh.b.color.assign(4 * n, 0); fresh.b.last_observed.assign(n, 0);
      fresh.b.last_occupied.assign(n, 0); fresh.b.flags.assign(n, 0); fresh.b.semantic_label.assign(n, 0);
      fresh.lik.assign(n * static_cast<size_t>(K), 0.f);
      it = dst->emplace(kv.first, std::move(fresh)).first;
    }
    MergeBlock& d = it->second;
    bool active = false;
    for (size_t v = 0; v < n; ++v) {
      if (s.b.weight[v] >= min_weight) {
        const float ws = s.b.weight[v], wd = d.b.weight[v];
        const uint8_t fs = s.b.flags[v], fd = d.b.flags[v];
        if (wd == 0.f) {
          ++st.n_added_voxels;
          d.b.distance[v] = s.b.distance[v];
          d.b.weight[v] = std::fmin(ws, max_weight);
          for (int c = 0; c < 4; ++c) d.b.color[4 * v + c] = s.b.color[4 * v + c];
          d.b.last_observed[v] = s.b.last_observed[v];
          d.b.last_occupied[v] = s.b.last_occupied[v];
          d.b.flags[v] = fs;
          d.b.semantic_label[v] = s.b.semantic_label[v];
          for (int k = 0; k < K; ++k) d.lik[k * n + v] = (fs & KHR_VOX_SEM_VALID) ? s.lik[k * n + v] : 0.f;
        } else {
          ++st.n_merged_voxels;
          const float sum = wd + ws;
          d.b.distance[v] = (d.b.distance[v] * wd + s.b.distance[v] * ws) / sum;
          if (s.b.color[4 * v + 3] != 0) {
            if (d.b.color[4 * v + 3] == 0) {
              for (int c = 0; c < 4; ++c) d.b.color[4 * v + c] = s.b.color[4 * v + c];
            } else {
              for (int c = 0; c < 3; ++c)
                d.b.color[4 * v + c] = static_cast<uint8_t>(
                    std::floor((static_cast<float>(d.b.color[4 * v + c]) * wd + static_cast<float>(s.b.color[4 * v + c]) * ws) / sum + 0.5f));
              d.b.color[4 * v + 3] = 255;
            }
          }
          d.b.weight[v] = std::fmin(sum, max_weight);
          d.b.last_observed[v] = std::max(d.b.last_observed[v], s.b.last_observed[v]);
          d.b.last_occupied[v] = std::max(d.b.last_occupied[v], s.b.last_occupied[v]);
          if (fs & KHR_VOX_SEM_VALID) {
            if (fd & KHR_VOX_SEM_VALID) {
              float best = 0.f;
              uint32_t arg = 0;
              for (int k = 0; k < K; ++k) {
                const float l = d.lik[k * n + v] + s.lik[k * n + v];
                d.lik[k * n + v] = l;
                if (k == 0 || l > best) best = l, arg = static_cast<uint32_t>(k);
              }
              d.b.semantic_label[v] = arg;
            } else {
              for (int k = 0; k < K; ++k) d.lik[k * n + v] = s.lik[k * n + v];
              d.b.semantic_label[v] = s.b.semantic_label[v];
            }
          }
          d.b.flags[v] = static_cast<uint8_t>(((fd | fs) & (KHR_VOX_ACTIVE | KHR_VOX_SEM_VALID)) | (fd & fs & (KHR_VOX_EVER_FREE | KHR_VOX_TO_REMOVE)));
        }
      }
      active = active || (d.b.flags[v] & KHR_VOX_ACTIVE);
    }
    d.b.block_flags |= KHR_BLK_UPDATED | KHR_BLK_MESH_UPDATED | KHR_BLK_TRACKING_UPDATED | (active ? KHR_BLK_HAS_ACTIVE_DATA : 0);
  }
  return st;
}

// aw_demo --merge <config.yaml> <width> <height> <frames>: the first half of the synthetic stream through one ActiveWindow, the
// second half through another; the second map is then merged into the first on the device (VolumetricMap::merge, ALIGNED, zero
// offset) and, from copies taken before, on one host thread by the same definition.  One JSON line: whether the two results are
// equal layer for layer, the statistics, the wall-clock time of the device merge and of the host alternative (the download of both
// maps and the merge; the upload of the result, which khr_checkpoint_load would only take into an empty map, is not in it).
static int mergeDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --merge <config.yaml> <width> <height> <frames>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto q1 = std::make_shared<ActiveWindow::OutputQueue>(), q2 = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw1(cfg, q1), aw2(cfg, q2);
  void* scene = synth_create(1234, 12, 1);
  const size_t np = static_cast<size_t>(W) * H;
  std::vector<float> depth(np);
  std::vector<uint8_t> rgb(np * 3);
  std::vector<int32_t> label(np);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    const bool first = i < N / 2;
    (first ? aw1 : aw2).step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while ((first ? q1 : q2)->pop(&popped)) {}
  }
  synth_destroy(scene);
  VolumetricMap dst(aw1.getMap().config, aw1.getMap().ctx());
  const VolumetricMap& src = aw2.getMap();
  khr_config kc{};
  if (khr_get_config(dst.ctx(), &kc) != KHR_OK) throw std::runtime_error(khr_last_error());
  const int K = kc.with_semantics ? kc.num_labels : 0;
  const size_t n = static_cast<size_t>(kc.voxels_per_side) * kc.voxels_per_side * kc.voxels_per_side;
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  // the host alternative first: it needs the maps as they are before the merge
  khr_sync(dst.ctx());
  khr_sync(src.ctx());
  const auto t0 = clk::now();
  MergeBlocks hd = downloadMap(dst, K);
  const MergeBlocks hs = downloadMap(src, K);
  const size_t n_dst_before = hd.size();
  const khr_merge_stats host_st = hostMerge(&hd, hs, n, K, kc.mesh_min_weight, kc.max_weight);
  const auto t1 = clk::now();
  const khr_merge_stats st = dst.merge(src, VolumetricMap::MergeRequest{});
  khr_sync(dst.ctx());
  const auto t2 = clk::now();
  const MergeBlocks got = downloadMap(dst, K);
  aw1.finishMapping();
  aw2.finishMapping();
  std::string diff;
  if (std::memcmp(&st, &host_st, sizeof(st)) != 0) diff = "statistics";
  else if (got.size() != hd.size()) diff = "block count";
  MergeBlocks::const_iterator a = got.begin(), b = hd.begin();
  for (; diff.empty() && a != got.end(); ++a, ++b) {
    const char* layer = nullptr;
    if (a->first != b->first) layer = "block index";
    else if (!sameBits(a->second.b.distance, b->second.b.distance)) layer = "distance";
    else if (!sameBits(a->second.b.weight, b->second.b.weight)) layer = "weight";
    else if (a->second.b.color != b->second.b.color) layer = "color";
    else if (a->second.b.last_observed != b->second.b.last_observed) layer = "last_observed";
    else if (a->second.b.last_occupied != b->second.b.last_occupied) layer = "last_occupied";
    else if (a->second.b.flags != b->second.b.flags) layer = "flags";
    else if (a->second.b.semantic_label != b->second.b.semantic_label) layer = "sem_label";
    else if (!sameBits(a->second.lik, b->second.lik)) layer = "likelihoods";
    else if (a->second.b.block_flags != b->second.b.block_flags) layer = "block_flags";
    if (layer) diff = std::string(layer) + " of block (" + std::to_string(a->first[0]) + ", " + std::to_string(a->first[1]) + ", " + std::to_string(a->first[2]) + ")";
  }
  std::printf("{\"what\": \"two half streams, the second map merged into the first: VolumetricMap::merge (device) vs block copies merged on one host "
              "thread, %dx%d, voxel %.4g m\", \"frames\": %d, \"n_dst_blocks\": %zu, \"n_src_blocks\": %llu, \"n_candidate_blocks\": %llu, "
              "\"n_touched_blocks\": %llu, \"n_new_blocks\": %llu, \"n_added_voxels\": %llu, \"n_merged_voxels\": %llu, \"equal\": %s, "
              "\"first_mismatch\": \"%s\", \"device_merge_ms\": %.4f, \"host_merge_ms\": %.4f}\n",
              W, H, static_cast<double>(kc.voxel_size), N, n_dst_before, static_cast<unsigned long long>(st.n_src_blocks),
              static_cast<unsigned long long>(st.n_candidate_blocks), static_cast<unsigned long long>(st.n_touched_blocks),
              static_cast<unsigned long long>(st.n_new_blocks), static_cast<unsigned long long>(st.n_added_voxels),
              static_cast<unsigned long long>(st.n_merged_voxels), diff.empty() ? "true" : "false", diff.c_str(), ms(t1, t2), ms(t0, t1));
  return diff.empty() ? 0 : 3;
}

// ---- aw_demo --diff -----------------------------------------------------------------------------------------------------------
using DiffBlocks = std::map<hydra::BlockIndex, hydra::BlockCopy>;

static DiffBlocks downloadBlocks(const VolumetricMap& map) {
  DiffBlocks out;
  for (const auto& idx : map.allocatedBlockIndices()) out[idx] = map.cloneBlock(idx);
  return out;
}

// ASSUMPTIONS.md A.18, ALIGNED with zero offset, one thread: `now` against `then` from block copies.  The candidates are the blocks
// of `then`; the map's order is the (x, y, z) order of the result.
static hydra::MapDiff hostDiff(const DiffBlocks& now, const DiffBlocks& then, int vps, float min_weight, float occupied, float free_d, bool sem,
                               bool trk) {
  hydra::MapDiff d;
  d.stats.n_ref_blocks = d.stats.n_candidate_blocks = then.size();
  const size_t n = static_cast<size_t>(vps) * vps * vps;
  for (const auto& kv : now) {
    const auto it = then.find(kv.first);
    if (it == then.end()) continue;
    ++d.stats.n_present_blocks;
    const hydra::BlockCopy& a = kv.second;
    const hydra::BlockCopy& b = it->second;
    uint32_t n_app = 0, n_dis = 0;
    const uint32_t first = static_cast<uint32_t>(d.kind.size());
    for (size_t v = 0; v < n; ++v) {
      const bool N = a.weight[v] >= min_weight, T = b.weight[v] >= min_weight;
      if (N && !T) ++d.stats.n_only_now;
      if (!N && T) ++d.stats.n_only_then;
      if (!(N && T)) continue;
      ++d.stats.n_compared_voxels;
      const float dn = a.distance[v], dt = b.distance[v];
      const bool app = dt >= free_d && dn <= occupied, dis = dt <= occupied && dn >= free_d;
      if (!app && !dis) continue;
      app ? ++n_app : ++n_dis;
      d.voxels.push_back(kv.first[0] * vps + static_cast<int32_t>(v % vps));
      d.voxels.push_back(kv.first[1] * vps + static_cast<int32_t>((v / vps) % vps));
      d.voxels.push_back(kv.first[2] * vps + static_cast<int32_t>(v / (static_cast<size_t>(vps) * vps)));
      d.kind.push_back(app ? hydra::MapDiff::kAppeared : hydra::MapDiff::kDisappeared);
      d.d_now.push_back(dn);
      d.d_then.push_back(dt);
      d.label.push_back(sem ? (app ? a.semantic_label[v] : b.semantic_label[v]) : 0u);
      d.stamp_now.push_back(trk ? a.last_observed[v] : 0ull);
      d.stamp_then.push_back(trk ? b.last_observed[v] : 0ull);
    }
    d.stats.n_appeared += n_app;
    d.stats.n_disappeared += n_dis;
    if (n_app + n_dis == 0) continue;
    ++d.stats.n_changed_blocks;
    for (int k = 0; k < 3; ++k) d.blocks.push_back(kv.first[k]);
    d.block_appeared.push_back(n_app);
    d.block_disappeared.push_back(n_dis);
    d.block_first.push_back(first);
  }
  return d;
}

// aw_demo --diff <config.yaml> <width> <height> <frames>: the synthetic stream through one ActiveWindow; halfway the live map is
// checkpointed into a side context; at the end the live map is compared with the side context on the device
// (VolumetricMap::diff, ALIGNED, zero offset, the default thresholds) and, from block copies of both maps, on one host thread by the
// same definition.  One JSON line: whether the two results are equal list for list, the statistics, and wall-clock times: the
// device diff through the completion of its last kernel (the first call, which creates the scratch, and a repeat), the diff with
// the copy of its lists to the host, and the host alternative (the download of both maps and the comparison).
static int diffDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --diff <config.yaml> <width> <height> <frames>\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]);
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  void* scene = synth_create(1234, 12, 1);
  const size_t np = static_cast<size_t>(W) * H;
  std::vector<float> depth(np);
  std::vector<uint8_t> rgb(np * 3);
  std::vector<int32_t> label(np);
  khr_ctx* side = nullptr;
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
    if (i + 1 == N / 2) {  // the checkpoint, through memory
      khr_ctx* live = aw.getMap().ctx();
      khr_config kc{};
      uint64_t bytes = 0, written = 0;
      int64_t blocks = 0, kept = 0;
      if (khr_get_config(live, &kc) != KHR_OK || khr_checkpoint_size(live, &bytes, &blocks) != KHR_OK) throw std::runtime_error(khr_last_error());
      std::vector<uint8_t> buf(bytes);
      if (khr_checkpoint_save(live, buf.data(), bytes, &written) != KHR_OK) throw std::runtime_error(std::string("khr_checkpoint_save: ") + khr_last_error());
      if (khr_create(&kc, &side) != KHR_OK) throw std::runtime_error(std::string("khr_create: ") + khr_last_error());
      if (khr_checkpoint_load(side, buf.data(), written, &kept) != KHR_OK || kept != blocks)
        throw std::runtime_error(std::string("khr_checkpoint_load: ") + khr_last_error());
    }
  }
  synth_destroy(scene);
  if (!side) throw std::runtime_error("aw_demo --diff needs at least two frames");
  const VolumetricMap& now = aw.getMap();
  const VolumetricMap then(now.config, side);
  khr_config kc{};
  if (khr_get_config(now.ctx(), &kc) != KHR_OK) throw std::runtime_error(khr_last_error());
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  khr_sync(now.ctx());
  khr_sync(side);
  const auto t0 = clk::now();
  const DiffBlocks hn = downloadBlocks(now), ht = downloadBlocks(then);
  const hydra::MapDiff host = hostDiff(hn, ht, kc.voxels_per_side, kc.mesh_min_weight, 0.f, kc.voxel_size, kc.with_semantics != 0, kc.with_tracking != 0);
  const auto t1 = clk::now();
  khr_diff_request rq{};
  rq.mode = KHR_MERGE_ALIGNED;
  rq.ctx_T_ref[0] = rq.ctx_T_ref[5] = rq.ctx_T_ref[10] = rq.ctx_T_ref[15] = 1.0;
  rq.occupied_distance = 0.f;
  rq.free_distance = kc.voxel_size;
  double call_ms[2];
  for (int r = 0; r < 2; ++r) {
    const auto a = clk::now();
    if (khr_diff_map(now.ctx(), side, &rq, nullptr) != KHR_OK) throw std::runtime_error(std::string("khr_diff_map: ") + khr_last_error());
    khr_sync(now.ctx());
    call_ms[r] = ms(a, clk::now());
  }
  const auto t2 = clk::now();
  const hydra::MapDiff dev = now.diff(then, VolumetricMap::DiffRequest{});
  const auto t3 = clk::now();
  aw.finishMapping();
  khr_destroy(side);
  const char* diff = nullptr;
  if (std::memcmp(&dev.stats, &host.stats, sizeof(dev.stats)) != 0) diff = "statistics";
  else if (dev.voxels != host.voxels) diff = "voxels";
  else if (dev.kind != host.kind) diff = "kind";
  else if (!sameBits(dev.d_now, host.d_now)) diff = "d_now";
  else if (!sameBits(dev.d_then, host.d_then)) diff = "d_then";
  else if (dev.label != host.label) diff = "label";
  else if (dev.stamp_now != host.stamp_now) diff = "stamp_now";
  else if (dev.stamp_then != host.stamp_then) diff = "stamp_then";
  else if (dev.blocks != host.blocks) diff = "blocks";
  else if (dev.block_appeared != host.block_appeared) diff = "block_appeared";
  else if (dev.block_disappeared != host.block_disappeared) diff = "block_disappeared";
  else if (dev.block_first != host.block_first) diff = "block_first";
  const khr_diff_stats& st = dev.stats;
  auto u = [](uint64_t v) { return static_cast<unsigned long long>(v); };
  std::printf("{\"what\": \"one stream, the live map against its own checkpoint of frame %d: VolumetricMap::diff (device) vs block copies compared on "
              "one host thread, %dx%d, voxel %.4g m\", \"frames\": %d, \"n_now_blocks\": %zu, \"n_ref_blocks\": %llu, \"n_candidate_blocks\": %llu, "
              "\"n_present_blocks\": %llu, \"n_compared_voxels\": %llu, \"n_appeared\": %llu, \"n_disappeared\": %llu, \"n_only_now\": %llu, "
              "\"n_only_then\": %llu, \"n_changed_blocks\": %llu, \"equal\": %s, \"first_mismatch\": \"%s\", \"device_diff_first_ms\": %.4f, "
              "\"device_diff_ms\": %.4f, \"diff_with_lists_ms\": %.4f, \"host_diff_ms\": %.4f}\n",
              N / 2, W, H, static_cast<double>(kc.voxel_size), N, hn.size(), u(st.n_ref_blocks), u(st.n_candidate_blocks), u(st.n_present_blocks),
              u(st.n_compared_voxels), u(st.n_appeared), u(st.n_disappeared), u(st.n_only_now), u(st.n_only_then), u(st.n_changed_blocks),
              diff ? "false" : "true", diff ? diff : "", call_ms[0], call_ms[1], ms(t2, t3), ms(t0, t1));
  return diff ? 3 : 0;
}

// ---- aw_demo --segment --------------------------------------------------------------------------------------------------------
// ASSUMPTIONS.md A.19 on one thread from block copies: the members into a hash of their global voxel indices, in voxel order; a
// breadth-first flood fill from every member not yet reached; the components in the order their least voxels come up.
static hydra::MapSegments hostSegment(const DiffBlocks& blocks, int vps, float min_weight, float surface_distance, int connectivity, bool by_label,
                                      bool sem, bool trk, bool want_voxels) {
  struct Member {
    int32_t g[3];
    uint32_t label;
    uint64_t stamp;
  };
  std::vector<Member> mem;
  struct VoxelHash {
    size_t operator()(const std::array<int32_t, 3>& k) const {
      uint64_t h = static_cast<uint32_t>(k[0]) * 0x9e3779b97f4a7c15ull;
      h = (h ^ (h >> 29)) + static_cast<uint32_t>(k[1]) * 0xbf58476d1ce4e5b9ull;
      h = (h ^ (h >> 31)) + static_cast<uint32_t>(k[2]) * 0x94d049bb133111ebull;
      return static_cast<size_t>(h ^ (h >> 32));
    }
  };
  std::unordered_map<std::array<int32_t, 3>, uint32_t, VoxelHash> at;
  auto key = [](int32_t x, int32_t y, int32_t z) { return std::array<int32_t, 3>{x, y, z}; };
  const size_t nv = static_cast<size_t>(vps) * vps * vps;
  for (const auto& kv : blocks) {  // (std::map: the (x, y, z) order)
    const hydra::BlockCopy& b = kv.second;
    for (size_t v = 0; v < nv; ++v) {
      if (!(b.weight[v] >= min_weight && b.distance[v] <= surface_distance)) continue;
      Member m;
      m.g[0] = kv.first[0] * vps + static_cast<int32_t>(v % vps);
      m.g[1] = kv.first[1] * vps + static_cast<int32_t>((v / vps) % vps);
      m.g[2] = kv.first[2] * vps + static_cast<int32_t>(v / (static_cast<size_t>(vps) * vps));
      m.label = sem ? b.semantic_label[v] : 0u;
      m.stamp = trk ? b.last_observed[v] : 0ull;
      at[key(m.g[0], m.g[1], m.g[2])] = static_cast<uint32_t>(mem.size());
      mem.push_back(m);
    }
  }
  std::vector<std::array<int, 3>> steps;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int n = std::abs(dx) + std::abs(dy) + std::abs(dz);
        if (n >= 1 && n <= (connectivity == 6 ? 1 : (connectivity == 18 ? 2 : 3))) steps.push_back({dx, dy, dz});
      }
  hydra::MapSegments s;
  s.stats.n_blocks = blocks.size();
  s.stats.n_member_voxels = mem.size();
  std::vector<uint8_t> seen(mem.size(), 0);
  std::vector<uint32_t> comp;
  for (uint32_t start = 0; start < mem.size(); ++start) {
    if (seen[start]) continue;
    seen[start] = 1;
    comp.assign(1, start);
    for (size_t q = 0; q < comp.size(); ++q) {  // (the component's list is the queue)
      const Member m = mem[comp[q]];
      for (const auto& d : steps) {
        const auto it = at.find(key(m.g[0] + d[0], m.g[1] + d[1], m.g[2] + d[2]));
        if (it == at.end() || seen[it->second] || (by_label && mem[it->second].label != m.label)) continue;
        seen[it->second] = 1;
        comp.push_back(it->second);
      }
    }
    std::sort(comp.begin(), comp.end());
    ++s.stats.n_components_all, ++s.stats.n_components;  // (min_voxels = 1, no upper limit: every component is kept)
    const uint32_t id = static_cast<uint32_t>(s.stats.n_components);
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    int64_t sum[3] = {0, 0, 0};
    uint64_t last = 0;
    for (uint32_t i : comp) {
      for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(lo[a], mem[i].g[a]), hi[a] = std::max(hi[a], mem[i].g[a]), sum[a] += mem[i].g[a];
        if (want_voxels) s.voxels.push_back(mem[i].g[a]);
      }
      last = std::max(last, mem[i].stamp);
      if (want_voxels) s.voxel_component.push_back(id);
    }
    s.label.push_back(static_cast<int32_t>(mem[start].label));
    s.n_voxels.push_back(comp.size());
    for (int a = 0; a < 3; ++a) {
      s.bbox_min.push_back(lo[a]), s.bbox_max.push_back(hi[a]), s.sum.push_back(sum[a]), s.representative.push_back(mem[start].g[a]);
    }
    s.last_observed_max.push_back(last);
    s.first.push_back(s.stats.n_voxels);
    s.stats.n_voxels += comp.size();
  }
  return s;
}

// aw_demo --segment <config.yaml> <width> <height> <frames> [connectivity]: the synthetic stream through one ActiveWindow; then the
// live map is segmented on the device (VolumetricMap::segment: the defaults, every component kept, with the voxel list) and, from
// block copies, on one host thread by a breadth-first flood fill.  One JSON line: whether the two results are equal array for
// array, the statistics, and wall-clock times: the device call through the completion of its last kernel (the first call, which
// creates the scratch, a repeat, and a repeat once the host knows the live block count and the scratch is sized by it), the call
// with the copy of its arrays to the host, and the host alternative (the download of the map and the flood fill).
static int segmentDemo(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: aw_demo --segment <config.yaml> <width> <height> <frames> [connectivity]\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), N = std::atoi(argv[5]), connectivity = argc > 6 ? std::atoi(argv[6]) : 26;
  ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
  cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
  auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
  ActiveWindow aw(cfg, out_queue);
  void* scene = synth_create(1234, 12, 1);
  const size_t np = static_cast<size_t>(W) * H;
  std::vector<float> depth(np);
  std::vector<uint8_t> rgb(np * 3);
  std::vector<int32_t> label(np);
  for (int i = 0; i < N; ++i) {
    hydra::InputPacket pkt;
    pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
    circlePose(0.1 * i, pkt.world_T_body);
    pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
    synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                 1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
    pkt.depth = depth.data();
    pkt.color = rgb.data();
    pkt.labels = label.data();
    aw.step(pkt);
    hydra::ActiveWindowOutput::Ptr popped;
    while (out_queue->pop(&popped)) {}
  }
  synth_destroy(scene);
  const VolumetricMap& map = aw.getMap();
  khr_config kc{};
  if (khr_get_config(map.ctx(), &kc) != KHR_OK) throw std::runtime_error(khr_last_error());
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  khr_sync(map.ctx());
  khr_segment_request rq{};
  rq.connectivity = connectivity;
  rq.by_label = kc.with_semantics != 0;
  rq.min_voxels = 1;
  rq.want_voxels = 1;
  double call_ms[2];
  for (int r = 0; r < 2; ++r) {  // (right after a frame the host knows no block count: the scratch is sized by the pool)
    const auto a = clk::now();
    if (khr_segment_map(map.ctx(), &rq, nullptr) != KHR_OK) throw std::runtime_error(std::string("khr_segment_map: ") + khr_last_error());
    khr_sync(map.ctx());
    call_ms[r] = ms(a, clk::now());
  }
  const auto t0 = clk::now();
  const DiffBlocks blocks = downloadBlocks(map);
  const auto t1 = clk::now();
  const hydra::MapSegments host = hostSegment(blocks, kc.voxels_per_side, kc.mesh_min_weight, 0.f, connectivity, rq.by_label != 0, kc.with_semantics != 0,
                                              kc.with_tracking != 0, true);
  const auto t2 = clk::now();
  double live_ms = 0.0;
  {  // (the download has brought the host index up to date: the scratch is sized by the live blocks now)
    const auto a = clk::now();
    if (khr_segment_map(map.ctx(), &rq, nullptr) != KHR_OK) throw std::runtime_error(std::string("khr_segment_map: ") + khr_last_error());
    khr_sync(map.ctx());
    live_ms = ms(a, clk::now());
  }
  const auto t2b = clk::now();
  VolumetricMap::SegmentRequest srq;
  srq.connectivity = connectivity;
  const hydra::MapSegments dev = map.segment(srq);
  const auto t3 = clk::now();
  aw.finishMapping();
  const char* diff = nullptr;
  if (std::memcmp(&dev.stats, &host.stats, sizeof(dev.stats)) != 0) diff = "statistics";
  else if (dev.label != host.label) diff = "label";
  else if (dev.n_voxels != host.n_voxels) diff = "n_voxels";
  else if (dev.bbox_min != host.bbox_min) diff = "bbox_min";
  else if (dev.bbox_max != host.bbox_max) diff = "bbox_max";
  else if (dev.sum != host.sum) diff = "sum";
  else if (dev.representative != host.representative) diff = "representative";
  else if (dev.last_observed_max != host.last_observed_max) diff = "last_observed_max";
  else if (dev.first != host.first) diff = "first";
  else if (dev.voxels != host.voxels) diff = "voxels";
  else if (dev.voxel_component != host.voxel_component) diff = "voxel_component";
  const khr_segment_stats& st = dev.stats;
  uint64_t largest = 0;
  for (uint64_t n : dev.n_voxels) largest = std::max(largest, n);
  auto u = [](uint64_t v) { return static_cast<unsigned long long>(v); };
  std::printf("{\"what\": \"one stream, then the connected components of the live map: VolumetricMap::segment (device) vs a breadth-first flood fill "
              "over block copies on one host thread, %dx%d, voxel %.4g m, connectivity %d, by_label %d\", \"frames\": %d, \"n_blocks\": %llu, "
              "\"n_member_voxels\": %llu, \"n_components\": %llu, \"n_voxels\": %llu, \"largest_component\": %llu, \"equal\": %s, "
              "\"first_mismatch\": \"%s\", \"device_segment_first_ms\": %.4f, \"device_segment_ms\": %.4f, \"device_segment_live_sized_ms\": %.4f, "
              "\"segment_with_arrays_ms\": %.4f, "
              "\"host_download_ms\": %.4f, \"host_flood_fill_ms\": %.4f}\n",
              W, H, static_cast<double>(kc.voxel_size), connectivity, rq.by_label, N, u(st.n_blocks), u(st.n_member_voxels), u(st.n_components),
              u(st.n_voxels), u(largest), diff ? "false" : "true", diff ? diff : "", call_ms[0], call_ms[1], live_ms, ms(t2b, t3), ms(t0, t1), ms(t1, t2));
  return diff ? 3 : 0;
}

int main(int argc, char** argv) {
  std::signal(SIGSEGV, onSegv);
  std::signal(SIGABRT, onSegv);
  if (argc >= 2 && std::string(argv[1]) == "--segment") {
    try {
      return segmentDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--diff") {
    try {
      return diffDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--merge") {
    try {
      return mergeDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--weld") {
    try {
      return weldDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 3 && std::string(argv[1]) == "--rayver") {
    try {
      return rayverDemo(argv[2]);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--slices") {
    try {
      return slicesDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--query") {
    try {
      return queryDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--distance") {
    try {
      return distanceDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--voronoi") {
    try {
      return voronoiDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--places") {
    try {
      return placesDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--travel") {
    try {
      return travelDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--render") {
    try {
      return renderDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--align") {
    try {
      return alignDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--checkpoint") {
    try {
      return checkpointDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "--bench") {
    try {
      return benchDemo(argc, argv);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "aw_demo: %s\n", e.what());
      return 1;
    }
  }
  if (argc < 5) {
    std::fprintf(stderr, "usage: aw_demo <config.yaml> <width> <height> <frames> [object_label] [timing_stats.csv]\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  std::stringstream ss;
  ss << in.rdbuf();
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), N = std::atoi(argv[4]);
  const int object_label = argc > 5 ? std::atoi(argv[5]) : -1;
  try {
    ActiveWindow::Config cfg = ActiveWindow::Config::fromYamlString(ss.str());
    cfg.max_frame_pixels = static_cast<uint32_t>(W) * H;
    auto out_queue = std::make_shared<ActiveWindow::OutputQueue>();
    ActiveWindow aw(cfg, out_queue);
    LabelObjectDetector* det = nullptr;
    if (object_label >= 0) {
      auto d = std::make_unique<LabelObjectDetector>(object_label);
      det = d.get();
      aw.setObjectDetector(std::move(d));
      aw.setTracker(std::make_unique<SingleTrackTracker>());
    }
    int sink_calls = 0;
    // (a window without sinks queues the detector's kernels and an output's device stages with the frame's fused call and defers the
    //  tracker's association, ActiveWindow::Config::fuse_device_stages: tests run both forms and compare)
    if (!std::getenv("AW_DEMO_NO_SINK")) aw.addKhronosSink([&](const FrameData&, const VolumetricMap&, const Tracks&) { ++sink_calls; });

    void* scene = synth_create(1234, 12, 1);
    std::vector<float> depth(static_cast<size_t>(W) * H);
    std::vector<uint8_t> rgb(static_cast<size_t>(W) * H * 3);
    std::vector<int32_t> label(static_cast<size_t>(W) * H);
    std::printf("{\"info\": \"%s\", \"outputs\": [", aw.printInfo().c_str());
    int n_out = 0;
    size_t n_popped = 0;
    hydra::ActiveWindowOutput::Ptr first_out;  // kept like the frontend's queue keeps it: read after the map has moved on
    std::vector<float> first_depth;
    std::vector<uint8_t> first_rgb;
    std::vector<int32_t> first_label;
    size_t total_dyn_clusters = 0, total_sem_clusters = 0;
    for (int i = 0; i < N; ++i) {
      hydra::InputPacket pkt;
      pkt.timestamp_ns = static_cast<uint64_t>(std::llround((1.0 + 0.1 * i) * 1e9));
      circlePose(0.1 * i, pkt.world_T_body);
      pkt.sensor = {W, H, W / 2.f, W / 2.f, W / 2.f, H / 2.f, 0.1f, 5.f};
      synth_render(scene, W, H, pkt.sensor.fx, pkt.sensor.fy, pkt.sensor.cx, pkt.sensor.cy, pkt.world_T_body, 0.1 * i, 5.f, 0.f,
                   1234u + 7919u * i, depth.data(), rgb.data(), label.data(), 0);
      pkt.depth = depth.data();
      pkt.color = rgb.data();
      pkt.labels = label.data();
      if (det) det->current_labels = label.data();
      auto out = aw.step(pkt);  // the module thread's iteration: spinOnce (protected) + output queue
      {  // the consumer (hydra frontend role): takes what the module queued
        hydra::ActiveWindowOutput::Ptr popped;
        while (out_queue->pop(&popped)) n_popped += popped == out ? 1 : 0;
      }
      total_dyn_clusters += aw.getLatestFrameData().num_dynamic_clusters;
      total_sem_clusters += aw.getLatestFrameData().semantic_clusters.size();
      if (out) {
        std::printf("%s{\"stamp\": %" PRIu64 ", \"updated\": %zu, \"archived\": %zu, \"objects\": %zu}", n_out ? ", " : "", out->timestamp_ns,
                    out->updatedBlocks().size(), out->archived_mesh_indices.size(), out->graph_update.size());
        if (!first_out) {
          first_out = out;
          first_depth = depth;
          first_rgb = rgb;
          first_label = label;
        }
        ++n_out;
      }
    }
    // map checksum in sorted block order
    double checksum = 0;
    size_t n_blocks = aw.getMap().numBlocks();
    for (const auto& idx : aw.getMap().allocatedBlockIndices()) {
      const hydra::BlockCopy b = aw.getMap().cloneBlock(idx);
      for (size_t k = 0; k < b.distance.size(); ++k) checksum += static_cast<double>(b.distance[k]) * b.weight[k];
    }
    const size_t n_tracks_before = aw.getTracks().size();
    std::string track_json = "[";
    for (const Track& t : aw.getTracks()) {
      char buf[256];
      std::snprintf(buf, sizeof(buf), "%s{\"id\": %d, \"dyn\": %d, \"active\": %d, \"conf\": %.9g, \"cat\": %d, \"n_obs\": %zu, \"first\": %" PRIu64
                    ", \"last\": %" PRIu64 "}", track_json.size() > 1 ? ", " : "", t.id, int(t.is_dynamic), int(t.is_active), t.confidence,
                    t.semantics ? t.semantics->category_id : -1, t.observations.size(), t.first_seen, t.last_seen);
      track_json += buf;
    }
    track_json += "]";
    auto objects = aw.extractObjects();
    std::printf("], \"n_outputs\": %d, \"sink_calls\": %d, \"dynamic_clusters\": %zu, \"n_blocks\": %zu, \"checksum\": %.17g, "
                "\"tracks\": %zu, \"track_list\": %s, \"semantic_clusters\": %zu, \"objects\": [",
                n_out, sink_calls, total_dyn_clusters, n_blocks, checksum, n_tracks_before, track_json.c_str(), total_sem_clusters);
    for (size_t k = 0; k < objects.size(); ++k) {
      const auto& o = *objects[k];
      std::printf("%s{\"label\": %d, \"dynamic\": %d, \"vertices\": %zu, \"bbox_min\": [%.6f, %.6f, %.6f], \"bbox_max\": [%.6f, %.6f, %.6f]}", k ? ", " : "",
                  o.semantic_label, int(!o.trajectory_positions.empty()), o.mesh.numVertices(), o.bounding_box.min[0], o.bounding_box.min[1], o.bounding_box.min[2], o.bounding_box.max[0],
                  o.bounding_box.max[1], o.bounding_box.max[2]);
    }
    aw.finishMapping();
    std::printf("], \"blocks_after_finish\": %zu, \"ring_waits\": %zu, \"queued_outputs\": %zu", aw.getMap().numBlocks(), aw.numRingWaits(),
                n_popped);
    if (first_out) {  // the first output's map clone, read only now (every block has been archived by finishMapping)
      double sum = 0;
      const auto blocks = first_out->cloneUpdatedTsdf();
      for (const auto& b : blocks)
        for (size_t k = 0; k < b.distance.size(); ++k) sum += static_cast<double>(b.distance[k]) * b.weight[k];
      std::printf(", \"first_output_clone\": {\"blocks\": %zu, \"checksum\": %.17g}", blocks.size(), sum);
      // ... and its sensor_data (active_window.cpp:165): the images of ITS frame, long after the ring slot has been reused
      const auto& sd = *first_out->sensor_data;
      const std::vector<float> d = sd.depthImage(), r = sd.rangeImage(), vm = sd.vertexMap();
      const std::vector<uint8_t> c = sd.colorImage();
      const std::vector<int32_t> l = sd.labelImage();
      size_t range_valid = 0, vertex_set = 0;
      for (size_t k = 0; k < r.size(); ++k) {
        range_valid += r[k] > 0.f ? 1 : 0;
        vertex_set += (k < vm.size() / 3 && (vm[3 * k] != 0.f || vm[3 * k + 1] != 0.f || vm[3 * k + 2] != 0.f)) ? 1 : 0;
      }
      std::printf(", \"first_output_images\": {\"depth_equal\": %s, \"color_equal\": %s, \"labels_equal\": %s, \"range_valid\": %zu, \"vertices\": %zu, "
                  "\"pixels\": %zu}", d == first_depth ? "true" : "false", c == first_rgb ? "true" : "false", l == first_label ? "true" : "false",
                  range_valid, vertex_set, r.size());
      first_out.reset();
    }
    // timing/stats.csv of the reference's experiment manager (experiment_manager.cpp:251-258), same scope names
    if (argc > 6) hydra::timing::ElapsedTimeRecorder::instance().logStats(argv[6]);
    std::printf(", \"timing\": {");
    bool first_t = true;
    for (const auto& kv : hydra::timing::ElapsedTimeRecorder::instance().stats()) {
      std::printf("%s\"%s\": {\"count\": %llu, \"mean_ms\": %.4f}", first_t ? "" : ", ", kv.first.c_str(),
                  static_cast<unsigned long long>(kv.second.count), 1e3 * kv.second.sum / static_cast<double>(kv.second.count));
      first_t = false;
    }
    std::printf("}}\n");
    synth_destroy(scene);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "aw_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
