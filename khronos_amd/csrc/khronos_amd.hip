// khronos_amd.hip — implementation of the C ABI declared in include/khronos_amd.h.
// Host code here only owns HBM buffers, enqueues the gfx950 kernels on one HIP stream and does the
// small sequential parts of the path (motion-cluster graph walk) that the reference also runs
// sequentially (free_space_motion_detector.cpp:205-379).  There is deliberately NO CPU fallback for any
// kernel: without a HIP device khr_create fails.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <climits>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/khronos_amd.h"
#include "khr_device.h"
#include "khr_owned.h"
#include "khr_box_host.h"
#include "khr_kernels_aux.h"
#include "khr_kernels_fusion.h"
#include "khr_kernels_fuse.h"
#include "khr_kernels_objects.h"
#include "khr_kernels_slice.h"
#include "khr_kernels_render.h"
#include "khr_kernels_query.h"
#include "khr_kernels_distance.h"
#include "khr_kernels_align.h"
#include "khr_kernels_checkpoint.h"
#include "khr_kernels_weld.h"
#include "khr_kernels_merge.h"
#include "khr_kernels_diff.h"
#include "khr_kernels_segment.h"
#include "khr_kernels_voronoi.h"
#include "khr_kernels_places.h"
#include "khr_kernels_travel.h"

using namespace khr;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(KHR_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define KHR_TRY(expr)                  \
  do {                                 \
    if (int _rc = (expr)) return _rc;  \
  } while (0)

// a chain of allocations that stops at its first failure: the argument is evaluated only while `rc` is still KHR_OK
#define KHR_CHAIN(...)                       \
  do {                                       \
    if (rc == KHR_OK) rc = (__VA_ARGS__);    \
  } while (0)

struct FrameSlot {
  // the slot's own planes: views into blocks the context's `allocs` own (khr_create)
  float* depth = nullptr;
  float* range = nullptr;
  uint32_t* rgba = nullptr;
  int32_t* label = nullptr;
  int32_t* dyn = nullptr;
  uint8_t* dynw = nullptr;  // beside the dynamic image: how often the reference's cluster.pixels lists each painted pixel (k_md_paint)
  int32_t* obj = nullptr;
  uint8_t* rgb_staging = nullptr;
  float* tile_max = nullptr;
  // adopted frames (khr_tick_adopt): the converted planes stay where the caller has them (e.g. the receive buffer of the
  // ranks' all-gather) and the slot only refers to them; nullptr = the slot's own arrays.  Reset when the slot is re-acquired.
  const float* x_depth = nullptr;
  const float* x_range = nullptr;
  const uint32_t* x_rgba = nullptr;
  const int32_t* x_label = nullptr;
  const float* x_tile_max = nullptr;
  const float* vDepth() const { return x_depth ? x_depth : depth; }
  const float* vRange() const { return x_range ? x_range : range; }
  const uint32_t* vRgba() const { return x_rgba ? x_rgba : rgba; }
  const int32_t* vLabel() const { return x_label ? x_label : label; }
  const float* vTileMax() const { return x_tile_max ? x_tile_max : tile_max; }
  int tw = 0, th = 0;
  khr_sensor sensor{};
  khr_frame meta{};
  bool valid = false, has_color = false, has_label = false, has_obj = false, objects_done = false;
  bool dyn_clean = false;  // the dynamic image is all zero (fresh from ingest, nothing painted yet)
  bool dynw_valid = false; // the weight image belongs to the dynamic image (painted here, not installed by khr_set_frame_image)
  uint64_t aux_seq = 0;    // sequence number of the last auxiliary-stream batch that read / wrote this slot (0 = none)
  std::vector<khr_cluster> sem_clusters;  // semantic clusters of the frame in this slot (khr_detect_objects)
  std::vector<khr_cluster> clusters;  // dynamic clusters of the frame in this slot (ids, listed pixel counts)
};

struct TimingRec {
  int which;
  Event a, b;
};

constexpr int kNumTimers = 13;  // 0..7: kernel groups; 8..12: single kernels (k_marching_cubes count / emit, k_tracking_update, k_ever_free, k_snapshot_pack)
constexpr uint32_t kObjHead = 512;   // cluster records in the first download of the object detector
constexpr uint32_t kCvHead = 8192;   // (cluster, voxel) keys in the first download of a voxel-set request
constexpr int kGvReleaseGrid = 64;   // workgroups of k_gv_release_publish: a few thousand slots to free, one returning atomic per workgroup
constexpr uint32_t kCompCap = 1024, kCompHead = 64;  // motion-cluster components: record capacity / records in the first download

}  // namespace

struct khr_ctx {
  khr_config cfg{};
  DevParams p{};
  DevMap m{};
  int device = 0;
  // Lifetime: a member either owns its resource (DevBuf / PinnedBuf / Event / Stream, khr_owned.h) or is a view of memory another
  // member owns and says so.  The streams come first, so that they are destroyed last: behind every buffer and event.
  Stream stream;  // the context's own, or the caller's (khr_set_stream: referred to, not owned)
  // second stream for the object detector / voxel-set kernels: they only read the frame, so they run beside the
  // volumetric kernels of the same frame instead of in front of them.  ev_aux orders it behind the main stream where
  // it has to be (the frame's ingest, a painted dynamic image), ev_aux_done orders consumers of the object image behind it.
  Stream aux_stream;
  Stream copy_stream;  // khr_snapshot_download_begin: device -> host copies beside the frames' kernels
  Stream snap_stream;  // khr_process_frame: the output's snapshot beside its marching cubes (both only read the voxel layers)
  Stream mc_stream;    // khr_process_frame: the output's marching cubes beside the tracking pass
  // pinned host input (KHR_PF_INPUT_PINNED / khr_ingest_ahead_host): the frame's three planes travel on a stream of their own
  // into the ring slot, the ingest kernel waits for them on the device; the host does not wait (round 5)
  Stream h2d_stream;
  Event ev_aux, ev_aux_done;
  // batches queued on the auxiliary stream are numbered; aux_seq_done = the latest one the host KNOWS to be complete
  // (a ticket it waited for, an idle stream): a frame slot is only re-ingested when its last batch is
  uint64_t aux_seq_issued = 0, aux_seq_done = 0, obj_seq = 0, cv_seq[3] = {0, 0, 0};  // (cv_seq: per result set, see d_cv_n)
  std::vector<DevBuf<uint8_t>> allocs;  // every buffer that lives as long as the context (devAlloc); the raw pointers below without
                                        // an owner type, DevMap m, MeshBuffers mesh[] and the frame slots' planes are views into these
  std::vector<FrameSlot> slots;
  int next_slot = 0;
  std::unique_ptr<std::atomic<int>[]> slot_leases;  // khr_retain_slot: frames somebody still reads are not overwritten
  // work lists
  uint32_t* d_work = nullptr;
  uint32_t* d_new = nullptr;
  uint32_t* d_ef = nullptr;
  uint32_t* d_trk_proc = nullptr;
  // tick path (khr_tick_*): per-camera work lists [kMaxTick][capacity], {visible, non-culled} counts, seed counts,
  // second record-cursor set, pinned result block (kMaxTick counts + ticket)
  uint32_t* d_tick_work = nullptr;
  uint32_t* d_tick_counts = nullptr;
  uint32_t* d_tick_seeds = nullptr;
  PinnedBuf<uint32_t> h_tick;
  uint32_t tick_ticket = 0;
  std::vector<uint32_t> tick_seed_host;  // seed counts of the latest khr_tick_ingest (collected lazily)
  int tick_seed_n = 0, tick_seed_collected = 0;
  // between the allocation and the update phase of a tick: the epoch the tick's new blocks carry (the motion detector
  // must not see them: in reference order it runs before the frames are integrated); 0 otherwise
  int tick_epoch = 0, motion_ignore_epoch = 0;
  unsigned long long* d_dbg = nullptr;
  unsigned long long* d_digest = nullptr;  // khr_map_digest accumulators
  uint32_t* d_wg_stats = nullptr;
  bool fold_pending = false;  // k_fuse's item records: folded by the next k_tracking_select instead of k_fuse_fold
  int stream_priority = 0;  // +1 the active window's streams (highest), -1 an object mini-map's (lowest), 0 default (env KHR_STREAM_PRIORITY=0)
  unsigned char* d_fuse_sink = nullptr;  // k_fuse: one 256-byte sink line per wave (kUpdateStatSlots workgroups x 16 waves)
  DevBuf<uint32_t> d_pix_scratch;  // khr_pixel_iou: mask image + counters (allocated on first use)
  DevBuf<uint8_t> d_inst;          // khr_forward_instances: per-id accumulators
  uint4* d_work4 = nullptr;       // update list of k_fuse: two descriptor arrays of item_cap entries (FuseList)
  uint4* d_tick_work4 = nullptr;  // tick path: two arrays per camera
  // tick path, one-launch form (tickUnion): the cameras' arguments on the device, one byte per wave item (camera bits)
  FuseFrame* d_tick_frames = nullptr;
  uint32_t* d_tick_mask = nullptr;
  bool tick_mask_dirty = false;
  uint32_t item_cap = 0;          // max_blocks x wave items per block
  // snapshots of the updated blocks (khr_snapshot_updated): arenas of released snapshots are reused
  struct SnapArena {
    DevBuf<uint8_t> buf;        // the packed blocks
    PinnedBuf<uint32_t> count;  // {blocks found, ticket}, written by the pack kernel through the device view
    volatile uint32_t* h_count() const { return count.get(); }
    int alloc(size_t bytes) {
      if (buf.alloc(bytes)) return fail(KHR_ENOMEM, "snapshot arena of %zu bytes", bytes);
      if (count.alloc(16)) {
        buf.reset();
        return fail(KHR_ENOMEM, "snapshot pinned words");
      }
      count[0] = count[1] = 0;
      return KHR_OK;
    }
  };
  // shared with the snapshots handed out: an output may outlive its ActiveWindow in the consumer's queue, so a release
  // after khr_destroy must still be safe (it then frees the arena instead of pooling it)
  struct SnapPool {
    std::mutex mu;
    std::vector<SnapArena> free;
    bool dead = false;
  };
  std::shared_ptr<SnapPool> snap_pool = std::make_shared<SnapPool>();
  // khr_frame_copy: device blocks of 16 bytes per pixel, pooled like the snapshot arenas (a copy may outlive the context)
  struct FramePool {
    std::mutex mu;
    std::vector<DevBuf<uint8_t>> free;
    bool dead = false;
  };
  std::shared_ptr<FramePool> frame_pool = std::make_shared<FramePool>();
  khr_snapshot* pending_snapshot = nullptr;  // taken inside khr_process_frame(KHR_PF_SNAPSHOT)
  Event ev_snap_fork, ev_snap_join;
  Event ev_mc_fork, ev_mc_join;
  // upper bound of the blocks an explicitly allocated map holds (khr_allocate_blocks since the last khr_reset_map; 0 =
  // unknown): the update kernel of an `allocate = false` integration (object mini-maps) sizes its persistent grid from it
  // instead of filling the chip with workgroups that find no item
  uint64_t explicit_blocks = 0;
  // integrateUpdateMulti: the items by frame count (k_multi_order): two arrays of item_cap descriptors, one uint4 of class counters,
  // one uint4 whose first word counts the untouched items, and those items' item_cap descriptors (the pruning launch's tail)
  DevBuf<uint4> d_multi_list;
  uint64_t box_gen = 0;             // map_gen as khr_begin_object_map left it: while equal,
  bool box_listed = false;          // ... the next integration's per-call reset is done and the live blocks are listed (k_setup_box),
  bool multi_counts_zeroed = false; // ... k_multi_order's counters are zero
  bool pruned_zeroed = false;       // ... and so is S_PRUNED
  DevBuf<uint32_t> d_frame_bits;    // integrateUpdateMulti: k_multi_cull's (item, frame) bits
  PinnedBuf<FuseFrame> h_frames;    // integrateUpdateMulti: per-frame arguments, pinned staging + device array
  DevBuf<FuseFrame> d_frames;
  Event ev_frames;
  uint32_t snap_ticket = 0;
  uint32_t wpb = 0;               // wave items per block of this context's k_fuse instantiation
  int fuse_zsplit = 2;            // z ranges per x-y patch of that instantiation
  // remote halo (multi-GPU): records gathered from the other ranks + their index
  DevBuf<uint64_t> d_halo_recs;
  const uint64_t* halo_view = nullptr;  // view, records in use: d_halo_recs, or the caller's device buffer (imported in place)
  DevBuf<uint64_t> d_halo_keys;
  DevBuf<uint32_t> d_halo_vals;
  uint32_t halo_cap_total = 0, halo_mask = 0, halo_n = 0;
  // remote mesh halo (three low voxel planes of blocks owned by other ranks)
  DevBuf<uint32_t> d_mh_recs;
  const uint32_t* mh_view = nullptr;  // view, the imported mesh halo records: d_mh_recs, or the caller's buffer (on_device = 2)
  DevBuf<uint64_t> d_mh_keys;
  DevBuf<uint32_t> d_mh_vals;
  uint32_t mh_cap_total = 0, mh_mask = 0, mh_n = 0;
  uint8_t* d_mh_flag = nullptr;
  // compact mesh halo (khr_mesh_halo_requests_sorted / _answer / _adopt)
  DevBuf<uint32_t> d_mh2_scratch;  // cnt | base | cursor (8 * kMeshHaloMaxWorld each) | total
  DevBuf<uint64_t> d_mh2_keys;
  DevBuf<uint32_t> d_mh2_offs;
  uint32_t mh2_ht = 0;
  bool mh_compact = false;
  PinnedBuf<uint32_t> h_pinned;  // [0] seed pixels of the last motion pass, [1] removed count, [2] count / [3] ticket written by
                                 // k_motion_pixels (zero-copy)
  uint32_t seed_ticket = 0;
  bool seed_publish_pending = false;
  bool seed_by_ticket = false;   // motionFinish waits for the ticket (k_motion_pixels) instead of ev_seed (key import)
  bool begun = false;            // the frame's ingest kernel did k_begin_integrate's work (khr_process_frame, main-stream ingest)
  uint32_t fetch_ticket = 0;                     // khr_fetch_mesh: completion ticket the gather kernel publishes
  bool fetch_pending = false;                    // khr_fetch_mesh_launch issued, khr_fetch_mesh outstanding
  uint32_t* d_fetch_done = nullptr;              //   + its workgroup completion counter (device)
  std::vector<uint32_t> fm_order;                // khr_fetch_mesh: slots that carry vertices, in sorted block order
  size_t fm_total = 0;
  uint64_t map_gen = 1, counters_gen = 0;        // block set generation / generation h_counters was read at (mesh download)
  int last_frame_slot = -1;                      // khr_process_frame: slot of the frame queued last
  // pinned host staging (downloads, block-index uploads): grow-only; one transfer batch in flight per buffer
  PinnedBuf<void> h_stage;
  PinnedBuf<uint32_t> h_totals;  // refreshMeshTotals' own pinned words
  PinnedBuf<void> h_up;                          // upload staging (khr_allocate_blocks: page-locked, read by the kernel in place)
  Event ev_ingest;                               // khr_process_frame: this frame's main-stream ingest is queued
  Event ev_up;                                   // the last upload out of h_up has been consumed
  // frames handed over with khr_ingest_ahead[_host], oldest first, waiting for their khr_process_frame calls.  Up to kMaxAhead: a
  // frontend that hands frame i + 1 over BEFORE it calls khr_process_frame for frame i keeps the copy engine busy across the
  // host's wait inside that call (round 5: with one entry the host-to-device copy of a 720p frame, ~205 us, started only after
  // the call had returned and the main stream idled behind it -- rocprofv3 timeline)
  struct AheadEntry { int slot; int ev; bool host; };
  std::vector<AheadEntry> ahead_q;
  Event ev_ahead[2];      // conversion of the entry finished (auxiliary stream)
  Event ev_ahead_h2d[2];  // host planes of the entry have arrived (host-to-device stream)
  int ahead_ev_next = 0;
  Event ev_h2d;                    // the pinned copy's own event (h2d_stream)
  bool h2d_pending = false;    // a copy out of caller memory is queued: the caller's buffers are released by the next call / khr_sync
  uint64_t h2d_bytes = 0;      // bytes queued through the pinned path (statistics)
  int ef_parity = 0, ef_cur = 0;  // which of C_N_EF / C_N_EF2 the next / the latest tracking pass fills
  Event ev_seed;
  uint32_t last_removed = 0;
  khr_ctx* dep_src = nullptr;     // view, khr_depend_on: this context's stream already waits for that context's earlier work
  Event ev_dep, ev_dep_aux;
  uint64_t last_track_stamp = 0;  // stamp of the latest tracking pass = last_occupied of every VOX_OCC voxel
  bool removed_pending = false;
  int4* d_removed = nullptr;
  // khr_process_frame(KHR_PF_OUTPUT): the list of the blocks about to be archived, published early (k_removed_publish)
  PinnedBuf<int4> h_removed_early;       // page-locked, max_blocks entries
  uint32_t* d_removed_early_n = nullptr; // [0] count, [1] workgroups done
  uint32_t removed_early_ticket = 0;     // h_pinned[11] (count in h_pinned[10]); 0 = the last archival has no early list
  bool removed_early = false;
  int* d_idx_staging = nullptr;
  // motion detection scratch
  uint64_t* d_keys = nullptr;
  uint32_t* d_pix = nullptr;
  void* d_cub_temp = nullptr;
  // motion detector voxel tables (seed table followed by boundary table) and compact lists
  uint64_t* d_md_keys = nullptr;
  uint32_t *d_md_counts = nullptr, *d_md_ids = nullptr, *d_md_adj = nullptr;
  uint32_t* d_md_n = nullptr;  // view: the first words of the head block {S, B, R, 0} + component records (owned by allocs)
  uint64_t *d_md_seed_keys = nullptr, *d_md_bnd_keys = nullptr;
  uint32_t *d_md_seed_counts = nullptr, *d_md_bnd_counts = nullptr;
  int32_t *d_md_seed_final = nullptr, *d_md_bnd_final = nullptr;
  int32_t* d_md_bnd_deg = nullptr;       // per boundary voxel: seeds of kept clusters that list it (k_md_comp_finals / the host walk)
  unsigned long long* d_md_bnd_mask = nullptr;  // per boundary voxel: bit set of the components that list it (k_md_bnd_comps; <= 64 components)
  // watchdog of the per-frame seed-count wait (khr_stats.n_seed_waits ...)
  uint64_t n_seed_waits = 0, n_seed_waits_late = 0, seed_wait_max_us = 0, seed_wait_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t seed_wait_late_us = 0, seed_wait_late_frame = 0, seed_wait_late_state = 0;
  bool last_ingest_on_aux = false;
  uint64_t n_md_device_merges = 0, n_md_host_walks = 0;  // seed frames whose clusters were merged from the device's overlap rows / walked on the host
  ClusterAcc* d_md_acc = nullptr;  // [256], index = cluster id
  // device components of the seed graph: head = {S, B, R, 0} followed by the component records
  uint32_t *d_md_parent = nullptr, *d_md_rootidx = nullptr;
  CompAcc* d_md_comp_acc = nullptr;
  int32_t* d_md_comp_final = nullptr;
  PinnedBuf<uint8_t> h_md_head;  // pinned mirror of the head + records, then the final ids going back
  bool md_host_walk = false;     // KHR_MD_HOST_WALK=1: always cluster on the host (A/B switch, results identical)
  uint32_t md_lds_max = kCompLds;  // KHR_MD_LDS_MAX=n: seed count up to which the single-workgroup LDS labelling is used
  uint32_t md_mask = 0, md_list_cap = 0;
  uint32_t md_head_ticket = 0;      // h_pinned[8]
  bool md_seed_run = false;         // the frame detected last had motion seeds: the next frame's chain is queued ahead of its seed count
  uint32_t md_prev_seed_px = 0;     // ... sized from that frame's seed pixels
  uint64_t n_md_prelaunched = 0, n_md_prelaunch_repeats = 0;
  uint32_t md_last_seeds = 0;       // seed voxels of the previous seed frame (predicts which component path is needed)
  uint32_t* d_md_edges = nullptr;     // seed-seed edge list of the latest seed frame (k_md_adjacency -> k_md_comp_lds)
  uint32_t* d_md_scratch4 = nullptr;  // 4 words k_publish may zero
  PinnedBuf<uint32_t> h_md_walk;     // page-locked block the host walk's lists and final ids travel through (kernels read / write it: no copy engine)
  Event ev_md_walk_up;               // the last upload out of it has been consumed
  PinnedBuf<ClusterAcc> h_md_acc_pinned;   // summaries of the latest seed frame (k_publish_cluster_acc), ticket h_pinned[7]
  uint32_t md_acc_ticket = 0;
  int md_acc_slot = -1;                    // the frame slot the published summaries belong to
  size_t cub_temp_bytes = 0;
  // object detector / cluster voxel sets (khr_kernels_objects.h); allocated on first use
  bool obj_configured = false;
  khr_object_detector_config obj_cfg{};
  std::vector<int32_t> obj_labels;  // sorted, unique
  DevBuf<int32_t> d_obj_labels;     // (replaced whenever the detector is configured again)
  uint64_t* d_gv_keys = nullptr;
  uint32_t gv_mask = 0;
  uint32_t *d_gv_parent = nullptr, *d_gv_rootidx = nullptr, *d_gv_node = nullptr;
  // views into ONE head block of allocs: the detector's counters, its records, and the voxel-set requests' counters / keys
  uint32_t* d_gv_n = nullptr;
  ObjAcc* d_obj_acc = nullptr;
  int32_t* d_obj_final = nullptr;
  uint64_t* d_cv_list = nullptr;
  uint32_t obj_root_cap = 0;
  uint32_t* d_gv_owners = nullptr;  // table slots claimed by the current request (work list + table reset)
  uint32_t* d_gv_done = nullptr;    // completion counter of k_gv_release_publish
  bool gv_clean = false;            // the (group, voxel) table is empty (every request gives it back empty)
  bool gv_counters_clean[4] = {false, false, false, false};  // request counters zeroed by their last k_publish: detect, voxel result sets 0 / 1 / 2
  PinnedBuf<uint8_t> h_obj_head;   // pinned: {roots, flags, -, -} + the cluster records (first download kObjHead of them)
  Event ev_obj;
  int obj_pending_slot = -1;       // objectsLaunch issued, objectsFinish outstanding
  // asynchronous per-cluster voxel sets, one request per id image (0 dynamic, 1 object).  Three result sets: set 0 belongs to the
  // dynamic image; the object image's requests use sets 1 and 2 in turn -- the set cv_set_obj is the one khr_cluster_voxels_fetch(1)
  // reads, the other one takes the voxel sets that objectsFinish queues ahead of the request (khr_configure_object_voxel_sets)
  // while the previous frame's may still be waiting for their fetch
  uint32_t* d_cv_n[3] = {nullptr, nullptr, nullptr};    // views (see d_gv_n)
  uint64_t* d_cv_keys[3] = {nullptr, nullptr, nullptr};
  PinnedBuf<uint8_t> h_cv[3];  // pinned: {count, flags, -, -} + keys
  Event ev_cv[3];
  int cv_pending_slot[2] = {-1, -1};
  uint32_t obj_ticket = 0, cv_ticket[3] = {0, 0, 0};  // h_pinned[4] / [5], [6], [12]
  int3 cv_origin[3]{};
  int cv_set_obj = 1;
  float obj_cv_size = 0.f;   // khr_configure_object_voxel_sets: the tracker's voxel size (0 = off)
  int obj_cv_slot = -1;      // objectsFinish queued the slot's voxel sets at obj_cv_size into the set 3 - cv_set_obj (-1 = nothing queued)
  // mesh
  MeshBuffers mesh[2]{};
  int mesh_cur = 0;
  uint32_t *d_mesh_count = nullptr, *d_mesh_offset = nullptr;
  uint8_t* d_regen = nullptr;
  uint32_t* d_mesh_old_off = nullptr;  // k_mesh_prepare's snapshot of mesh_desc[].offset (read by the copy of the kept meshes)
  uint32_t* d_mesh_nwork = nullptr;
  // generateMesh's work-list counter: words 0 and 4 of d_mesh_nwork alternate, each pass zeroes the other one (k_mesh_prepare), so no
  // memset is queued; mesh_nwork_last is the word of the latest pass (refreshMeshTotals)
  int mesh_nwork_par = 0, mesh_nwork_last = 0;
  bool mesh_made = false;  // a mesh was generated since the map was last emptied (only then can blocks keep vertices of an earlier pass)
  uint64_t mesh_total = 0;
  bool mesh_stale = false;
  // host mirrors
  std::vector<uint32_t> h_counters;
  khr_stats stats{};
  bool host_index_valid = false;
  std::map<std::array<int32_t, 3>, uint32_t> host_index;
  std::vector<uint32_t> host_flags;
  // map slices (khr_map_slice): sort keys (nextpow2(capacity) words) + count, created at the first slice; the SoA staging and its
  // page-locked mirror (same layout, count word in front) grow on demand; slice_hint = blocks the next call copies up front
  DevBuf<uint64_t> d_slice_keys;
  DevBuf<uint32_t> d_slice_count;
  DevBuf<uint8_t> d_slice_stage;
  PinnedBuf<uint8_t> h_slice_stage;
  uint32_t slice_cap = 0, slice_hint = 0;
  // rendered views (khr_render_view): the counters (created when a caller first asks for them) and the image staging of the host
  // form (created at the first host-form call, grown to the largest image)
  DevBuf<unsigned long long> d_render_stats;
  DevBuf<uint8_t> d_render_stage;
  PinnedBuf<uint8_t> h_render_stage;  // page-locked mirror of d_render_stage
  // point queries (khr_query_points): the same pair for its counters and the point / output staging of the host form
  DevBuf<unsigned long long> d_query_stats;
  DevBuf<uint8_t> d_query_stage;
  PinnedBuf<uint8_t> h_query_stage;  // page-locked mirror of d_query_stage
  // distance fields (khr_distance_field): the two int32 work grids (grown to the largest box), the counters, and the output
  // staging of the host form with its page-locked mirror
  DevBuf<int32_t> d_df_outer, d_df_inner;
  DevBuf<unsigned long long> d_df_stats;
  DevBuf<uint8_t> d_df_stage;
  PinnedBuf<uint8_t> h_df_stage;
  // registration (khr_align_linearize): the accumulator (its words 128 bytes apart) with its page-locked mirror, and the source /
  // weight staging of the host form
  DevBuf<unsigned long long> d_align_acc;
  PinnedBuf<unsigned long long> h_align_acc;
  DevBuf<uint8_t> d_align_stage;
  PinnedBuf<uint8_t> h_align_stage;  // page-locked mirror of d_align_stage
  // map checkpoints (khr_checkpoint_save / _load): two chunk staging areas of kCkptStageBytes each (created at the first call; their
  // page-locked mirrors only when a caller passes pageable memory), the chunk's slot list, the load's error word, and per
  // staging area one event for "filled" and one for "drained"
  DevBuf<uint8_t> d_ckpt[2];
  PinnedBuf<uint8_t> h_ckpt[2];
  DevBuf<uint32_t> d_ckpt_slots[2];
  DevBuf<uint32_t> d_ckpt_err;
  Event ev_ckpt_filled[2], ev_ckpt_drained[2];
  // welded mesh (khr_weld_mesh): the work area (block bases, per-vertex words, the cell table), the scans' temporary storage and
  // the result, each grown to the largest mesh so far; the counts come back through a page-locked block of their own
  DevBuf<uint8_t> d_weld_work, d_weld_cub, d_weld_out;
  PinnedBuf<uint32_t> h_weld;
  WeldOut weld_out{};       // views into d_weld_out
  khr_weld_stats weld_stats{};
  bool weld_valid = false;  // a weld succeeded and nothing has discarded its result
  // map merges (khr_merge_map, this context as the destination): the candidate set, the candidate list, its per-candidate words
  // (slot, hit, touched list), each grown to the largest merge so far; the counters with their page-locked mirror; the event that
  // orders this context's stream behind the source's
  DevBuf<uint64_t> d_merge_set;
  DevBuf<int4> d_merge_cand;
  DevBuf<uint32_t> d_merge_words;
  DevBuf<uint32_t> d_merge_ctr;
  PinnedBuf<uint32_t> h_merge;
  Event ev_merge;
  // map diffs (khr_diff_map, this context as `now`; the candidates and counters use the merge scratch above): the sorted changed
  // list with its scan, the sort's and the scan's temporary storage and the result, each grown to the largest diff so far
  DevBuf<uint8_t> d_diff_work, d_diff_cub, d_diff_out;
  khr_diff_stats diff_stats{};
  bool diff_valid = false;  // a diff succeeded and nothing has discarded its result
  // map segmentation (khr_segment_map; the sorted block list is d_slice_keys above): the scratch (tables, parents, counts, numbers,
  // counters), hipcub's temporary storage, the sort keys of the voxel list (twice) and the result, each grown to the largest call
  DevBuf<uint8_t> d_seg_work, d_seg_cub, d_seg_sort, d_seg_out;
  PinnedBuf<unsigned long long> h_seg;
  khr_segment_stats seg_stats{};
  bool seg_valid = false;   // a segmentation succeeded and nothing has discarded its result
  bool seg_listed = false;  // ... and it holds the voxel list
  // Voronoi fields (khr_voronoi_field; the seeds use d_df_outer above): the key grid, the dense outputs with the per-workgroup
  // list counts behind them, the scan's temporary storage, the list, the counters with their page-locked mirror, and the
  // page-locked staging of khr_voronoi_field_into's host form; each grown to the largest call
  DevBuf<uint64_t> d_vor_keys;
  DevBuf<uint8_t> d_vor_dense, d_vor_cub, d_vor_list;
  DevBuf<unsigned long long> d_vor_ctr;
  PinnedBuf<unsigned long long> h_vor;
  PinnedBuf<uint8_t> h_vor_stage;
  khr_voronoi_stats vor_stats{};
  BoxResult vor;            // the box of the last Voronoi field and its cell size (khr_places_graph and khr_travel_field read the field)
  float vor_cell_size = 0.f;
  // places graphs (khr_places_graph / khr_places_graph_from): the device copy of a host caller's field, the per-cell work arrays
  // with the dense place ids, the pair / edge / component work lists, the scan's and the sort's temporary storage, the result
  // lists, the counters with their page-locked mirror, and the page-locked staging of the host forms; each grown to the largest call
  DevBuf<uint8_t> d_pl_in, d_pl_dense, d_pl_work, d_pl_cub, d_pl_out;
  DevBuf<unsigned long long> d_pl_ctr;
  PinnedBuf<unsigned long long> h_pl;
  PinnedBuf<uint8_t> h_pl_stage;
  khr_places_stats pl_stats{};
  BoxResult pl;                  // the box of the last places graph (khr_places_graph_box)
  bool pl_from_voronoi = false;  // ... which was read from the Voronoi result
  // travel fields and paths (khr_travel_field / khr_travel_field_from / khr_travel_paths): the device copy of a host caller's field
  // and goals, the per-cell keys, masks, tile flags and result arrays, the counters with their page-locked mirror, the page-locked
  // staging of the host forms; the per-start arrays, the scan's temporary storage and the path cells; each grown to the largest call
  DevBuf<uint8_t> d_tf_in, d_tf_dense, d_tf_path, d_tf_cub, d_tf_cells;
  DevBuf<unsigned long long> d_tf_ctr;
  PinnedBuf<unsigned long long> h_tf;
  PinnedBuf<uint8_t> h_tf_stage;
  khr_travel_stats tf_stats{};
  BoxResult tf;                  // the box of the last travel field (khr_travel_field_box)
  bool tf_from_voronoi = false;  // ... which was read from the Voronoi result
  size_t tfp_starts = 0, tfp_total = 0;  // starts and path cells of the last khr_travel_paths
  bool tfp_valid = false;      // ... which succeeded, on the travel field that is still there
  // timing
  uint32_t timing = 0;  // bit i = timer i enabled
  std::vector<TimingRec> pending;
  std::vector<Event> event_pool;  // timing events that are free (created with timing; the ones in use sit in `pending`)
  double t_ms[kNumTimers] = {0};
  uint64_t t_n[kNumTimers] = {0};
};

namespace {

// a timing event: out of the pool of free ones, or a new one
Event takeEvent(khr_ctx* c) {
  Event e;
  if (!c->event_pool.empty()) {
    e = std::move(c->event_pool.back());
    c->event_pool.pop_back();
  } else {
    e.ensure(hipEventDefault);
  }
  return e;
}

struct ScopedTimer {
  khr_ctx* c;
  int which;
  Event a, b;
  hipStream_t st;  // the stream the bracketed launches go to
  bool on = false;
  ScopedTimer(khr_ctx* ctx, int w, hipStream_t stream = nullptr)  // (nullptr: the context's)
      : c(ctx), which(w), st(stream ? stream : static_cast<hipStream_t>(ctx->stream)) {
    on = w >= 0 && ((c->timing >> w) & 1u);
    if (on) {
      a = takeEvent(c);
      b = takeEvent(c);
      hipEventRecord(a, st);
    }
  }
  ~ScopedTimer() {
    if (on) {
      hipEventRecord(b, st);
      c->pending.push_back({which, std::move(a), std::move(b)});
    }
  }
};

// Single-kernel timers use the start / stop events of the dispatch packet itself (hipExtLaunchKernelGGL): the same
// begin / end timestamps rocprofv3 reports, and no extra barrier packets in the stream.  ScopedTimer (event records
// around a group of launches) costs ~5 us of stream time per bracket.
#define KHR_LAUNCH_TIMED_ON(which, strm, kernel, grid, block, ...)                                     \
  do {                                                                                                 \
    if ((c->timing >> (which)) & 1u) {                                                                 \
      Event ev_a = takeEvent(c), ev_b = takeEvent(c);                                                  \
      hipExtLaunchKernelGGL(kernel, grid, block, 0, strm, ev_a, ev_b, 0, __VA_ARGS__);                 \
      c->pending.push_back({(which), std::move(ev_a), std::move(ev_b)});                               \
    } else {                                                                                           \
      hipLaunchKernelGGL(kernel, grid, block, 0, strm, __VA_ARGS__);                                   \
    }                                                                                                  \
  } while (0)
#define KHR_LAUNCH_TIMED(which, kernel, grid, block, ...) KHR_LAUNCH_TIMED_ON(which, c->stream, kernel, grid, block, __VA_ARGS__)

void resolveTimers(khr_ctx* c) {
  for (auto& r : c->pending) {
    hipEventSynchronize(r.b);
    float ms = 0.f;
    hipEventElapsedTime(&ms, r.a, r.b);
    if (r.which >= 0) {  // (-1: a speculative launch whose device-side gate was closed)
      c->t_ms[r.which] += ms;
      c->t_n[r.which] += 1;
    }
    c->event_pool.push_back(std::move(r.a));
    c->event_pool.push_back(std::move(r.b));
  }
  c->pending.clear();
}

// temporary device buffer of the host-pointer variants of the exchange calls (tests / non-RCCL callers): freed on
// every exit path; hipFree waits for the device, so work still using the buffer is finished first
struct DevTemp : DevBuf<uint8_t> {
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(get()); }
};

// a buffer that lives as long as the context: owned by c->allocs, *out is a view of it
template <typename T>
int devAlloc(khr_ctx* c, T** out, size_t count, bool zero = true) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  DevBuf<uint8_t> b;
  if (int rc = b.alloc(bytes)) return rc;
  void* p = b.get();
  c->allocs.push_back(std::move(b));
  if (zero) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, c->stream);
    if (e != hipSuccess) return fail(KHR_EDEVICE, "hipMemset failed: %s", hipGetErrorString(e));
  }
  *out = static_cast<T*>(p);
  return KHR_OK;
}

void makePose(const double* T, float* R, float* t, float* Rw, float* tw) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rw[3 * r + c] = static_cast<float>(T[4 * r + c]);
    tw[r] = static_cast<float>(T[4 * r + 3]);
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = static_cast<float>(T[4 * c + r]);
    const double v = -(T[4 * 0 + r] * T[3] + T[4 * 1 + r] * T[7] + T[4 * 2 + r] * T[11]);
    t[r] = static_cast<float>(v);
  }
}

void crossn(const float* a, const float* b, float* o) {
  const float x = a[1] * b[2] - a[2] * b[1];
  const float y = a[2] * b[0] - a[0] * b[2];
  const float z = a[0] * b[1] - a[1] * b[0];
  const float n = std::sqrt((x * x + y * y) + z * z);
  o[0] = x / n;
  o[1] = y / n;
  o[2] = z / n;
}

DevFrame makeDevFrame(const khr_ctx* c, const FrameSlot& s) {
  DevFrame f{};
  f.depth = const_cast<float*>(s.vDepth());  // (kernels that take a DevFrame only read the planes; the ingest kernels get the slot's own arrays)
  f.range = const_cast<float*>(s.vRange());
  f.rgba = const_cast<uint32_t*>(s.vRgba());
  f.label = const_cast<int32_t*>(s.vLabel());
  f.dyn = s.dyn;
  f.obj = s.has_obj ? s.obj : nullptr;
  f.W = s.sensor.width;
  f.H = s.sensor.height;
  f.fx = s.sensor.fx;
  f.fy = s.sensor.fy;
  f.cx = s.sensor.cx;
  f.cy = s.sensor.cy;
  f.min_range = s.sensor.min_range;
  f.max_range = s.sensor.max_range;
  makePose(s.meta.world_T_sensor, f.R, f.t, f.Rw, f.tw);
  f.stamp = s.meta.timestamp_ns;
  f.has_color = s.has_color;
  f.has_label = s.has_label;
  (void)c;
  return f;
}

DevFrustum makeFrustum(const khr_ctx* c, const DevFrame& f) {
  DevFrustum fr{};
  const float xl = (0.f - f.cx) / f.fx, xr = (static_cast<float>(f.W) - f.cx) / f.fx;
  const float yt = (0.f - f.cy) / f.fy, yb = (static_cast<float>(f.H) - f.cy) / f.fy;
  const float tl[3] = {xl, yt, 1.f}, tr[3] = {xr, yt, 1.f}, bl[3] = {xl, yb, 1.f}, br[3] = {xr, yb, 1.f};
  crossn(bl, tl, fr.n[0]);
  crossn(tr, br, fr.n[1]);
  crossn(tl, tr, fr.n[2]);
  crossn(br, bl, fr.n[3]);
  fr.infl = 0.8660254f * c->p.bs;
  fr.n_steps = static_cast<int>(std::ceil(f.max_range * c->p.bs_inv)) + 1;
  fr.max_steps = static_cast<int>(std::floor((f.max_range + fr.infl) * c->p.bs_inv));  // (alloc_candidate = camera_offset; <= n_steps - 1)
  for (int a = 0; a < 3; ++a) fr.tw[a] = f.tw[a];
  fr.bc = make_int3(static_cast<int>(std::floor(f.tw[0] * c->p.bs_inv)),
                    static_cast<int>(std::floor(f.tw[1] * c->p.bs_inv)),
                    static_cast<int>(std::floor(f.tw[2] * c->p.bs_inv)));
  return fr;
}

// a device staging block and its page-locked mirror (the host forms of the map readers) grow together: both are released before
// either is allocated again, and a failure leaves both empty.  The caller has waited for whatever used the old pair.
int reserveStagePair(DevBuf<uint8_t>& d, PinnedBuf<uint8_t>& h, size_t bytes, const char* what) {
  if (bytes <= d.count() && bytes <= h.count()) return KHR_OK;
  d.reset();
  h.reset();
  if (d.alloc(bytes)) return fail(KHR_ENOMEM, "%s staging of %zu bytes", what, bytes);
  if (h.alloc(bytes)) {
    d.reset();
    return fail(KHR_ENOMEM, "page-locked %s staging of %zu bytes", what, bytes);
  }
  return KHR_OK;
}

// grow-only pinned staging; contents are undefined after a call that grows it
int ensureStage(khr_ctx* c, size_t bytes) {
  if (bytes <= c->h_stage.count()) return KHR_OK;
  return c->h_stage.reserve(std::max<size_t>(bytes + bytes / 2, 1u << 20));
}

int readCounters(khr_ctx* c) {
  c->h_counters.resize(C_COUNT);
  HIP_TRY(hipMemcpyAsync(c->h_counters.data(), c->m.counters, sizeof(uint32_t) * C_COUNT, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

int ensureHostIndex(khr_ctx* c) {
  if (c->host_index_valid) return KHR_OK;
  int rc = readCounters(c);
  if (rc) return rc;
  const uint32_t n = c->h_counters[C_MAX_SLOT];
  std::vector<int4> idx(n);
  c->host_flags.resize(n);
  if (n) {
    HIP_TRY(hipMemcpyAsync(idx.data(), c->m.blk_index, sizeof(int4) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->host_flags.data(), c->m.blk_flags, sizeof(uint32_t) * n, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  c->host_index.clear();
  for (uint32_t s = 0; s < n; ++s)
    if (c->host_flags[s] & BLK_LIVE) c->host_index[{idx[s].x, idx[s].y, idx[s].z}] = s;
  c->host_index_valid = true;
  return KHR_OK;
}

inline int gridFor(size_t n, int block = 256) { return static_cast<int>((n + block - 1) / block); }

template <typename F>
int dispatchVps(khr_ctx* c, F&& f) {
  if (c->cfg.voxels_per_side == 16) return f(std::integral_constant<int, 16>());
  if (c->cfg.voxels_per_side == 8) return f(std::integral_constant<int, 8>());
  return fail(KHR_EINVAL, "voxels_per_side must be 8 or 16");
}

constexpr int kUpdateWavesPerCu = 16;  // resident waves per CU the update kernel's persistent grid is sized for
constexpr int kUpdateWpw = 12;         // waves per workgroup of k_fuse
constexpr int kMultiChunk = 7;         // frames per launch of the object extractor's multi-frame update (integrateUpdateMulti)
constexpr int kMaxMultiFrames = 1024;
constexpr int kStreamGrid = 4096;

// exact (bit-for-bit) arithmetic in the update kernels unless the configuration asks for the relaxed form
inline bool exactArithmetic(const khr_ctx* c) { return c->cfg.relaxed_arithmetic == 0; }

// ---- what the box-field calls share on the host (khr_distance_field, khr_voronoi_field, khr_places_graph, khr_travel_field;
// khr_box_host.h holds the part without HIP) ---------------------------------------------------------------------------------

// checkCellBox as the calls report it (KHR_EINVAL; `cells` on success)
int checkBox(const char* who, const int32_t origin[3], const int32_t dims[3], int ratio, size_t* cells) {
  int a = -1;
  switch (checkCellBox(origin, dims, ratio, cells, &a)) {
    case BOX_BAD_DIM: return fail(KHR_EINVAL, "%s: dims[%d] = %d: 1 .. %d", who, a, dims[a], KHR_DF_MAX_DIM);
    case BOX_BAD_RANGE: return fail(KHR_EINVAL, "%s: the box leaves the index range on axis %d", who, a);
    case BOX_BAD_CELLS: return fail(KHR_EINVAL, "%s: %zu cells: at most 2^24", who, *cells);
    case BOX_OK: break;
  }
  return KHR_OK;
}

// K result arrays out of the context's buffers into the caller's: device-to-device in stream order, or through the feature's
// page-locked staging with one wait.  A growth of the staging waits first for whatever may still read the old block.
template <size_t K>
int copyOut(khr_ctx* c, PinnedBuf<uint8_t>& stage, int on_device, void* const (&dst)[K], const void* const (&src)[K], const size_t (&bytes)[K], const char* who) {
  if (on_device) {
    for (size_t k = 0; k < K; ++k)
      if (dst[k] && bytes[k]) HIP_TRY(hipMemcpyAsync(dst[k], src[k], bytes[k], hipMemcpyDeviceToDevice, c->stream));
    return KHR_OK;
  }
  Arena a;
  size_t off[K];
  for (size_t k = 0; k < K; ++k) off[k] = dst[k] ? a.take(bytes[k]) : 0;
  if (a.bytes() == 0) return KHR_OK;
  if (stage.count() < a.bytes()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stage.reserve(a.bytes())) return fail(KHR_ENOMEM, "%s: %zu bytes of page-locked staging", who, a.bytes());
  }
  for (size_t k = 0; k < K; ++k)
    if (dst[k] && bytes[k]) HIP_TRY(hipMemcpyAsync(stage + off[k], src[k], bytes[k], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < K; ++k)
    if (dst[k] && bytes[k]) std::memcpy(dst[k], stage + off[k], bytes[k]);
  return KHR_OK;
}

// a host array into device memory through page-locked staging (the caller has reserved both) ...
int copyIn(khr_ctx* c, uint8_t* d_in, uint8_t* stage, const void* src, size_t bytes) {
  std::memcpy(stage, src, bytes);
  HIP_TRY(hipMemcpyAsync(d_in, stage, bytes, hipMemcpyHostToDevice, c->stream));
  return KHR_OK;
}
// ... and K of them, each at byte at[k] of a device block and of its page-locked mirror
template <size_t K>
int copyIn(khr_ctx* c, uint8_t* d_in, uint8_t* stage, const void* const (&src)[K], const size_t (&bytes)[K], const size_t (&at)[K]) {
  for (size_t k = 0; k < K; ++k) KHR_TRY(copyIn(c, d_in + at[k], stage + at[k], src[k], bytes[k]));
  return KHR_OK;
}

// device words into page-locked memory, and the wait for them
int readWords(khr_ctx* c, const void* d_src, void* h_dst, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

}  // namespace

extern "C" {

// other translation units of the library (khr_rayver.hip) report through the same per-thread error text
extern "C" void khr_set_last_error(const char* text) { g_last_error = text ? text : ""; }

// ---- host timeline (diagnostic; KHR_HOST_TRACE=<file>) --------------------------------------------------------------
// Marks are (tag, monotonic ns) pairs appended by the thread that passes them; the file is written at process exit.
// Off (one predictable branch per mark) unless the variable is set.
namespace {
struct HostTrace {
  bool on = false;
  std::string path;
  std::mutex mu;
  std::vector<std::pair<const char*, uint64_t>> marks;
  HostTrace() {
    if (const char* e = std::getenv("KHR_HOST_TRACE")) {
      on = e[0] != 0;
      path = e;
      marks.reserve(1 << 20);
    }
  }
  ~HostTrace() {
    if (!on) return;
    if (FILE* f = std::fopen(path.c_str(), "w")) {
      for (const auto& m : marks) std::fprintf(f, "%s %llu\n", m.first, static_cast<unsigned long long>(m.second));
      std::fclose(f);
    }
  }
};
HostTrace g_trace;
}  // namespace
// tag must outlive the process (string literal / interned)
extern "C" void khr_host_trace(const char* tag) {
  if (!g_trace.on) return;
  const uint64_t t = static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                              std::chrono::steady_clock::now().time_since_epoch()).count());
  std::lock_guard<std::mutex> lk(g_trace.mu);
  g_trace.marks.emplace_back(tag, t);
}
#define HT(tag) khr_host_trace(tag)

const char* khr_last_error(void) { return g_last_error.c_str(); }

void khr_default_config(khr_config* cfg) {
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->voxel_size = 0.1f;
  cfg->voxels_per_side = 16;
  cfg->truncation_distance = 0.3f;
  cfg->with_semantics = 0;  // ActiveWindow::Config() : hydra::ActiveWindowModule::Config(false, true)
  cfg->with_tracking = 1;
  cfg->num_labels = 20;
  cfg->use_weight_dropoff = 1;
  cfg->weight_dropoff_epsilon = -1.0f;
  cfg->use_constant_weight = 0;
  cfg->max_weight = 1e5f;
  cfg->interpolation_method = 2;
  cfg->adaptive_max_range_difference = 0.2f;
  cfg->range_mode = 0;
  cfg->semantic_mode = 0;
  cfg->label_confidence = 0.9f;
  cfg->temporal_buffer = 1.f;
  cfg->tsdf_occupancy_threshold = -1.5f;
  cfg->neighbor_connectivity = 18;
  cfg->temporal_window = 3.f;
  cfg->md_neighbor_connectivity = 26;
  cfg->md_min_cluster_size = 0;
  cfg->md_max_cluster_size = 1000000;
  cfg->md_min_separation_distance = 1.0f;
  cfg->md_max_range = 10000.f;
  cfg->md_min_z_coordinate = -10000.f;
  cfg->mesh_min_weight = 1e-4f;
  cfg->max_blocks = 16384;
  cfg->max_frame_pixels = 1280 * 720;
  cfg->num_frame_slots = 2;
  cfg->max_mesh_vertices = 8u << 20;
  cfg->device = 0;
  cfg->rank = 0;
  cfg->world_size = 1;
  cfg->max_snapshot_blocks = 0;  // = min(max_blocks, 8192)
  cfg->alloc_candidate = 0;
  cfg->color_blend_weight = 0;
  cfg->mesh_attr_source = 0;
  cfg->mesh_degenerate_eps = 0.f;  // = 1e-6
  cfg->relaxed_arithmetic = 0;  // bit-exact values: 2 % slower update kernel than the relaxed mode (measured), so it is the default
}

// the voxel-size dependent part of DevParams (khr_create, khr_reset_map)
static void deriveMetricParams(const khr_config& cfg, DevParams& p) {
  p.vs = cfg.voxel_size;
  p.vs_inv = 1.f / cfg.voxel_size;
  p.bs = cfg.voxel_size * static_cast<float>(cfg.voxels_per_side);
  p.bs_inv = 1.f / p.bs;
  p.trunc = cfg.truncation_distance;
  p.dropoff_eps = cfg.weight_dropoff_epsilon > 0.f ? cfg.weight_dropoff_epsilon : cfg.weight_dropoff_epsilon * -cfg.voxel_size;
  p.occ_thr = cfg.tsdf_occupancy_threshold < 0 ? cfg.tsdf_occupancy_threshold * -cfg.voxel_size : cfg.tsdf_occupancy_threshold;
}

int khr_retain_slot(khr_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= static_cast<int>(c->slots.size())) return fail(KHR_EINVAL, "bad slot");
  c->slot_leases[slot].fetch_add(1, std::memory_order_acq_rel);
  return KHR_OK;
}

// contexts that exist: a slot lease may be dropped after its context is gone (an output that carries a copy of the frame's
// InputData can sit in the consumer's queue longer than the ActiveWindow lives); that release must be a no-op, not a
// use-after-free
static std::mutex g_live_mu;
static std::vector<khr_ctx*> g_live_ctx;
// Streams of a context by role.  HIP multiplexes a process's streams onto a handful of hardware queues (4 by default), per priority
// level: with the window's main / auxiliary / mesh / snapshot / copy streams and the extraction workers' streams all at the default
// priority, a frame's ingest on the auxiliary stream could sit in the same hardware queue behind an object extraction's 1 - 2 ms
// kernel chain -- the "one run in ten" late seed count (profiles/r06_seed_latency.txt, state 0xa: main stream idle, auxiliary busy).
// The active window's streams (16^3 blocks) are created at the highest priority, the object mini-maps' (8^3) at the lowest: different
// priority levels never share a hardware queue, and the dispatcher prefers the window's workgroups when both have some ready.
static int createStream(khr_ctx* c, Stream& out) {
  int lo = 0, hi = 0;  // (numerically: greatest = lowest priority)
  if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess || lo == hi || c->stream_priority == 0)
    return out.create(hipStreamNonBlocking);
  const int prio = c->stream_priority > 0 ? hi : lo;
  return out.create(hipStreamNonBlocking, &prio);
}

static bool ctxIsLive(khr_ctx* c) {
  std::lock_guard<std::mutex> lock(g_live_mu);
  return std::find(g_live_ctx.begin(), g_live_ctx.end(), c) != g_live_ctx.end();
}

int khr_release_slot(khr_ctx* c, int slot) {
  if (!c) return fail(KHR_EINVAL, "bad slot");
  // the registry lock is held across the dereference: khr_destroy takes the context off the registry under the
  // same lock before it frees it, so a release that has seen the context alive finishes before the ring goes away
  std::lock_guard<std::mutex> live_lock(g_live_mu);
  if (std::find(g_live_ctx.begin(), g_live_ctx.end(), c) == g_live_ctx.end())
    return KHR_OK;  // the context (and with it the frame ring) is gone: nothing to give back
  if (slot < 0 || slot >= static_cast<int>(c->slots.size())) return fail(KHR_EINVAL, "bad slot");
  // decrement only while positive (leases are taken and dropped by the frame thread and by detached extraction workers:
  // an unmatched release must not erase a lease somebody else takes at the same moment)
  int cur = c->slot_leases[slot].load(std::memory_order_acquire);
  while (cur > 0)
    if (c->slot_leases[slot].compare_exchange_weak(cur, cur - 1, std::memory_order_acq_rel, std::memory_order_acquire)) return KHR_OK;
  return fail(KHR_ESTATE, "slot %d was not retained", slot);
}

int khr_depend_on(khr_ctx* c, khr_ctx* other) {
  if (!c || !other) return fail(KHR_EINVAL, "null ctx");
  if (c->device != other->device) return fail(KHR_EINVAL, "contexts live on different devices");
  HIP_TRY(hipSetDevice(c->device));
  // (events owned by the DEPENDENT context: khr_depend_on may be called from a worker thread while the other context's
  // own thread keeps using its events)
  KHR_TRY(c->ev_dep_aux.ensure());
  if (c->stream == other->stream) {
    HIP_TRY(hipEventRecord(c->ev_dep_aux, other->aux_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_dep_aux, 0));
    c->dep_src = other;
    return KHR_OK;
  }
  KHR_TRY(c->ev_dep.ensure());
  HIP_TRY(hipEventRecord(c->ev_dep, other->stream));
  HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_dep, 0));
  // ... and behind its object detector (the object images of its frame slots)
  HIP_TRY(hipEventRecord(c->ev_dep_aux, other->aux_stream));
  HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_dep_aux, 0));
  c->dep_src = other;
  return KHR_OK;
}

// the reset itself (khr_reset_map, khr_begin_object_map): the launch and the host-side state that goes with the map's contents
static int resetMap(khr_ctx* c, float voxel_size, float truncation_distance) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!(voxel_size > 0.f) || !(truncation_distance > 0.f)) return fail(KHR_EINVAL, "voxel_size / truncation_distance must be > 0");
  HIP_TRY(hipSetDevice(c->device));
  c->cfg.voxel_size = voxel_size;
  c->cfg.truncation_distance = truncation_distance;
  deriveMetricParams(c->cfg, c->p);
  const size_t n = std::max<size_t>(static_cast<size_t>(c->m.ht_mask) + 1, c->m.capacity);
  hipLaunchKernelGGL(k_reset_map, dim3(gridFor(n)), dim3(256), 0, c->stream, c->m, c->d_wg_stats);
  HIP_TRY(hipGetLastError());
  c->mesh_cur = 0;
  c->mesh_total = 0;
  c->mesh_stale = false;
  c->mesh_made = false;
  c->weld_valid = false;
  c->diff_valid = false;
  c->seg_valid = false;
  c->vor.valid = false;
  c->pl.valid = false;
  c->tf.valid = c->tfp_valid = false;
  c->host_index_valid = false, ++c->map_gen;
  c->explicit_blocks = 0;
  c->box_listed = false;
  c->last_removed = 0;
  c->removed_pending = false;
  c->last_track_stamp = 0;
  c->dep_src = nullptr;
  c->halo_n = 0;
  c->mh_n = 0;
  c->stats = khr_stats{};
  for (auto& s : c->slots) {
    s.valid = false;
    s.clusters.clear();
    s.sem_clusters.clear();
  }
  for (size_t i = 0; i < c->slots.size(); ++i) c->slot_leases[i].store(0);
  return KHR_OK;
}

int khr_reset_map(khr_ctx* c, float voxel_size, float truncation_distance) { return resetMap(c, voxel_size, truncation_distance); }

int khr_get_config(khr_ctx* c, khr_config* out) {
  if (!c || !out) return fail(KHR_EINVAL, "null argument");
  *out = c->cfg;
  return KHR_OK;
}

int khr_create(const khr_config* cfg, khr_ctx** out) {
  if (!cfg || !out) return fail(KHR_EINVAL, "null argument");
  *out = nullptr;
  // config validation (reference: config::checkValid, tracking_integrator.cpp:61-65,
  // free_space_motion_detector.cpp:63-67)
  if (!(cfg->voxel_size > 0.f) || !(cfg->truncation_distance > 0.f)) return fail(KHR_EINVAL, "voxel_size / truncation_distance must be > 0");
  if (cfg->voxels_per_side != 16 && cfg->voxels_per_side != 8) return fail(KHR_EINVAL, "voxels_per_side must be 8 or 16");
  auto conn_ok = [](int c) { return c == 6 || c == 18 || c == 26; };
  if (!conn_ok(cfg->neighbor_connectivity) || !conn_ok(cfg->md_neighbor_connectivity)) return fail(KHR_EINVAL, "neighbor_connectivity must be one of {6, 18, 26}");
  if (!(cfg->temporal_buffer > 0.f) || !(cfg->temporal_window > 0.f)) return fail(KHR_EINVAL, "temporal_buffer / temporal_window must be > 0");
  if (cfg->tsdf_occupancy_threshold == 0.f) return fail(KHR_EINVAL, "tsdf_occupancy_threshold must be != 0");
  if (cfg->md_max_cluster_size < cfg->md_min_cluster_size) return fail(KHR_EINVAL, "param 'max_cluster_size' must be >= 'min_cluster_size'");
  if (!(cfg->md_max_range > 0.f)) return fail(KHR_EINVAL, "md_max_range must be > 0");
  if (cfg->with_semantics && cfg->num_labels < 1) return fail(KHR_EINVAL, "num_labels must be >= 1 with semantics");
  if (cfg->semantic_mode == 1 && cfg->with_semantics && cfg->num_labels != 2) return fail(KHR_EINVAL, "binary semantic integrator needs num_labels == 2");
  if (cfg->max_blocks < 1 || cfg->max_frame_pixels < 1 || cfg->num_frame_slots < 1) return fail(KHR_EINVAL, "capacities must be >= 1");
  if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return fail(KHR_EINVAL, "bad rank / world_size");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(KHR_EDEVICE, "no HIP device available: the khronos_amd fusion path has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(KHR_EINVAL, "device %d out of range (%d devices)", cfg->device, ndev);
  HIP_TRY(hipSetDevice(cfg->device));

  // (every failure below leaves through this owner, i.e. through khr_destroy: the one teardown path)
  std::unique_ptr<khr_ctx, void (*)(khr_ctx*)> owner(new khr_ctx(), khr_destroy);
  khr_ctx* c = owner.get();
  c->cfg = *cfg;
  c->device = cfg->device;
  {
    static const bool prio_off = std::getenv("KHR_STREAM_PRIORITY") && std::atoi(std::getenv("KHR_STREAM_PRIORITY")) == 0;
    static const int prio_window = std::getenv("KHR_WINDOW_PRIORITY") ? std::atoi(std::getenv("KHR_WINDOW_PRIORITY")) : 0;
    c->stream_priority = prio_off ? 0 : (cfg->voxels_per_side == 8 ? -1 : prio_window);
  }
  if (createStream(c, c->stream)) return fail(KHR_EDEVICE, "hipStreamCreate failed");
  if (createStream(c, c->aux_stream) || c->ev_aux.ensure() || c->ev_aux_done.ensure())
    return fail(KHR_EDEVICE, "auxiliary stream / event creation failed");
  if (c->h_pinned.alloc(16) || c->ev_seed.ensure()) return fail(KHR_EDEVICE, "pinned scratch / event creation failed");
  std::memset(c->h_pinned, 0, 64);
  // staging buffers up front: growing them later means hipHostMalloc / hipMalloc in the middle of a run (hundreds of us,
  // and hipMalloc stalls every stream of the device)
  // (object mini-maps take their whole block list through it, khr_allocate_blocks per extraction: sized for a full pool -- round 5:
  // an extraction whose list outgrew the 64 KB grew it from its worker thread, and the hipMalloc waited 5 - 11 ms for the window's
  // frames to leave the device idle, profiles/r05_host_input_marks.txt)
  if (ensureStage(c, 1u << 20) != KHR_OK ||
      c->h_up.alloc(std::max<size_t>(1u << 16, cfg->voxels_per_side == 8 ? sizeof(int32_t) * 3 * static_cast<size_t>(cfg->max_blocks) : 0)))
    return fail(KHR_ENOMEM, "pinned staging buffers");

  DevParams& p = c->p;
  deriveMetricParams(*cfg, p);
  p.vps = cfg->voxels_per_side;
  p.nvox = p.vps * p.vps * p.vps;
  p.K = cfg->with_semantics ? cfg->num_labels : 1;
  p.KS = cfg->packed_likelihood_rows ? p.K : likStride(p.K);
  p.with_semantics = cfg->with_semantics;
  p.with_tracking = cfg->with_tracking;
  p.use_dropoff = cfg->use_weight_dropoff;
  p.const_weight = cfg->use_constant_weight;
  p.interp = cfg->interpolation_method;
  p.range_mode = cfg->range_mode;
  p.sem_mode = cfg->semantic_mode;
  p.max_weight = cfg->max_weight;
  p.adaptive_diff = cfg->adaptive_max_range_difference;
  p.log_match = std::log(cfg->label_confidence);
  p.log_nomatch = cfg->num_labels > 1 ? std::log((1.f - cfg->label_confidence) / static_cast<float>(cfg->num_labels - 1)) : 0.f;
  p.temporal_buffer = static_cast<double>(cfg->temporal_buffer);
  p.temporal_window = static_cast<double>(cfg->temporal_window);
  p.nn = cfg->neighbor_connectivity;
  p.mesh_min_weight = cfg->mesh_min_weight;
  p.mesh_eps = cfg->mesh_degenerate_eps > 0.f ? cfg->mesh_degenerate_eps : 1e-6f;
  p.mesh_attr_source = cfg->mesh_attr_source;
  p.alloc_candidate = cfg->alloc_candidate;
  p.rank = cfg->rank;
  p.world = cfg->world_size;
  p.dbg = std::getenv("KHR_DEBUG") ? std::atoi(std::getenv("KHR_DEBUG")) : 0;

  DevMap& m = c->m;
  const size_t cap = cfg->max_blocks, nv = p.nvox;
  uint32_t ht = 1;
  while (ht < cap * 4) ht <<= 1;
  m.ht_mask = ht - 1;
  m.capacity = static_cast<uint32_t>(cap);
  int rc = KHR_OK;
  KHR_CHAIN(devAlloc(c, &m.ht_keys, ht, false));
  KHR_CHAIN(devAlloc(c, &m.ht_vals, ht));
  KHR_CHAIN(devAlloc(c, &m.blk_index, cap));
  KHR_CHAIN(devAlloc(c, &m.blk_flags, cap));
  KHR_CHAIN(devAlloc(c, &m.dist, cap * nv, false));
  KHR_CHAIN(devAlloc(c, &m.weight, cap * nv, false));
  KHR_CHAIN(devAlloc(c, &m.color, cap * nv, false));
  KHR_CHAIN(devAlloc(c, &m.vflags, cap * nv, false));
  KHR_CHAIN(devAlloc(c, &m.sem_label, cfg->with_semantics ? cap * nv : 1, false));
  if (rc == KHR_OK && devAlloc(c, &m.lik, cfg->with_semantics ? cap * nv * p.KS : 1, false) != KHR_OK) {
    // (the largest layer of the pool: say what it needs and what the switch saves)
    fail(KHR_ENOMEM, "the label-likelihood layer of %zu blocks needs %.2f GB (%d floats per voxel%s); khr_config.packed_likelihood_rows = 1 "
                     "stores %d per voxel, a smaller max_blocks less of everything", static_cast<size_t>(cap),
         1e-9 * static_cast<double>(cap) * nv * p.KS * 4, p.KS, p.KS != p.K ? ": rows padded to 128-byte lines" : "", p.K);
    KHR_CHAIN(KHR_ENOMEM);
  }
  KHR_CHAIN(devAlloc(c, &m.last_obs, cfg->with_tracking ? cap * nv : 1, false));
  KHR_CHAIN(devAlloc(c, &m.last_occ, cfg->with_tracking ? cap * nv : 1, false));
  KHR_CHAIN(devAlloc(c, &m.trk_lim, cfg->with_tracking ? cap * 2 : 2));
  KHR_CHAIN(devAlloc(c, &m.freebits, cfg->with_tracking ? cap * (nv / 64) : 1, false));
  KHR_CHAIN(devAlloc(c, &m.obs, cfg->with_tracking ? cap * (nv / 64) : 1, false));
  KHR_CHAIN(devAlloc(c, &m.free_slots, cap, false));
  KHR_CHAIN(devAlloc(c, &m.counters, C_COUNT));
  KHR_CHAIN(devAlloc(c, &m.stats, S_COUNT));
  KHR_CHAIN(devAlloc(c, &m.mesh_desc, cap));
  KHR_CHAIN(devAlloc(c, &c->d_work, cap));
  KHR_CHAIN(devAlloc(c, &c->d_new, cap));
  KHR_CHAIN(devAlloc(c, &c->d_ef, cap));
  KHR_CHAIN(devAlloc(c, &c->d_trk_proc, cap));
  KHR_CHAIN(devAlloc(c, &c->d_dbg, 4096 * 4 * 12));
  KHR_CHAIN(devAlloc(c, &c->d_digest, kDigestWords));
  KHR_CHAIN(devAlloc(c, &c->d_wg_stats, 2 * kUpdateStatSlots));
  KHR_CHAIN(devAlloc(c, &c->d_fuse_sink, static_cast<size_t>(kUpdateStatSlots) * 16 * 256, false));
  KHR_CHAIN(devAlloc(c, &c->d_fetch_done, 4));
  {
    // shards of a >= 4-rank map and small frames (up to 640 x 480 pixels) see few blocks per launch: 8 z ranges per patch
    // instead of 4 halve the longest dependent chain (an item's band rounds) and double the items the waves can share.
    // A wave item is a 64-voxel patch x 4 (or 2) z steps; 8^3 blocks always take 4.
    const int zs = (cfg->voxels_per_side != 8 && (cfg->world_size >= 4 || cfg->max_frame_pixels <= 640u * 480u)) ? 8 : 4;
    c->fuse_zsplit = zs;
    c->wpb = static_cast<uint32_t>((cfg->voxels_per_side * cfg->voxels_per_side / 64) * zs);
    c->item_cap = static_cast<uint32_t>(cap) * c->wpb;
  }
  KHR_CHAIN(devAlloc(c, &c->d_work4, 2 * static_cast<size_t>(c->item_cap), false));
  if (cfg->voxels_per_side == 8 && rc == KHR_OK) {
    // an object mini-map: the buffers of its multi-frame update now, not at the first extraction -- that one runs beside the window's
    // frames, and a hipMalloc / hipHostMalloc there waits for (and stalls) every stream of the device (round 6: one run of the
    // driver's command in ten had a 3 ms step at its first extraction)
    const size_t bits_words = static_cast<size_t>(c->item_cap) * 4;  // four words per item = 128 buffered frames
    if (c->h_frames.alloc(kMaxMultiFrames) || c->d_frames.alloc(kMaxMultiFrames) || c->ev_frames.ensure() ||
        hipEventRecord(c->ev_frames, c->stream) != hipSuccess || c->d_frame_bits.alloc(bits_words) ||
        c->d_multi_list.alloc(3 * static_cast<size_t>(c->item_cap) + 2))  // (two lists, 4 + 1 counters, the untouched items)
      rc = fail(KHR_ENOMEM, "buffers of the multi-frame update");
    // ... and the small page-locked block and events its first extraction would otherwise create on the worker's thread
    if (rc == KHR_OK && (c->h_totals.alloc(C_COUNT + 2) || c->ev_up.ensure() || hipEventRecord(c->ev_up, c->stream) != hipSuccess ||
                         c->ev_dep.ensure() || c->ev_dep_aux.ensure()))
      rc = fail(KHR_ENOMEM, "page-locked words / events of an object mini-map");
  }
  KHR_CHAIN(devAlloc(c, &m.blk_band, cap * kBandSlots));
  KHR_CHAIN(devAlloc(c, &c->d_removed, cap));
  KHR_CHAIN(devAlloc(c, &c->d_mesh_count, cap + 1));
  KHR_CHAIN(devAlloc(c, &c->d_mesh_offset, cap + 1));
  KHR_CHAIN(devAlloc(c, &c->d_regen, cap));
  KHR_CHAIN(devAlloc(c, &c->d_mesh_old_off, cap + 1));
  KHR_CHAIN(devAlloc(c, &c->d_mh_flag, cap));
  KHR_CHAIN(devAlloc(c, &c->d_mesh_nwork, 8));
  const size_t npx = cfg->max_frame_pixels;
  KHR_CHAIN(devAlloc(c, &c->d_keys, npx, false));
  KHR_CHAIN(devAlloc(c, &c->d_pix, npx, false));
  {
    // voxel tables: every pixel can at most open one voxel; 2x slots keep probing short
    uint32_t ts = 1;
    while (ts < 2 * npx) ts <<= 1;
    c->md_mask = ts - 1;
    c->md_list_cap = static_cast<uint32_t>(std::min<size_t>(npx, 1u << 20));
    KHR_CHAIN(devAlloc(c, &c->d_md_keys, 3 * static_cast<size_t>(ts), false));
    KHR_CHAIN(devAlloc(c, &c->d_md_counts, 3 * static_cast<size_t>(ts), false));
    KHR_CHAIN(devAlloc(c, &c->d_md_ids, 3 * static_cast<size_t>(ts), false));
    {
      uint8_t* head = nullptr;
      KHR_CHAIN(devAlloc(c, &head, 16 + sizeof(CompAcc) * kCompCap));
      c->d_md_n = reinterpret_cast<uint32_t*>(head);
    }
    KHR_CHAIN(devAlloc(c, &c->d_md_parent, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_rootidx, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_edges, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_comp_acc, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_comp_final, kCompCap));
    KHR_CHAIN(c->h_md_head.alloc(16 + sizeof(CompAcc) * kCompCap));
    KHR_CHAIN(devAlloc(c, &c->d_md_scratch4, 16));  // [0..3] words k_publish may zero, [8..13] voxel box of the seed voxels
    c->md_host_walk = std::getenv("KHR_MD_HOST_WALK") != nullptr;
    if (const char* e = std::getenv("KHR_MD_LDS_MAX")) c->md_lds_max = std::min<uint32_t>(kCompLds, static_cast<uint32_t>(std::atoi(e)));
    KHR_CHAIN(devAlloc(c, &c->d_md_seed_keys, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_bnd_keys, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_seed_counts, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_bnd_counts, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_seed_final, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_bnd_final, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_bnd_deg, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_bnd_mask, c->md_list_cap, false));
    KHR_CHAIN(devAlloc(c, &c->d_md_adj, static_cast<size_t>(c->md_list_cap) * 26, false));
    // the host walk's page-locked block (lists + final ids), for 16 k seed voxels to begin with (grown on demand: a growth is a hipHostMalloc inside a frame)
    KHR_CHAIN(c->h_md_walk.alloc(std::min<size_t>(c->md_list_cap, 16384) * (3 + 26 + 3 + 3) + 16));
    // (not zeroed: devAlloc's memset is queued on the context's NON-BLOCKING stream, and the synchronous copy of the reduction
    //  identities below runs on the null stream -- nothing orders the two, and a memset that lands second leaves zeros, i.e.
    //  boxes clamped at 0 for the first seed frame's clusters.  Found by tests/test_gpu_ref_pin.py.)
    KHR_CHAIN(devAlloc(c, &c->d_md_acc, 256, false));
    KHR_CHAIN(c->h_md_acc_pinned.alloc(256));
    {
      std::vector<ClusterAcc> init(256);
      for (auto& a : init) clusterAccReset(a);
      KHR_CHAIN(hipMemcpy(c->d_md_acc, init.data(), sizeof(ClusterAcc) * 256, hipMemcpyHostToDevice) != hipSuccess ? KHR_EDEVICE : KHR_OK);
    }
  }
  if (rc == KHR_OK) {
    size_t t3 = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, t3, c->d_mesh_count, c->d_mesh_offset, static_cast<int>(cap + 1), c->stream);
    c->cub_temp_bytes = t3 + 256;
    uint8_t* tmp = nullptr;
    KHR_CHAIN(devAlloc(c, &tmp, c->cub_temp_bytes, false));
    c->d_cub_temp = tmp;
  }
  for (int b = 0; b < 2 && rc == KHR_OK; ++b) {
    KHR_CHAIN(devAlloc(c, &c->mesh[b].points, cfg->max_mesh_vertices * 3, false));
    KHR_CHAIN(devAlloc(c, &c->mesh[b].colors, cfg->max_mesh_vertices, false));
    KHR_CHAIN(devAlloc(c, &c->mesh[b].labels, cfg->max_mesh_vertices, false));
    KHR_CHAIN(devAlloc(c, &c->mesh[b].stamps, cfg->max_mesh_vertices, false));
  }
  c->slots.resize(cfg->num_frame_slots);
  c->slot_leases.reset(new std::atomic<int>[cfg->num_frame_slots]);
  for (uint32_t i = 0; i < cfg->num_frame_slots; ++i) c->slot_leases[i].store(0);
  for (auto& s : c->slots) {
    if (rc != KHR_OK) break;
    KHR_CHAIN(devAlloc(c, &s.depth, npx, false));
    KHR_CHAIN(devAlloc(c, &s.range, npx + 4, false));  // + pad: k_fuse gathers pixel pairs (u0, u0 + 1) with one 8-byte load
    KHR_CHAIN(devAlloc(c, &s.rgba, npx + 4, false));   // + pad: the band phase gathers colour pixel pairs like the range samples
    KHR_CHAIN(devAlloc(c, &s.label, npx, false));
    KHR_CHAIN(devAlloc(c, &s.dyn, npx));
    KHR_CHAIN(devAlloc(c, &s.dynw, npx, false));
    KHR_CHAIN(devAlloc(c, &s.obj, npx));
    KHR_CHAIN(devAlloc(c, &s.rgb_staging, npx * 3, false));
    KHR_CHAIN(devAlloc(c, &s.tile_max, npx / 16 + 64, false));
  }
  if (rc != KHR_OK) return rc;
  // initial state: empty hash, free list = identity, constant tables
  hipError_t e = hipMemsetAsync(m.ht_keys, 0xff, sizeof(uint64_t) * ht, c->stream);
  if (e == hipSuccess) {
    std::vector<uint32_t> ident(cap);
    for (size_t i = 0; i < cap; ++i) ident[i] = static_cast<uint32_t>(i);
    e = hipMemcpyAsync(m.free_slots, ident.data(), sizeof(uint32_t) * cap, hipMemcpyHostToDevice, c->stream);
    uint32_t ctr[C_COUNT] = {0};
    ctr[C_N_FREE] = static_cast<uint32_t>(cap);
    if (e == hipSuccess) e = hipMemcpyAsync(m.counters, ctr, sizeof(ctr), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_mc_tri), kMcTriTable, sizeof(kMcTriTable));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_mc_ntri), kMcNumTris, sizeof(kMcNumTris));
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e != hipSuccess) return fail(KHR_EDEVICE, "context initialisation failed: %s", hipGetErrorString(e));
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live_ctx.push_back(c);
  }
  *out = owner.release();
  return KHR_OK;
}

// What depends on order is here; everything else is released by the members' destructors (the streams last).
void khr_destroy(khr_ctx* c) {
  if (!c) return;
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live_ctx.erase(std::remove(g_live_ctx.begin(), g_live_ctx.end(), c), g_live_ctx.end());
  }
  hipSetDevice(c->device);
  for (Stream* st : {&c->stream, &c->aux_stream, &c->h2d_stream, &c->snap_stream, &c->mc_stream, &c->copy_stream})
    if (*st) hipStreamSynchronize(*st);
  resolveTimers(c);
  if (c->pending_snapshot) khr_snapshot_release(c->pending_snapshot);
  {
    std::lock_guard<std::mutex> lock(c->snap_pool->mu);
    c->snap_pool->dead = true;  // snapshots still held by a consumer free their arenas themselves from now on
    c->snap_pool->free.clear();
  }
  {
    std::lock_guard<std::mutex> lock(c->frame_pool->mu);
    c->frame_pool->dead = true;  // frame copies still held by a consumer free their blocks themselves from now on
    c->frame_pool->free.clear();
  }
  delete c;
}

int khr_set_stream(khr_ctx* c, void* hip_stream) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->aux_stream));
  if (hip_stream) {
    c->stream.refer(static_cast<hipStream_t>(hip_stream));
    return KHR_OK;
  }
  return createStream(c, c->stream);
}

int khr_sync(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->aux_stream));
  return KHR_OK;
}

// the auxiliary stream continues behind everything queued on the main stream so far (a frame's ingest, a painted
// dynamic image)
static int auxAfterMain(khr_ctx* c) {
  HIP_TRY(hipEventRecord(c->ev_aux, c->stream));
  HIP_TRY(hipStreamWaitEvent(c->aux_stream, c->ev_aux, 0));
  return KHR_OK;
}

// next slot of the frame ring that nobody holds
// the slot acquireSlot would hand out next (-1: none free); no side effects
static int peekSlot(const khr_ctx* c) {
  const int n_slots = static_cast<int>(c->slots.size());
  for (int k = 0; k < n_slots; ++k) {
    const int cand = (c->next_slot + k) % n_slots;
    if (c->slot_leases[cand].load(std::memory_order_acquire) == 0) return cand;
  }
  return -1;
}

static int acquireSlot(khr_ctx* c) {
  const int n_slots = static_cast<int>(c->slots.size());
  int slot = -1;
  for (int k = 0; k < n_slots && slot < 0; ++k) {
    const int cand = (c->next_slot + k) % n_slots;
    if (c->slot_leases[cand].load(std::memory_order_acquire) == 0) slot = cand;
  }
  if (slot < 0) return fail(KHR_ENOMEM, "all %d frame slots are retained (raise num_frame_slots)", n_slots);
  c->next_slot = (slot + 1) % n_slots;
  if (c->slots[slot].aux_seq > c->aux_seq_done) {  // the auxiliary stream may still be reading the previous occupant (tiny rings only)
    const uint64_t upto = c->aux_seq_issued;
    if (hipStreamQuery(c->aux_stream) != hipSuccess) HIP_TRY(hipStreamSynchronize(c->aux_stream));
    c->aux_seq_done = upto;
  }
  c->slots[slot].aux_seq = 0;
  FrameSlot& fs = c->slots[slot];
  fs.x_depth = fs.x_range = nullptr, fs.x_rgba = nullptr, fs.x_label = nullptr, fs.x_tile_max = nullptr;
  return slot;
}

// is `slot` a frame of this context that can be read?
static bool validSlot(const khr_ctx* c, int slot) {
  return slot >= 0 && slot < static_cast<int>(c->slots.size()) && c->slots[slot].valid;
}

static int checkSensor(const khr_ctx* c, const khr_sensor* sensor) {
  const size_t n = static_cast<size_t>(sensor->width) * sensor->height;
  if (sensor->width < 2 || sensor->height < 2 || n > c->cfg.max_frame_pixels)
    return fail(KHR_EINVAL, "frame %dx%d exceeds max_frame_pixels=%u", sensor->width, sensor->height, c->cfg.max_frame_pixels);
  if (!(sensor->fx > 0.f) || !(sensor->fy > 0.f) || !(sensor->max_range > sensor->min_range))
    return fail(KHR_EINVAL, "bad intrinsics / range");
  return KHR_OK;
}

// a ring slot becomes a new frame: nothing of its previous occupant is left (`meta` without its plane pointers)
static FrameSlot& newFrameSlot(khr_ctx* c, int slot, const khr_sensor& sensor, const khr_frame& meta, bool has_color, bool has_label,
                               bool valid) {
  FrameSlot& s = c->slots[slot];
  s.valid = valid;
  s.sensor = sensor;
  s.meta = meta;
  s.meta.depth = nullptr;
  s.meta.color = nullptr;
  s.meta.label = nullptr;
  s.has_color = has_color;
  s.has_label = has_label;
  s.has_obj = false;
  if (c->obj_cv_slot == slot) c->obj_cv_slot = -1;
  s.objects_done = false;
  s.clusters.clear();
  s.sem_clusters.clear();
  s.tw = (sensor.width + kTile - 1) / kTile;
  s.th = (sensor.height + kTile - 1) / kTile;
  s.dyn_clean = true, s.dynw_valid = false;
  return s;
}

// what the caller of an ingest chooses for its frame (khr_upload_frame: the defaults)
struct IngestOpts {
  hipStream_t stream = nullptr;  // where the ingest kernel runs, for device and page-locked inputs (nullptr: the main stream)
  bool pinned = false;           // host buffers are page-locked: their copies go to the host-to-device stream, no host wait
  Event* h2d_event = nullptr;    // the event those copies record (nullptr: c->ev_h2d, and the context notes h2d_pending)
  bool begin = false;            // the ingest kernel also does k_begin_integrate's work
};

static int uploadFrame(khr_ctx* c, const khr_sensor* sensor, const khr_frame* frame, int on_device, const IngestOpts& opts) {
  if (!c || !sensor || !frame || !frame->depth) return fail(KHR_EINVAL, "null argument");
  KHR_TRY(checkSensor(c, sensor));
  const size_t n = static_cast<size_t>(sensor->width) * sensor->height;
  HIP_TRY(hipSetDevice(c->device));
  // next slot of the ring that nobody holds (khr_retain_slot): buffered frames and frames a detached extraction still reads
  // stay intact however far the stream has advanced
  const int slot = acquireSlot(c);
  if (slot < 0) return slot;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // not valid until the ingest is queued: an error below leaves a slot nobody can integrate, not the previous occupant
  FrameSlot& s = newFrameSlot(c, slot, *sensor, *frame, frame->color != nullptr, frame->label != nullptr, false);
  const bool pinned = !on_device && opts.pinned;
  hipStream_t ist = ((on_device || pinned) && opts.stream) ? opts.stream : static_cast<hipStream_t>(c->stream);
  Event& evh = opts.h2d_event ? *opts.h2d_event : c->ev_h2d;
  ScopedTimer tm(c, ist == c->stream ? 6 : -1);
  const float* depth_src = frame->depth;
  const uint8_t* rgb_src = frame->color;
  const int32_t* label_src = frame->label;
  if (!on_device) {  // host buffers: stage them in the slot, the ingest kernel then works in place
    // page-locked caller memory (KHR_PF_INPUT_PINNED): the planes travel on the context's host-to-device stream while whatever
    // is queued on the other streams runs, the ingest waits for them on the device, the host does not wait at all -- the
    // caller keeps the buffers untouched until the next khr_process_frame / khr_sync on this context has returned.
    // Pageable memory: copies on the ingest's own stream and a host wait below (the caller may reuse the memory at once).
    hipStream_t cs = c->stream;
    if (pinned) {
      if (!c->h2d_stream) KHR_TRY(createStream(c, c->h2d_stream));
      KHR_TRY(evh.ensure());
      cs = c->h2d_stream;
      if (ist == c->stream) {  // main-stream ingest: the slot's previous readers are ordered in front of it, so must the copy be
        KHR_TRY(c->ev_ingest.ensure());
        HIP_TRY(hipEventRecord(c->ev_ingest, c->stream));
        HIP_TRY(hipStreamWaitEvent(cs, c->ev_ingest, 0));
      }
    }
    HIP_TRY(hipMemcpyAsync(s.depth, frame->depth, n * sizeof(float), kind, cs));
    depth_src = s.depth;
    if (frame->color) {
      HIP_TRY(hipMemcpyAsync(s.rgb_staging, frame->color, n * 3, kind, cs));
      rgb_src = s.rgb_staging;
    }
    if (frame->label) {
      HIP_TRY(hipMemcpyAsync(s.label, frame->label, n * sizeof(int32_t), kind, cs));
      label_src = s.label;
    }
    if (pinned) {
      HIP_TRY(hipEventRecord(evh, cs));
      HIP_TRY(hipStreamWaitEvent(ist, evh, 0));
      if (!opts.h2d_event) c->h2d_pending = true;
      c->h2d_bytes += n * (4u + (frame->color ? 3u : 0u) + (frame->label ? 4u : 0u));
    }
  }
  hipLaunchKernelGGL(k_frame_ingest, dim3(s.tw * s.th), dim3(256), 0, ist, depth_src, rgb_src, label_src, s.depth,
                     s.range, s.rgba, s.label, s.dyn, s.tile_max, s.tw, sensor->width, sensor->height, sensor->fx, sensor->fy,
                     sensor->cx, sensor->cy, c->p.range_mode, c->m, c->p.nvox, c->d_wg_stats, opts.begin ? 1 : 0);
  HIP_TRY(hipGetLastError());
  c->begun = opts.begin;
  if (!on_device && !pinned) HIP_TRY(hipStreamSynchronize(c->stream));  // caller buffers may be reused after return
  s.valid = true;
  return slot;
}

int khr_upload_frame(khr_ctx* c, const khr_sensor* sensor, const khr_frame* frame, int on_device) {
  return uploadFrame(c, sensor, frame, on_device, IngestOpts{});
}

int khr_set_frame_image(khr_ctx* c, int slot, int which, const int32_t* image, int on_device) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  FrameSlot& s = c->slots[slot];
  const size_t n = static_cast<size_t>(s.sensor.width) * s.sensor.height;
  int32_t* dst = which == 0 ? s.dyn : s.obj;
  if (image) {
    HIP_TRY(hipMemcpyAsync(dst, image, n * sizeof(int32_t), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if (!on_device) HIP_TRY(hipStreamSynchronize(c->stream));
  } else {
    HIP_TRY(hipMemsetAsync(dst, 0, n * sizeof(int32_t), c->stream));
  }
  if (which == 1) s.has_obj = image != nullptr;
  if (which == 1 && c->obj_cv_slot == slot) c->obj_cv_slot = -1;  // (voxel sets queued for the image this one replaces)
  if (which == 0) s.dyn_clean = image == nullptr;
  if (which == 0) s.dynw_valid = false;  // (an installed image brings no list multiplicities: its summaries count every pixel once)
  if (which == 1) {  // an object image written here is read by kernels of the auxiliary stream (voxel sets)
    const int rca = auxAfterMain(c);
    if (rca) return rca;
  }
  return KHR_OK;
}

int khr_download_frame(khr_ctx* c, int slot, float* range, float* vertex_map, int32_t* dynamic_image) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  FrameSlot& s = c->slots[slot];
  const size_t n = static_cast<size_t>(s.sensor.width) * s.sensor.height;
  if (range) HIP_TRY(hipMemcpyAsync(range, s.vRange(), n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (dynamic_image) HIP_TRY(hipMemcpyAsync(dynamic_image, s.dyn, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (vertex_map) {
    DevTemp tmpv;
    KHR_TRY(tmpv.alloc(n * 3 * sizeof(float)));
    float* d_v = tmpv.as<float>();
    hipLaunchKernelGGL(k_vertex_map, dim3(gridFor(n)), dim3(256), 0, c->stream, makeDevFrame(c, s), d_v);
    HIP_TRY(hipMemcpyAsync(vertex_map, d_v, n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

struct khr_frame_copy {
  std::shared_ptr<khr_ctx::FramePool> pool;
  DevBuf<uint8_t> block;  // (out of the pool: may be larger than this frame needs)
  int device = 0;
  Event ready;  // recorded behind the copy kernel
  DevFrame f{};                // intrinsics + pose of the frame; the plane pointers refer to `block`
  size_t n = 0, n_pad = 0;
};

int khr_frame_copy_create(khr_ctx* c, int slot, khr_frame_copy** out) {
  if (!c || !out || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const size_t n = static_cast<size_t>(s.sensor.width) * s.sensor.height, n_pad = (n + 3) / 4 * 4;
  if (n_pad > c->cfg.max_frame_pixels) return fail(KHR_EINVAL, "frame larger than max_frame_pixels");
  auto fc = std::make_unique<khr_frame_copy>();
  fc->pool = c->frame_pool;
  fc->device = c->device;
  const size_t bytes = 16 * n_pad;
  {
    std::lock_guard<std::mutex> lock(c->frame_pool->mu);
    auto& fr = c->frame_pool->free;
    for (size_t i = 0; i < fr.size(); ++i)
      if (fr[i].count() >= bytes) {
        fc->block = std::move(fr[i]);
        fr.erase(fr.begin() + static_cast<long>(i));
        break;
      }
  }
  if (!fc->block && fc->block.alloc(bytes)) return fail(KHR_ENOMEM, "frame copy (%zu bytes)", bytes);
  if (fc->ready.ensure()) return fail(KHR_EDEVICE, "event");
  // (the slot's planes are allocated for max_frame_pixels: reading the padding of the last 16-byte vector is inside the allocation)
  if (s.aux_seq) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_aux_done, 0));  // (an ingest queued on the auxiliary stream)
  hipLaunchKernelGGL(k_frame_copy, dim3(512), dim3(256), 0, c->stream, reinterpret_cast<const uint4*>(s.vDepth()),
                     reinterpret_cast<const uint4*>(s.vRange()), s.has_color ? reinterpret_cast<const uint4*>(s.vRgba()) : nullptr,
                     s.has_label ? reinterpret_cast<const uint4*>(s.vLabel()) : nullptr, reinterpret_cast<uint4*>(fc->block.get()),
                     static_cast<uint32_t>(n_pad / 4));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(fc->ready, c->stream));
  fc->f = makeDevFrame(c, s);
  fc->f.depth = reinterpret_cast<const float*>(fc->block.get());
  fc->f.range = reinterpret_cast<const float*>(fc->block + 4 * n_pad);
  fc->f.rgba = reinterpret_cast<const uint32_t*>(fc->block + 8 * n_pad);
  fc->f.label = reinterpret_cast<const int32_t*>(fc->block + 12 * n_pad);
  fc->f.dyn = nullptr;
  fc->f.obj = nullptr;
  fc->n = n;
  fc->n_pad = n_pad;
  *out = fc.release();
  return KHR_OK;
}

int khr_frame_copy_download(khr_frame_copy* fc, float* depth, float* range, uint8_t* color_rgb, int32_t* labels, float* vertex_map) {
  if (!fc) return fail(KHR_EINVAL, "null frame copy");
  HIP_TRY(hipSetDevice(fc->device));
  HIP_TRY(hipEventSynchronize(fc->ready));
  const size_t n = fc->n;
  if (depth) HIP_TRY(hipMemcpy(depth, fc->f.depth, n * 4, hipMemcpyDeviceToHost));
  if (range) HIP_TRY(hipMemcpy(range, fc->f.range, n * 4, hipMemcpyDeviceToHost));
  if (labels) HIP_TRY(hipMemcpy(labels, fc->f.label, n * 4, hipMemcpyDeviceToHost));
  if (color_rgb || vertex_map) {
    DevTemp tmp;
    KHR_TRY(tmp.alloc(n * 12));
    if (color_rgb) {
      hipLaunchKernelGGL(k_rgba_to_rgb, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, fc->f.rgba, tmp.as<uint8_t>(), static_cast<uint32_t>(n));
      HIP_TRY(hipMemcpy(color_rgb, tmp.get(), n * 3, hipMemcpyDeviceToHost));
    }
    if (vertex_map) {
      hipLaunchKernelGGL(k_vertex_map, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, nullptr, fc->f, tmp.as<float>());
      HIP_TRY(hipMemcpy(vertex_map, tmp.get(), n * 12, hipMemcpyDeviceToHost));
    }
  }
  return KHR_OK;
}

void khr_frame_copy_release(khr_frame_copy* fc) {
  if (!fc) return;
  hipSetDevice(fc->device);
  if (fc->ready) hipEventSynchronize(fc->ready);  // (the block goes back to the pool: nothing may still be writing it)
  {
    std::lock_guard<std::mutex> lock(fc->pool->mu);
    if (!fc->pool->dead && fc->pool->free.size() < 8) fc->pool->free.push_back(std::move(fc->block));
  }
  delete fc;  // (frees the block unless the pool took it)
}

int khr_copy_frame_image(khr_ctx* c, int slot, int which, void* device_dst) {
  if (!c || !device_dst || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  if (which != 0 && which != 1) return fail(KHR_EINVAL, "which must be 0 (dynamic) or 1 (object)");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const size_t n = static_cast<size_t>(s.sensor.width) * s.sensor.height;
  if (which == 1 && !s.has_obj) {
    HIP_TRY(hipMemsetAsync(device_dst, 0, n * sizeof(int32_t), c->stream));
    return KHR_OK;
  }
  if (which == 1) {  // painted / remapped by the object detector's stream
    HIP_TRY(hipEventRecord(c->ev_aux_done, c->aux_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_aux_done, 0));
  }
  HIP_TRY(hipMemcpyAsync(device_dst, which == 0 ? s.dyn : s.obj, n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
  return KHR_OK;
}

int khr_download_frame_image(khr_ctx* c, int slot, int which, int32_t* image) {
  if (!c || !image || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  if (which != 0 && which != 1) return fail(KHR_EINVAL, "which must be 0 (dynamic) or 1 (object)");
  FrameSlot& s = c->slots[slot];
  const size_t n = static_cast<size_t>(s.sensor.width) * s.sensor.height;
  if (which == 1 && !s.has_obj) {  // never written: FrameData::object_image starts as zeros (active_window.cpp:284)
    std::memset(image, 0, n * sizeof(int32_t));
    return KHR_OK;
  }
  if (which == 1) HIP_TRY(hipStreamSynchronize(c->aux_stream));  // painted / remapped by the object detector's stream
  HIP_TRY(hipMemcpyAsync(image, which == 0 ? s.dyn : s.obj, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

// block allocation + culling of one integrate call (independent of the dynamic mask)
static int integrateAlloc(khr_ctx* c, FrameSlot& s, const DevFrame& f, int allocate_blocks) {
  DevMap& m = c->m;
  // khr_begin_object_map has done the per-call reset AND listed the box's blocks (k_setup_box): nothing to launch
  const bool listed = c->box_listed;
  c->box_listed = false;
  if (listed) {
    if (!allocate_blocks && c->box_gen == c->map_gen) return KHR_OK;
    // (the block set has changed since, or this integration builds its own lists: back to the state behind k_begin_integrate, whose
    // statistics are in already)
    HIP_TRY(hipMemsetAsync(&m.counters[C_N_VISIBLE], 0, 2 * sizeof(uint32_t), c->stream));  // C_N_VISIBLE, C_N_NEW
    HIP_TRY(hipMemsetAsync(&m.counters[C_N_ITEMS0], 0, 4 * sizeof(uint32_t), c->stream));
    c->begun = true;
  }
  // reset per-call counters (already done by k_frame_ingest inside khr_process_frame)
  if (!c->begun) hipLaunchKernelGGL(k_begin_integrate, dim3(1), dim3(256), 0, c->stream, m, c->p.nvox, c->d_wg_stats);
  c->begun = false;
  if (allocate_blocks) {
    ScopedTimer tm(c, 3);
    const DevFrustum fr = makeFrustum(c, f);
    const int S = 2 * fr.n_steps + 1;
    const size_t total = static_cast<size_t>(S) * S * S;
    hipLaunchKernelGGL(k_alloc_visible, dim3(gridFor(total)), dim3(256), 0, c->stream, m, c->p, f, fr, c->d_work, c->d_new,
                       c->h_pinned.dev() + 2, c->seed_publish_pending ? c->seed_ticket : 0u, &m.counters[C_N_VISIBLE], 0);
    c->seed_publish_pending = false;
    hipLaunchKernelGGL(k_init_cull, dim3(1024 + 1024), dim3(256), 0, c->stream, m, c->p, f, c->d_new, c->d_work,
                       FuseList{c->d_work4, c->d_work4 + c->item_cap, c->item_cap, &m.counters[C_N_ITEMS0]}, c->wpb,
                       c->cfg.disable_culling ? nullptr : s.vTileMax(), s.tw, s.th, 1024u);
    c->host_index_valid = false, ++c->map_gen;
  } else {
    hipLaunchKernelGGL(k_list_live, dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m, c->d_work,
                       &m.counters[C_N_VISIBLE], 0u, FuseList{c->d_work4, c->d_work4 + c->item_cap, c->item_cap, &m.counters[C_N_ITEMS0]},
                       c->wpb);
  }
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

// the fused TSDF / colour / label update kernel of one integrate call (k_fuse)
// tick path: the camera's own work list
struct UpdateLists {
  FuseList list{nullptr, nullptr, 0u, nullptr};
};

// resident workgroups of a k_fuse instantiation x CUs, rounded down to whole XCD rounds (the grid is persistent: static
// striding over the work items, so workgroups beyond residency would only add a tail)
static int fuseGrid(khr_ctx* c, const void* kernel, int group, int block) {
  static std::map<std::pair<int, const void*>, int> cache;  // (per device: the grid depends on its CU count)
  static std::mutex cache_mu;  // contexts of different threads (active window + extraction workers) launch concurrently
  std::lock_guard<std::mutex> lock(cache_mu);
  const std::pair<int, const void*> key{c->device, kernel};
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  per_cu = std::min(per_cu, std::max(1, kUpdateWavesPerCu / (block / 64)));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  per_cu = std::min(per_cu, 8);
  int grid = std::min(kUpdateStatSlots, per_cu * cus);
  grid = std::max(8 * group, grid / (8 * group) * (8 * group));
  cache[key] = grid;
  return grid;
}

// the per-frame part of the update kernel's arguments
// resident workgroups of a k_fuse2 instantiation x CUs (occupancy query, cached per kernel)
static int fuse2Grid(khr_ctx* c, const void* kern, int wpw) {
  static std::map<std::pair<int, const void*>, int> cache;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  const std::pair<int, const void*> key{c->device, kern};
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * wpw, 0) != hipSuccess || per_cu < 1) per_cu = 1;
  hipDeviceProp_t prop;
  int cus = 256;
  if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  const int grid = std::min(kUpdateStatSlots, per_cu * cus) / 8 * 8;
  cache[key] = grid;
  return grid;
}

static void fillFuseFrame(const khr_ctx* c, const FrameSlot& s, const DevFrame& f, int use_mask, int object_id, FuseFrame* a) {
  a->range = f.range; a->dyn = f.dyn; a->rgba = f.rgba; a->label = f.label; a->obj = f.obj;
  a->W = f.W; a->H = f.H; a->fx = f.fx; a->fy = f.fy; a->cx = f.cx; a->cy = f.cy; a->min_range = f.min_range; a->max_range = f.max_range;
  std::memcpy(a->R, f.R, sizeof(a->R));
  std::memcpy(a->t, f.t, sizeof(a->t));
  a->stamp = f.stamp;
  // a dynamic image nobody has painted since the ingest is all zero: the mask cannot reject anything
  a->use_mask = (use_mask && !s.dyn_clean) ? 1 : 0;
  a->has_color = f.has_color;
  a->object_id = object_id;
  a->do_sem = (c->p.with_semantics && ((c->p.sem_mode == 1) ? (object_id >= 0 && f.obj != nullptr) : (f.has_label != 0))) ? 1 : 0;
  a->tile_max = s.vTileMax();
  a->tw = s.tw;
  a->th = s.th;
}
static void fillFuseMap(khr_ctx* c, FuseArgs* a) {
  DevMap& m = c->m;
  a->blk_index = m.blk_index; a->blk_flags = m.blk_flags; a->dist = m.dist; a->weight = m.weight; a->last_obs = m.last_obs; a->obs = m.obs;
  a->color = m.color; a->vflags = m.vflags; a->sem_label = m.sem_label; a->lik = m.lik; a->wg_stats = c->d_wg_stats;
  a->blk_band = m.blk_band;
  a->vs = c->p.vs; a->bs = c->p.bs; a->trunc = c->p.trunc; a->dropoff_eps = c->p.dropoff_eps; a->max_weight = c->p.max_weight;
  a->adaptive_diff = c->p.adaptive_diff; a->log_match = c->p.log_match; a->log_nomatch = c->p.log_nomatch;
  a->interp = c->p.interp; a->range_mode = c->p.range_mode; a->use_dropoff = c->p.use_dropoff; a->const_weight = c->p.const_weight;
  a->with_tracking = c->p.with_tracking;
  a->K = c->p.K; a->KS = c->p.KS; a->sem_mode = c->p.sem_mode;
  // whole-line rows pay where the memory path is busy; small frames (up to 640 x 480: 3 - 5 k items, fewer than two per wave) are one
  // dependent chain per wave, and there the shorter lane <-> record form wins (c1: 17.8 - 18.3 against 20.3 us).  Decided HERE, not
  // from the item count inside the kernel: one more value alive in k_fuse's band dispatch tipped the register allocator into
  // spilling vector registers inside the item loop (scratch traffic is vector memory: every wait became vmcnt(0), 72 -> 95 us;
  // tests/test_cpu_host.py::test_update_kernel_keeps_its_registers guards the build against that)
  a->band_mode = c->cfg.max_frame_pixels <= 640u * 480u ? 0 : 1;
  if (!fuseBandRowLanesOk(c->p.KS)) a->band_mode = 0;  // (rows whose lanes do not divide a wave: khr_kernels_fuse.h)
  a->sink = c->d_fuse_sink;
  a->blend_pre = c->cfg.color_blend_weight != 0;
}

// the pruning request of a batch goes with its last launch only
static FusePrune lastChunk(const FusePrune& pr, bool last) { return last ? pr : FusePrune{}; }

// The frames of a batch in one launch per kMultiChunk of them (k_fuse_obj for the extractor's binary object map, k_fuse2 otherwise):
// every wave item is walked through the frames in order.  Only for `allocate = false` integrations of 8^3-voxel maps with the
// default integrator switches (the object extractor's mini-map);
// returns 1 when the batch was not taken (the caller then integrates frame by frame).
// the extractor's confidence pruning behind a batch (khr_integrate_prune_batch); `fused` reports whether the update's last launch did it
struct PruneRequest {
  float min_confidence, min_observations;
  bool fused;
};

// does integrateUpdateMulti take a batch of n_frames frames?
static bool multiApplies(const khr_ctx* c, int n_frames) {
  if (c->cfg.voxels_per_side != 8 || n_frames < 2 || n_frames > kMaxMultiFrames) return false;
  return c->p.range_mode == 0 && c->p.interp == 2 && c->p.use_dropoff && !c->p.const_weight;  // (the default integrator switches)
}

static int integrateUpdateMulti(khr_ctx* c, khr_ctx* src, const int* src_slots, const int* object_ids, int n_frames, int use_mask,
                                PruneRequest* prune = nullptr) {
  if (!multiApplies(c, n_frames)) return 1;
  FuseArgs a{};
  fillFuseMap(c, &a);
  // per-frame arguments: pinned staging -> device array (reused only after the previous batch's copy has been consumed)
  if (!c->h_frames) {
    if (c->h_frames.alloc(kMaxMultiFrames) || c->d_frames.alloc(kMaxMultiFrames)) return fail(KHR_ENOMEM, "frame argument staging");
    KHR_TRY(c->ev_frames.ensure());
  } else {
    HIP_TRY(hipEventSynchronize(c->ev_frames));
  }
  for (int i = 0; i < n_frames; ++i) {
    FrameSlot& s = src->slots[src_slots[i]];
    const DevFrame f = makeDevFrame(src, s);
    fillFuseFrame(c, s, f, use_mask, object_ids ? object_ids[i] : -1, &c->h_frames[i]);
  }
  // the frames' arguments reach the device array through a kernel that reads the page-locked staging block (not a hipMemcpyAsync:
  // issued from an extraction worker's thread it can sit for milliseconds behind the window thread's frame transfers, round 5)
  {
    const uint32_t n_words = static_cast<uint32_t>(sizeof(FuseFrame) / 4) * static_cast<uint32_t>(n_frames);
    hipLaunchKernelGGL(k_copy_words, dim3((n_words + 255) / 256), dim3(256), 0, c->stream, reinterpret_cast<const uint32_t*>(c->h_frames.dev()),
                       reinterpret_cast<uint32_t*>(c->d_frames.get()), n_words);
  }
  HIP_TRY(hipEventRecord(c->ev_frames, c->stream));
  static_cast<FuseFrame&>(a) = c->h_frames[0];  // (the head frame; k_fuse2 itself reads a.frames)
  a.frames = c->d_frames;
  a.n_frames = n_frames;
  // which frames can touch which item (k_multi_cull): one bit per (item, frame), read by the update kernel through the scalar cache
  if (c->item_cap > 0) {
    const int n_words = (n_frames + 31) / 32;
    const size_t need = static_cast<size_t>(c->item_cap) * static_cast<size_t>(n_words);
    if (need > c->d_frame_bits.count()) {  // (grown in steps of four words per item = 128 frames: a worker thread's hipMalloc waits for the device)
      const size_t want = static_cast<size_t>(c->item_cap) * static_cast<size_t>((n_words + 3) / 4 * 4);
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (c->d_frame_bits.reserve(want)) return fail(KHR_ENOMEM, "frame bits of the multi-frame update (%zu bytes)", want * sizeof(uint32_t));
    }
    const uint64_t tests = static_cast<uint64_t>(c->explicit_blocks > 0 ? std::min<uint64_t>(c->explicit_blocks, c->m.capacity) : c->m.capacity) *
                           c->wpb * static_cast<uint64_t>(n_words) * 32u;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((tests + 255) / 256, 8192));
    hipLaunchKernelGGL((k_multi_cull<8>), dim3(std::max(1u, grid)), dim3(256), 0, c->stream, c->m.blk_flags, c->m.blk_index, &c->m.counters[C_MAX_SLOT],
                       c->p.vs, c->p.bs, c->p.trunc, static_cast<const FuseFrame*>(c->d_frames.get()), n_frames, n_words, c->wpb, BLK_LIVE, c->d_frame_bits);
    HIP_TRY(hipGetLastError());
    a.frame_bits = c->d_frame_bits;
    a.frame_words = n_words;
  }
  FuseList list{c->d_work4, c->d_work4 + c->item_cap, c->item_cap, &c->m.counters[C_N_ITEMS0]};
  // the extractor's configuration (binary object layer, no tracking stamps) has a kernel of its own that keeps the whole voxel
  // state in registers across a launch's frames (k_fuse_obj); every other map keeps k_fuse2
  const bool object_map = c->p.with_semantics && a.sem_mode == 1 && a.K == 2 && a.KS == 2 && !a.with_tracking;
  // ... and that kernel prunes in the batch's last launch, given the list of the items no frame touches (k_multi_order)
  const bool fuse_prune = prune != nullptr && object_map && a.frame_bits != nullptr;
  if (a.frame_bits != nullptr) {
    // ... and the items in the order of their frame counts, the untouched ones left out (k_multi_order): a list of its own
    if (!c->d_multi_list) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (c->d_multi_list.alloc(3 * static_cast<size_t>(c->item_cap) + 2)) return fail(KHR_ENOMEM, "item list of the multi-frame update");
    }
    uint32_t* const counts = reinterpret_cast<uint32_t*>(c->d_multi_list + 2 * static_cast<size_t>(c->item_cap));
    if (!(c->multi_counts_zeroed && c->box_gen == c->map_gen)) HIP_TRY(hipMemsetAsync(counts, 0, 32, c->stream));  // (class counters + the tail's)
    c->multi_counts_zeroed = false;
    list = FuseList{c->d_multi_list, c->d_multi_list + c->item_cap, c->item_cap, counts};
    const uint64_t n_it = static_cast<uint64_t>(c->explicit_blocks > 0 ? std::min<uint64_t>(c->explicit_blocks, c->m.capacity) : c->m.capacity) * c->wpb;
    hipLaunchKernelGGL(k_multi_order, dim3(static_cast<unsigned>((n_it + 1023) / 1024)), dim3(1024), 0, c->stream, c->m.blk_flags, c->m.blk_index,
                       &c->m.counters[C_MAX_SLOT], static_cast<const uint32_t*>(c->d_frame_bits.get()), a.frame_words, n_frames, c->wpb, BLK_LIVE, list,
                       fuse_prune ? c->d_multi_list + 2 * static_cast<size_t>(c->item_cap) + 2 : static_cast<uint4*>(nullptr),
                       fuse_prune ? counts + 4 : static_cast<uint32_t*>(nullptr));
    HIP_TRY(hipGetLastError());
  }
  constexpr int WPW = 8;
  auto go = [&](auto kern, auto... extra) {
    // one workgroup per WPW items is enough (c->explicit_blocks bounds the map), at most what is resident
    // (fuse2Grid: the occupancy query is a driver call of tens of microseconds, once per instantiation, not once per extracted object)
    int grid = fuse2Grid(c, reinterpret_cast<const void*>(kern), WPW);
    if (c->explicit_blocks > 0) {
      const uint64_t items = c->explicit_blocks * c->wpb;
      grid = std::max(8, static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(grid), (items + WPW - 1) / WPW) + 7) / 8 * 8);
    }
    // the buffered frames in chunks of kMultiChunk per launch: the next chunk's workgroups cannot start before the
    // current chunk has drained, so the window's update kernel -- whose workgroup needs a whole CU's vector registers -- gets its CUs
    // within one chunk instead of within the whole extraction (an item's distance / weight pass through HBM at the chunk boundaries)
    for (int k0 = 0; k0 < n_frames; k0 += kMultiChunk) {
      a.frames = c->d_frames + k0;
      a.n_frames = std::min(kMultiChunk, n_frames - k0);
      a.frame_bit0 = k0;
      KHR_LAUNCH_TIMED(0, kern, dim3(grid), dim3(64 * WPW), a, list, lastChunk(extra, k0 + kMultiChunk >= n_frames)...);
    }
  };
  if (object_map) {
    FusePrune pr{};
    if (fuse_prune) {
      if (!(c->pruned_zeroed && c->box_gen == c->map_gen)) HIP_TRY(hipMemsetAsync(&c->m.stats[S_PRUNED], 0, sizeof(unsigned long long), c->stream));
      c->pruned_zeroed = false;
      const uint32_t* const counts = reinterpret_cast<const uint32_t*>(c->d_multi_list + 2 * static_cast<size_t>(c->item_cap));
      pr = FusePrune{1, prune->min_confidence, prune->min_observations, c->d_multi_list + 2 * static_cast<size_t>(c->item_cap) + 2, counts + 4,
                     &c->m.stats[S_PRUNED]};
      prune->fused = true;
    }
    if (exactArithmetic(c)) go(&k_fuse_obj<true, WPW, 4>, pr);
    else go(&k_fuse_obj<false, WPW, 4>, pr);
  } else {
    if (exactArithmetic(c)) go(&k_fuse2<8, 4, true, WPW, 4>);
    else go(&k_fuse2<8, 4, false, WPW, 4>);
  }
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

// defer_fold: the items' records are left to the next k_tracking_select (c->fold_pending) instead of a k_fuse_fold launch
static int integrateUpdate(khr_ctx* c, FrameSlot& s, const DevFrame& f, int allocate_blocks, int use_mask,
                           int object_id, bool defer_fold, const UpdateLists* lists = nullptr, const uint32_t* gate = nullptr) {
  DevMap& m = c->m;
  FuseList list{c->d_work4, c->d_work4 + c->item_cap, c->item_cap, &m.counters[C_N_ITEMS0]};
  if (lists) list = lists->list;
  FuseArgs a{};
  fillFuseMap(c, &a);
  fillFuseFrame(c, s, f, use_mask, object_id, &a);
  const bool defcfg = a.range_mode == 0 && a.interp == 2 && a.use_dropoff && !a.const_weight;
  const bool exact = exactArithmetic(c);
  int rc = dispatchVps(c, [&](auto vps) {
    constexpr int V = decltype(vps)::value;
    auto launch = [&](auto zsplit) {
      constexpr int ZS = decltype(zsplit)::value;
      constexpr int G = 1;
      auto go = [&](auto kern, int wpw) {
        int grid = fuseGrid(c, reinterpret_cast<const void*>(kern), G, 64 * wpw);
        // a small explicitly allocated map (object extraction): one workgroup per wpw items is enough; the rest of the
        // persistent grid would only be launched to find an empty queue (and takes CUs from the window's own kernels)
        if (!allocate_blocks && c->explicit_blocks > 0) {
          const uint64_t items = c->explicit_blocks * c->wpb;
          const int want = static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(grid), (items + wpw - 1) / wpw));
          grid = std::max(8, (want + 7) / 8 * 8);
        }
        static bool said = false;
        if (!said && std::getenv("KHR_VERBOSE")) { said = true; std::fprintf(stderr, "[khr] k_fuse<%d,%d> %d waves / workgroup, grid %d\n", V, ZS, wpw, grid); }
        KHR_LAUNCH_TIMED(0, kern, dim3(grid), dim3(64 * wpw), a, list);
        // the items' {touched, negative} bits -> block flags (k_fuse writes one record per item instead of an atomic); left to
        // k_tracking_select when the tracking pass follows directly (khr_process_frame)
        if (defer_fold) c->fold_pending = true;
        else hipLaunchKernelGGL(k_fuse_fold, dim3((c->m.capacity + 255) / 256), dim3(256), 0, c->stream, m.blk_flags, m.blk_band,
                                &m.counters[C_MAX_SLOT], gate);
      };
      // non-default switches are test configurations: they always run the bit-exact arithmetic
      a.gate = gate;
      constexpr int WD = kUpdateWpw;
      if (defcfg && !exact) {
        go(&k_fuse<V, ZS, true, false, WD>, WD);
      } else if (defcfg) {
        go(&k_fuse<V, ZS, true, true, WD>, WD);
      } else {
        go(&k_fuse<V, ZS, false, true, WD>, WD);
      }
    };
    // a shard of a sharded map sees 1 / world of every frame's blocks: shorter z ranges per wave keep the number of
    // wave items (and with it the number of busy SIMDs) up
    const int zs = c->fuse_zsplit;
    if (V == 8) {
      launch(std::integral_constant<int, 4>());
    } else {
      if (zs == 8) launch(std::integral_constant<int, (V == 16 ? 8 : 4)>());
      else launch(std::integral_constant<int, 4>());
    }
    return KHR_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

int khr_integrate(khr_ctx* c, int slot, int allocate_blocks, int use_mask, int object_id) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const DevFrame f = makeDevFrame(c, s);
  if (object_id >= 0 && s.has_obj) {  // the object image comes from the auxiliary stream
    HIP_TRY(hipEventRecord(c->ev_aux_done, c->aux_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_aux_done, 0));
  }
  int rc = integrateAlloc(c, s, f, allocate_blocks);
  if (rc) return rc;
  return integrateUpdate(c, s, f, allocate_blocks, use_mask, object_id, false);
}

int khr_integrate_shared(khr_ctx* c, khr_ctx* src, int src_slot, int allocate_blocks, int use_mask, int object_id) {
  if (!c || !src || !validSlot(src, src_slot)) return fail(KHR_EINVAL, "bad source slot");
  if (c->device != src->device) return fail(KHR_EINVAL, "contexts live on different devices");
  HIP_TRY(hipSetDevice(c->device));
  // the frame must be complete: either the caller declared the dependency on the device (khr_depend_on) or the host waits
  if (c->dep_src != src) {
    if (c->stream != src->stream) HIP_TRY(hipStreamSynchronize(src->stream));
    HIP_TRY(hipStreamSynchronize(src->aux_stream));
  }
  FrameSlot& s = src->slots[src_slot];
  const DevFrame f = makeDevFrame(src, s);
  int rc = integrateAlloc(c, s, f, allocate_blocks);
  if (rc) return rc;
  return integrateUpdate(c, s, f, allocate_blocks, use_mask, object_id, false);
}

static int integrateSharedBatch(khr_ctx* c, khr_ctx* src, const int* src_slots, const int* object_ids, int n_frames, int allocate_blocks,
                                int use_mask, PruneRequest* prune) {
  if (!c || !src || !src_slots || n_frames < 0) return fail(KHR_EINVAL, "bad argument");
  for (int i = 0; i < n_frames; ++i)
    if (!validSlot(src, src_slots[i])) return fail(KHR_EINVAL, "bad source slot");
  if (c->device != src->device) return fail(KHR_EINVAL, "contexts live on different devices");
  if (n_frames == 0) return KHR_OK;
  if (allocate_blocks) {  // the frustum differs per frame: nothing to share
    for (int i = 0; i < n_frames; ++i) {
      const int rc = khr_integrate_shared(c, src, src_slots[i], 1, use_mask, object_ids ? object_ids[i] : -1);
      if (rc) return rc;
    }
    return KHR_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (c->dep_src != src) {
    if (c->stream != src->stream) HIP_TRY(hipStreamSynchronize(src->stream));
    HIP_TRY(hipStreamSynchronize(src->aux_stream));
  }
  // "blocks = all allocated" (updateMap(allocate = false)): one list for all frames; the integrator never allocates or
  // frees blocks, so it stays valid
  {
    FrameSlot& s0 = src->slots[src_slots[0]];
    const DevFrame f0 = makeDevFrame(src, s0);
    const int rc = integrateAlloc(c, s0, f0, 0);
    if (rc) return rc;
  }
  {
    const int rc = integrateUpdateMulti(c, src, src_slots, object_ids, n_frames, use_mask, prune);
    if (rc <= 0) return rc;  // done (or failed); 1 = not applicable: frame by frame below
  }
  for (int i = 0; i < n_frames; ++i) {
    FrameSlot& s = src->slots[src_slots[i]];
    const DevFrame f = makeDevFrame(src, s);
    const int rc = integrateUpdate(c, s, f, 0, use_mask, object_ids ? object_ids[i] : -1, false);
    if (rc) return rc;
  }
  // (statistics: cum_integrate_calls counts this batch once; the voxel counts cover all its frames)
  return KHR_OK;
}

int khr_integrate_shared_batch(khr_ctx* c, khr_ctx* src, const int* src_slots, const int* object_ids, int n_frames,
                               int allocate_blocks, int use_mask) {
  return integrateSharedBatch(c, src, src_slots, object_ids, n_frames, allocate_blocks, use_mask, nullptr);
}

static int readPruned(khr_ctx* c, int64_t* n_pruned) {
  unsigned long long np = 0;
  HIP_TRY(hipMemcpyAsync(&np, &c->m.stats[S_PRUNED], sizeof(np), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *n_pruned = static_cast<int64_t>(np);
  return KHR_OK;
}

// khr_integrate_shared_batch(allocate = 0) followed by khr_object_prune, the pruning inside the update's last launch where the batch
// runs on k_fuse_obj; every other batch is integrated as before and pruned by k_object_prune
int khr_integrate_prune_batch(khr_ctx* c, khr_ctx* src, const int* src_slots, const int* object_ids, int n_frames, int use_mask,
                              float min_confidence, float min_observations, int64_t* n_pruned) {
  PruneRequest pr{min_confidence, min_observations, false};
  const bool can_prune = c && c->cfg.with_semantics && c->p.K >= 2;  // (khr_object_prune refuses every other map, after the batch)
  const int rc = integrateSharedBatch(c, src, src_slots, object_ids, n_frames, 0, use_mask, can_prune ? &pr : nullptr);
  if (rc) return rc;
  if (!pr.fused) return khr_object_prune(c, min_confidence, min_observations, n_pruned);
  return n_pruned ? readPruned(c, n_pruned) : KHR_OK;
}

// smallest unsigned x with  double(x) / 1e9 >= T  (T = toSeconds(now) - window, reference arithmetic:
// tracking_integrator.cpp:238,250).  fl(double(x)/1e9) is non-decreasing in x, so a binary search is exact.
static uint64_t stampThreshold(double T) {
  auto sec = [](uint64_t x) { return static_cast<double>(x) / 1e9; };
  if (sec(0) >= T) return 0;
  uint64_t lo = 0, hi = ~0ull;  // sec(lo) < T; find the first x with sec(x) >= T (or ~0 if none)
  if (!(sec(hi) >= T)) return hi;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (sec(mid) >= T) hi = mid; else lo = mid;
  }
  return hi;
}

// fork_event: recorded behind k_tracking_select (nullptr: none)
static int trackingPhase(khr_ctx* c, uint64_t stamp, int phase, hipEvent_t fork_event = nullptr) {
  DevMap& m = c->m;
  const double now = static_cast<double>(stamp) / 1e9;
  const uint64_t lim_active = stampThreshold(now - c->p.temporal_window);
  const uint64_t lim_free = stampThreshold(now - c->p.temporal_buffer);
  return dispatchVps(c, [&](auto vps) {
    constexpr int V = decltype(vps)::value;
    if (phase & 1) {
      // the ever-free work list is gathered by the tracking pass itself; the two list counters alternate and each
      // pass zeroes the other one, so no memset / compaction launch is needed
      const int cur = c->ef_parity;
      c->ef_parity ^= 1;
      c->ef_cur = cur;
      uint32_t* const cnt = &m.counters[cur ? C_N_PROC2 : C_N_PROC];
      uint32_t* const cnt_next = &m.counters[cur ? C_N_PROC : C_N_PROC2];
      ScopedTimer tm(c, 1);
      // stamps going backwards void the per-block skip thresholds (they assume monotone limits)
      const int force_full = stamp < c->last_track_stamp || c->cfg.disable_culling ? 1 : 0;
      hipLaunchKernelGGL(k_tracking_select, dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m, lim_active, lim_free, force_full,
                         c->d_trk_proc, c->d_ef, cnt, cnt_next, c->fold_pending ? m.blk_band : nullptr);
      c->fold_pending = false;
      // (khr_process_frame at output cadence: marching cubes start here, beside the rest of the tracking pass)
      if (fork_event) HIP_TRY(hipEventRecord(fork_event, c->stream));
      KHR_LAUNCH_TIMED(10, (k_tracking_update<V, (V == 16 ? 4 : 1)>), dim3(V == 16 ? 4096 : 1024), dim3(256), m, c->p, stamp,
                       c->last_track_stamp, lim_active, lim_free, c->d_trk_proc, cnt);
      c->last_track_stamp = stamp;
    }
    if (phase & 2) {
      ScopedTimer tm(c, 2);
      RemoteHalo rh{};
      if (c->halo_n) {
        rh.recs = c->halo_view;
        rh.ht_keys = c->d_halo_keys;
        rh.ht_vals = c->d_halo_vals;
        rh.ht_mask = c->halo_mask;
      }
      KHR_LAUNCH_TIMED(11, (k_ever_free<V>), dim3(kStreamGrid), dim3(256), m, c->p, c->d_ef,
                       &m.counters[c->ef_cur ? C_N_EF2 : C_N_EF_A], rh);
    }
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
}

int khr_update_tracking(khr_ctx* c, uint64_t stamp) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->cfg.with_tracking) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  return trackingPhase(c, stamp, 3);
}

int khr_update_tracking_phase(khr_ctx* c, uint64_t stamp, int phase) {
  if (!c || phase < 1 || phase > 3) return fail(KHR_EINVAL, "bad argument");
  if (!c->cfg.with_tracking) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  return trackingPhase(c, stamp, phase);
}

// ---------------------------------------------------------------------------------------------
// tick path: the camera frames of one tick batched (sharded multi-camera runs).  Every rank of a
// sharded run sees every camera, so what a rank does PER CAMERA is the part that does not shrink with the number of
// ranks: one ingest launch for all cameras with the motion detector's seed test folded in, one host wait per tick,
// allocation per camera but ONE block initialisation and ONE culling launch, then the update kernels per camera.
// ---------------------------------------------------------------------------------------------
// spin on a word of pinned memory a one-workgroup publish kernel writes (the stream keeps running)
static int waitWord(khr_ctx* c, volatile uint32_t* w, uint32_t ticket, const char* what) {
  uint64_t spins = 0;
  while (*w != ticket) {
    __builtin_ia32_pause();
    if ((++spins & 0xffffu) == 0) {
      const hipError_t q = hipStreamQuery(c->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(KHR_EDEVICE, "stream failed while waiting for %s: %s", what, hipGetErrorString(q));
      if (q == hipSuccess && *w != ticket) {
        uint32_t done = 0xffffffffu;
        if (c->d_fetch_done) (void)hipMemcpy(&done, c->d_fetch_done, sizeof(done), hipMemcpyDeviceToHost);
        return fail(KHR_EDEVICE, "%s was never published (word %u, expected ticket %u, gather completion counter %u)", what, *w, ticket, done);
      }
    }
  }
  return KHR_OK;
}

static int ensureTick(khr_ctx* c) {
  if (c->d_tick_work) return KHR_OK;
  const size_t cap = c->m.capacity;
  int rc = devAlloc(c, &c->d_tick_work, cap * kMaxTick, false);
  if (!rc) rc = devAlloc(c, &c->d_tick_work4, 2 * static_cast<size_t>(c->item_cap) * kMaxTick, false);
  if (!rc) rc = devAlloc(c, &c->d_tick_counts, 6 * kMaxTick + 32);
  if (!rc) rc = devAlloc(c, &c->d_tick_seeds, kMaxTick + 32);
  if (!rc) rc = devAlloc(c, &c->d_tick_frames, kMaxTick, false);
  if (!rc) rc = devAlloc(c, &c->d_tick_mask, c->item_cap / 4 + 1);
  if (rc) return rc;
  if (c->h_tick.alloc(64)) return fail(KHR_ENOMEM, "pinned tick block");
  std::memset(c->h_tick, 0, 256);
  HIP_TRY(hipStreamSynchronize(c->stream));  // the zero-fills above
  return KHR_OK;
}

// the frame slots of a tick: nothing of the ring's state is touched unless the whole tick fits
static int acquireTickSlots(khr_ctx* c, int n_frames, int* slots_out) {
  const int ring_pos = c->next_slot;
  for (int i = 0; i < n_frames; ++i) {
    const int slot = acquireSlot(c);
    bool wrapped = false;
    for (int j = 0; j < i && slot >= 0; ++j) wrapped |= slots_out[j] == slot;  // the ring wrapped around retained slots
    if (slot < 0 || wrapped) {
      c->next_slot = ring_pos;
      return slot < 0 ? slot : fail(KHR_ENOMEM, "not enough free frame slots for a tick of %d frames (raise num_frame_slots)", n_frames);
    }
    slots_out[i] = slot;
  }
  return KHR_OK;
}
struct TickSlotsGuard {  // an error after the acquisition leaves the tick's slots unusable instead of half-written
  khr_ctx* c; const int* slots; int n; bool armed = true;
  ~TickSlotsGuard() { if (armed) for (int i = 0; i < n; ++i) c->slots[slots[i]].valid = false; }
};

// the arguments khr_tick_ingest and khr_tick_adopt share
static int tickArgs(const khr_ctx* c, const khr_sensor* sensor, const void* frames, int n_frames, const int* slots_out) {
  if (!c || !sensor || !frames || !slots_out || n_frames < 1) return fail(KHR_EINVAL, "bad argument");
  KHR_TRY(checkSensor(c, sensor));
  if (static_cast<size_t>(n_frames) > c->slots.size()) return fail(KHR_EINVAL, "more frames than frame slots (num_frame_slots)");
  return KHR_OK;
}

// ... and what they do: the tick's slots, and per batch of up to kMaxTick frames `batch(base, nb, count_seeds)` -- which turns the
// slots slots_out[base .. base + nb) into the batch's frames and queues their kernel -- followed by the seed counts' publish
static int tickFrames(khr_ctx* c, int n_frames, int count_seeds, int* slots_out, uint32_t* n_seed_pixels, int64_t* seed_counts_device,
                      const std::function<void(int, int, int)>& batch) {
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensureTick(c);
  if (rc) return rc;
  count_seeds = count_seeds && c->cfg.with_tracking;
  c->tick_seed_host.assign(n_frames, 0u);
  c->tick_seed_collected = 0;
  ScopedTimer tm(c, 6);
  if ((rc = acquireTickSlots(c, n_frames, slots_out))) return rc;
  TickSlotsGuard undo{c, slots_out, n_frames};
  for (int base = 0; base < n_frames; base += kMaxTick) {
    const int nb = std::min(kMaxTick, n_frames - base);
    batch(base, nb, count_seeds);
    if (count_seeds) {
      ++c->tick_ticket;
      if (c->tick_ticket == 0) ++c->tick_ticket;
      hipLaunchKernelGGL(k_tick_publish, dim3(1), dim3(64), 0, c->stream, c->d_tick_seeds, nb,
                         c->h_tick.dev(), c->h_tick.dev() + 32, c->tick_ticket,
                         seed_counts_device ? reinterpret_cast<long long*>(seed_counts_device) + base : nullptr);
    }
    HIP_TRY(hipGetLastError());
    // one result block: a tick of one batch may be collected later (khr_tick_seed_counts), more batches are collected
    // as they go
    if (count_seeds && (n_seed_pixels || n_frames > kMaxTick)) {
      rc = waitWord(c, &c->h_tick[32], c->tick_ticket, "tick seed counts");
      if (rc) return rc;
      for (int k = 0; k < nb; ++k) c->tick_seed_host[base + k] = c->h_tick[k];
      c->tick_seed_collected = base + nb;
    }
  }
  c->tick_seed_n = count_seeds ? n_frames : 0;
  if (count_seeds && n_seed_pixels) std::memcpy(n_seed_pixels, c->tick_seed_host.data(), sizeof(uint32_t) * n_frames);
  if (!count_seeds && n_seed_pixels) std::memset(n_seed_pixels, 0, sizeof(uint32_t) * n_frames);
  if (!count_seeds && seed_counts_device) HIP_TRY(hipMemsetAsync(seed_counts_device, 0, sizeof(int64_t) * n_frames, c->stream));
  c->begun = false;
  undo.armed = false;
  return KHR_OK;
}

int khr_tick_ingest(khr_ctx* c, const khr_sensor* sensor, const khr_frame* frames, int n_frames, int count_seeds,
                    int* slots_out, uint32_t* n_seed_pixels, int64_t* seed_counts_device) {
  KHR_TRY(tickArgs(c, sensor, frames, n_frames, slots_out));
  for (int i = 0; i < n_frames; ++i)
    if (!frames[i].depth) return fail(KHR_EINVAL, "frame %d has no depth image", i);
  return tickFrames(c, n_frames, count_seeds, slots_out, n_seed_pixels, seed_counts_device, [&](int base, int nb, int seeds) {
    TickIngest t{};
    int tw = 0, th = 0;
    for (int k = 0; k < nb; ++k) {
      const khr_frame& fr = frames[base + k];
      FrameSlot& s = newFrameSlot(c, slots_out[base + k], *sensor, fr, fr.color != nullptr, fr.label != nullptr, true);
      tw = s.tw, th = s.th;
      t.depth_in[k] = fr.depth; t.rgb_in[k] = fr.color; t.label_in[k] = fr.label;
      t.depth[k] = s.depth; t.range[k] = s.range; t.rgba[k] = s.rgba; t.label[k] = s.label; t.dyn[k] = s.dyn;
      t.tile_max[k] = s.tile_max;
      float R[9], tt[3];
      makePose(fr.world_T_sensor, R, tt, t.Rw[k], t.tw[k]);
      t.min_z_world[k] = static_cast<float>(fr.world_T_sensor[11] + static_cast<double>(c->cfg.md_min_z_coordinate));
    }
    hipLaunchKernelGGL(k_tick_ingest, dim3(tw * th, nb), dim3(256), 0, c->stream, t, tw, sensor->width, sensor->height, sensor->fx,
                       sensor->fy, sensor->cx, sensor->cy, c->p.range_mode, c->m, c->p, c->cfg.md_max_range, seeds ? 1 : 0,
                       c->d_tick_seeds);
  });
}

// ---- sender-side ingest: converted planes travel, not raw frames -------------------------------------------------------
static uint32_t convertedTilesPadded(const khr_sensor* s) {
  const uint32_t tiles = static_cast<uint32_t>(((s->width + kTile - 1) / kTile) * ((s->height + kTile - 1) / kTile));
  return (tiles + 63u) / 64u * 64u;
}

size_t khr_converted_bytes(const khr_sensor* sensor, int with_depth) {
  if (!sensor || sensor->width < 2 || sensor->height < 2) return 0;
  const size_t n = static_cast<size_t>(sensor->width) * sensor->height;
  return 4 * ((with_depth ? 4 : 3) * n + convertedTilesPadded(sensor));
}

int khr_converted_views(const khr_sensor* sensor, const void* packed_device, int with_depth, khr_converted_frame* out) {
  if (!sensor || !packed_device || !out) return fail(KHR_EINVAL, "null argument");
  const size_t n = static_cast<size_t>(sensor->width) * sensor->height;
  const uint32_t* w = static_cast<const uint32_t*>(packed_device);
  out->range = reinterpret_cast<const float*>(w);
  out->rgba = w + n;
  out->label = reinterpret_cast<const int32_t*>(w + 2 * n);
  out->tile_max = reinterpret_cast<const float*>(w + 3 * n);
  out->depth = with_depth ? reinterpret_cast<const float*>(w + 3 * n + convertedTilesPadded(sensor)) : nullptr;
  return KHR_OK;
}

int khr_export_converted(khr_ctx* c, int slot, void* packed_device, int with_depth) {
  if (!c || !packed_device || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  HIP_TRY(hipSetDevice(c->device));
  const FrameSlot& s = c->slots[slot];
  const uint32_t n = static_cast<uint32_t>(s.sensor.width) * static_cast<uint32_t>(s.sensor.height);
  hipLaunchKernelGGL(k_pack_converted, dim3(1024), dim3(256), 0, c->stream, s.vRange(), s.has_color ? s.vRgba() : nullptr,
                     s.has_label ? s.vLabel() : nullptr, s.vTileMax(), with_depth ? s.vDepth() : nullptr, n,
                     static_cast<uint32_t>(s.tw * s.th), convertedTilesPadded(&s.sensor), static_cast<uint32_t*>(packed_device));
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

int khr_tick_adopt(khr_ctx* c, const khr_sensor* sensor, const khr_converted_frame* frames, int n_frames, int count_seeds,
                   int* slots_out, uint32_t* n_seed_pixels, int64_t* seed_counts_device) {
  KHR_TRY(tickArgs(c, sensor, frames, n_frames, slots_out));
  for (int i = 0; i < n_frames; ++i) {
    if (!frames[i].range || !frames[i].tile_max) return fail(KHR_EINVAL, "frame %d has no range image / range tiles", i);
    if (!frames[i].depth && c->p.range_mode != 0)
      return fail(KHR_EINVAL, "frame %d has no depth plane (only with range_mode 0 is depth == range where it is read)", i);
  }
  // slots adopted by an EARLIER tick refer to planes in a receive buffer the caller is about to reuse: they
  // stop being readable here, instead of silently mixing the new tick's planes with the old tick's meta data
  for (FrameSlot& old : c->slots)
    if (old.x_range != nullptr) old.valid = false;
  const size_t n = static_cast<size_t>(sensor->width) * sensor->height;
  return tickFrames(c, n_frames, count_seeds, slots_out, n_seed_pixels, seed_counts_device, [&](int base, int nb, int seeds) {
    TickAdopt t{};
    for (int k = 0; k < nb; ++k) {
      const khr_converted_frame& fr = frames[base + k];
      khr_frame meta{};
      meta.timestamp_ns = fr.timestamp_ns;
      std::memcpy(meta.world_T_sensor, fr.world_T_sensor, sizeof(meta.world_T_sensor));
      FrameSlot& s = newFrameSlot(c, slots_out[base + k], *sensor, meta, fr.rgba != nullptr, fr.label != nullptr, true);
      s.x_range = fr.range;
      s.x_depth = fr.depth ? fr.depth : fr.range;
      s.x_rgba = fr.rgba;
      s.x_label = fr.label;
      s.x_tile_max = fr.tile_max;
      t.range[k] = fr.range;
      t.depth[k] = fr.depth;
      t.dyn[k] = s.dyn;
      float R[9], tt[3];
      makePose(fr.world_T_sensor, R, tt, t.Rw[k], t.tw[k]);
      t.min_z_world[k] = static_cast<float>(fr.world_T_sensor[11] + static_cast<double>(c->cfg.md_min_z_coordinate));
    }
    hipLaunchKernelGGL(k_tick_adopt, dim3(gridFor(n), nb), dim3(256), 0, c->stream, t, sensor->width, sensor->height, sensor->fx,
                       sensor->fy, sensor->cx, sensor->cy, c->m, c->p, c->cfg.md_max_range, seeds ? 1 : 0, c->d_tick_seeds);
  });
}

int khr_tick_seed_counts(khr_ctx* c, uint32_t* n_seed_pixels, int n_frames) {
  if (!c || !n_seed_pixels || n_frames < 0) return fail(KHR_EINVAL, "bad argument");
  if (n_frames > static_cast<int>(c->tick_seed_host.size())) return fail(KHR_ESTATE, "no khr_tick_ingest of that many frames");
  if (c->tick_seed_n && c->tick_seed_collected < c->tick_seed_n) {  // the last batch's block has not been read yet
    const int rc = waitWord(c, &c->h_tick[32], c->tick_ticket, "tick seed counts");
    if (rc) return rc;
    for (int k = 0; k < c->tick_seed_n; ++k) c->tick_seed_host[k] = c->h_tick[k];
    c->tick_seed_collected = c->tick_seed_n;
  }
  std::memcpy(n_seed_pixels, c->tick_seed_host.data(), sizeof(uint32_t) * n_frames);
  return KHR_OK;
}

// The cameras of a tick in ONE update launch (k_fuse2 over the union of their item lists, a camera mask per item)
// instead of one launch per camera: taken for the block shapes and switches k_fuse2 is instantiated for.
static bool tickUnion(const khr_ctx* c) {
  const DevParams& p = c->p;
  const bool defcfg = p.range_mode == 0 && p.interp == 2 && p.use_dropoff && !p.const_weight;
  if (!defcfg) return false;
  return c->cfg.voxels_per_side == 8 || (c->cfg.voxels_per_side == 16 && exactArithmetic(c));
}

static int tickUpdateUnion(khr_ctx* c, const int* slots, const DevFrame* frames, int nb, int use_mask, int object_id) {
  FuseArgs a{};
  fillFuseMap(c, &a);
  FuseFrameSet set{};
  for (int k = 0; k < nb; ++k) fillFuseFrame(c, c->slots[slots[k]], frames[k], use_mask, object_id, &set.f[k]);
  hipLaunchKernelGGL(k_put_frames, dim3(1), dim3(256), 0, c->stream, set, c->d_tick_frames, nb);
  static_cast<FuseFrame&>(a) = set.f[0];
  a.frames = c->d_tick_frames;
  a.n_frames = nb;
  a.item_mask = reinterpret_cast<uint8_t*>(c->d_tick_mask);
  FuseList list{c->d_tick_work4, c->d_tick_work4 + c->item_cap, c->item_cap, &c->d_tick_counts[2 * kMaxTick]};
  auto go = [&](auto kern, int wpw) {
    const int grid = fuse2Grid(c, reinterpret_cast<const void*>(kern), wpw);
    KHR_LAUNCH_TIMED(0, kern, dim3(grid), dim3(64 * wpw), a, list);
  };
  if (c->cfg.voxels_per_side == 8) {
    if (exactArithmetic(c)) go(&k_fuse2<8, 4, true, 8, 4>, 8);
    else go(&k_fuse2<8, 4, false, 8, 4>, 8);
  } else if (c->fuse_zsplit == 8) {
    go(&k_fuse2<16, 8, true, 16, 4>, 16);
  } else {
    go(&k_fuse2<16, 4, true, 16, 4>, 16);
  }
  c->tick_mask_dirty = false;
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

int khr_tick_integrate(khr_ctx* c, const int* slots, int n_frames, int use_mask, int object_id, int phases) {
  if (!c || !slots || n_frames < 1 || (phases & 15) == 0) return fail(KHR_EINVAL, "bad argument");
  if (phases & 1) phases |= 12;  // bit 0 = allocation (bit 2) + initialisation / culling (bit 3)
  if ((phases & 14) != 14 && n_frames > kMaxTick) return fail(KHR_EINVAL, "split phases take at most %d frames", kMaxTick);
  for (int i = 0; i < n_frames; ++i) {
    if (!validSlot(c, slots[i])) return fail(KHR_EINVAL, "bad slot");
    const khr_sensor &a = c->slots[slots[i]].sensor, &b = c->slots[slots[0]].sensor;
    if (a.width != b.width || a.height != b.height) return fail(KHR_EINVAL, "the frames of a tick must come from sensors of one image size");
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensureTick(c);
  if (rc) return rc;
  DevMap& m = c->m;
  const uint32_t cap = m.capacity;
  const bool one_launch = tickUnion(c);
  for (int base = 0; base < n_frames; base += kMaxTick) {
    const int nb = std::min(kMaxTick, n_frames - base);
    TickFrames t{};
    for (int k = 0; k < nb; ++k) {
      FrameSlot& s = c->slots[slots[base + k]];
      t.f[k] = makeDevFrame(c, s);
      t.tile_max[k] = s.vTileMax();
    }
    if (phases & 4) {
      if (++c->tick_epoch <= 0) c->tick_epoch = 1;
      c->motion_ignore_epoch = c->tick_epoch;
      if (std::getenv("KHR_DEBUG_TICK_NO_EPOCH")) c->motion_ignore_epoch = 0;  // test hook: shows that the epoch matters
      hipLaunchKernelGGL(k_tick_begin, dim3(1), dim3(256), 0, c->stream, m, c->p.nvox, c->d_wg_stats, c->d_tick_counts,
                         static_cast<uint32_t>(nb - 1));
      c->begun = false;
      ScopedTimer tm(c, 3);
      // one allocation launch over the bounding lattice of the cameras' candidate cubes when that box is not much larger
      // than the cubes themselves (a rig: cameras around one centre); otherwise camera by camera
      TickFrusta tf{};
      int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
      size_t cubes = 0;
      for (int k = 0; k < nb; ++k) {
        const DevFrustum fr = makeFrustum(c, t.f[k]);
        tf.fr[k] = fr;
        std::memcpy(tf.R[k], t.f[k].R, sizeof(tf.R[k]));
        std::memcpy(tf.t[k], t.f[k].t, sizeof(tf.t[k]));
        tf.max_range[k] = t.f[k].max_range;
        const int bc[3] = {fr.bc.x, fr.bc.y, fr.bc.z};
        for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], bc[a] - fr.n_steps), hi[a] = std::max(hi[a], bc[a] + fr.n_steps);
        const size_t S = static_cast<size_t>(2 * fr.n_steps + 1);
        cubes += S * S * S;
      }
      const size_t box = static_cast<size_t>(hi[0] - lo[0] + 1) * static_cast<size_t>(hi[1] - lo[1] + 1) * static_cast<size_t>(hi[2] - lo[2] + 1);
      if (nb > 1 && box <= cubes && box < (1ull << 31)) {
        hipLaunchKernelGGL(k_tick_alloc, dim3(static_cast<unsigned>((box + kTickAllocThreads - 1) / kTickAllocThreads)), dim3(kTickAllocThreads), 0, c->stream, m, c->p, tf, nb, make_int3(lo[0], lo[1], lo[2]),
                           make_int3(hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1), c->d_tick_work, cap, c->d_new,
                           c->d_tick_counts, c->motion_ignore_epoch);
      } else {
        for (int k = 0; k < nb; ++k) {
          const int S = 2 * tf.fr[k].n_steps + 1;
          const size_t total = static_cast<size_t>(S) * S * S;
          hipLaunchKernelGGL(k_alloc_visible, dim3(gridFor(total)), dim3(256), 0, c->stream, m, c->p, t.f[k], tf.fr[k],
                             c->d_tick_work + static_cast<size_t>(k) * cap, c->d_new, c->h_pinned.dev() + 2, 0u, &c->d_tick_counts[2 * k],
                             c->motion_ignore_epoch);
        }
      }
      HIP_TRY(hipGetLastError());
    }
    if (phases & 8) {
      ScopedTimer tm(c, 3);
      hipLaunchKernelGGL(k_init_blocks, dim3(2048), dim3(256), 0, c->stream, m, c->p, c->d_new);
      const FrameSlot& s0 = c->slots[slots[base]];
      if (one_launch && c->tick_mask_dirty)  // a first phase whose second phase never ran left camera bits behind
        HIP_TRY(hipMemsetAsync(c->d_tick_mask, 0, sizeof(uint32_t) * (c->item_cap / 4 + 1), c->stream));
      c->tick_mask_dirty = one_launch;
      hipLaunchKernelGGL(k_tick_cull, dim3(256, nb), dim3(256), 0, c->stream, m, c->p, t, c->d_tick_work, cap, c->d_tick_work4, c->item_cap, c->wpb,
                         c->d_tick_counts, c->cfg.disable_culling ? 0 : 1, s0.tw, s0.th, one_launch ? c->d_tick_mask : nullptr);
      c->host_index_valid = false, ++c->map_gen;
      HIP_TRY(hipGetLastError());
    }
    if ((phases & 2) && one_launch) {
      rc = tickUpdateUnion(c, slots + base, t.f, nb, use_mask, object_id);
      if (rc) return rc;
    }
    for (int k = 0; k < nb && (phases & 2) && !one_launch; ++k) {
      FrameSlot& s = c->slots[slots[base + k]];
      UpdateLists lists;
      lists.list = FuseList{c->d_tick_work4 + static_cast<size_t>(2 * k) * c->item_cap, c->d_tick_work4 + static_cast<size_t>(2 * k + 1) * c->item_cap,
                            c->item_cap, &c->d_tick_counts[2 * kMaxTick + 4 * k]};
      rc = integrateUpdate(c, s, t.f[k], 1, use_mask, object_id, false, &lists);
      if (rc) return rc;
    }
    if (phases & 2) c->motion_ignore_epoch = 0;
  }
  return KHR_OK;
}

int khr_tick_live_bound(khr_ctx* c, int64_t* out_device, int n_out, int index) {
  if (!c || !out_device || n_out < 1 || index < 0 || index >= n_out) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_live_bound, dim3(1), dim3(64), 0, c->stream, c->m, out_device, n_out, index);
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

int khr_export_halo(khr_ctx* c, void* records, int64_t cap_records, int on_device) {
  if (!c || !records || cap_records < 1) return fail(KHR_EINVAL, "bad argument");
  if (!c->cfg.with_tracking) return fail(KHR_ESTATE, "halo records need the tracking layer");
  HIP_TRY(hipSetDevice(c->device));
  DevMap& m = c->m;
  const size_t bytes = static_cast<size_t>(cap_records) * kHaloRecWords * sizeof(uint64_t);
  uint64_t* dst = static_cast<uint64_t*>(records);
  DevTemp holder;
  uint64_t* tmp = nullptr;
  if (!on_device) {
    KHR_TRY(holder.alloc(bytes));
    dst = tmp = holder.as<uint64_t>();
  }
  HIP_TRY(hipMemsetAsync(c->d_mesh_nwork + 1, 0, sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_list_live, dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m, c->d_work, c->d_mesh_nwork + 1, 0u);
  int rc = dispatchVps(c, [&](auto vps) {
    hipLaunchKernelGGL((k_export_halo<decltype(vps)::value>), dim3(1024), dim3(256), 0, c->stream, m, c->d_work,
                       c->d_mesh_nwork + 1, dst, static_cast<uint32_t>(cap_records));
    return KHR_OK;
  });
  if (rc == KHR_OK && !on_device) {
    hipError_t e = hipMemcpyAsync(records, tmp, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(KHR_EDEVICE, "halo export copy failed: %s", hipGetErrorString(e));
  }
  return rc;
}

int khr_import_halo(khr_ctx* c, const void* records, int64_t n_records, int on_device) {
  if (!c || (!records && n_records > 0) || n_records < 0) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  if (n_records == 0) {
    c->halo_n = 0;
    return KHR_OK;
  }
  // the index of this import: 4 slots per record (a caller that ships fewer records than its buffers hold -- the trimmed
  // all-gather of the sharded tick -- also clears and probes a smaller table)
  uint32_t ht = 1;
  while (ht < static_cast<uint64_t>(n_records) * 4) ht <<= 1;
  if (static_cast<uint64_t>(n_records) > c->halo_cap_total) {  // (re)allocate the remote table
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->halo_cap_total = 0;
    c->d_halo_keys.reset(), c->d_halo_vals.reset();  // (both go before either comes back)
    KHR_TRY(c->d_halo_keys.alloc(ht));
    KHR_TRY(c->d_halo_vals.alloc(ht));
    c->halo_cap_total = static_cast<uint32_t>(n_records);
  }
  // the staging copy of the records exists only for host-side callers (on_device imports use the caller's buffer in place:
  // the RCCL tick pre-sizes the table with world x halo_cap records and would otherwise pin hundreds of MB it never reads)
  if (!on_device && static_cast<size_t>(n_records) * kHaloRecWords > c->d_halo_recs.count()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    KHR_TRY(c->d_halo_recs.reserve(static_cast<size_t>(n_records) * kHaloRecWords));
  }
  c->halo_mask = ht - 1;
  // device records are used where they lie (the caller keeps the buffer until the next khr_update_tracking_phase(.., 2)
  // has been queued: stream order does the rest); host records are staged
  if (on_device) {
    c->halo_view = static_cast<const uint64_t*>(records);
  } else {
    HIP_TRY(hipMemcpyAsync(c->d_halo_recs, records, static_cast<size_t>(n_records) * kHaloRecWords * sizeof(uint64_t),
                           hipMemcpyHostToDevice, c->stream));
    c->halo_view = c->d_halo_recs;
  }
  HIP_TRY(hipMemsetAsync(c->d_halo_keys, 0xff, sizeof(uint64_t) * (static_cast<size_t>(c->halo_mask) + 1), c->stream));
  hipLaunchKernelGGL(k_import_halo, dim3(gridFor(n_records)), dim3(256), 0, c->stream, c->halo_view,
                     static_cast<uint32_t>(n_records), c->cfg.rank, c->cfg.world_size, c->d_halo_keys, c->d_halo_vals, c->halo_mask);
  HIP_TRY(hipGetLastError());
  if (!on_device) HIP_TRY(hipStreamSynchronize(c->stream));
  c->halo_n = static_cast<uint32_t>(n_records);
  return KHR_OK;
}

// ---------------------------------------------------------------------------------------------
// motion detection: device pixel pass + sort / run-length encode, host graph walk, device paint
// ---------------------------------------------------------------------------------------------
// motion detection, part 1: per-pixel pass; the seed-pixel count travels to pinned host memory
// asynchronously so that other kernels can be queued behind it before the host has to look at it
static int motionLaunch(khr_ctx* c, FrameSlot& s, bool fresh_slot, bool do_begin = false) {
  const size_t n = static_cast<size_t>(s.sensor.width) * s.sensor.height;
  if (!fresh_slot) {  // a slot that was just ingested already has a zero dynamic image and seed counter
    if (!s.dyn_clean) HIP_TRY(hipMemsetAsync(s.dyn, 0, n * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(&c->m.counters[C_N_SEEDS], 0, sizeof(uint32_t), c->stream));
  }
  c->stats.n_seeds = 0;
  c->h_pinned[0] = 0;
  c->seed_by_ticket = false;
  if (!c->cfg.with_tracking) return KHR_OK;
  DevMap& m = c->m;
  const DevFrame f = makeDevFrame(c, s);
  // free_space_motion_detector.cpp:80
  const float min_z_world = static_cast<float>(s.meta.world_T_sensor[11] + static_cast<double>(c->cfg.md_min_z_coordinate));
  {
    ScopedTimer tm(c, 4);
    ++c->seed_ticket;
    if (c->seed_ticket == 0) ++c->seed_ticket;
    hipLaunchKernelGGL(k_motion_pixels, dim3(gridFor(n)), dim3(256), 0, c->stream, m, c->p, f, c->cfg.md_max_range,
                       min_z_world, c->d_keys, c->motion_ignore_epoch, do_begin ? c->d_wg_stats : nullptr);
    if (do_begin) c->begun = true;
  }
  HIP_TRY(hipGetLastError());
  c->seed_by_ticket = true;
  c->seed_publish_pending = true;  // the next kernel in the stream (k_alloc_visible or k_publish_seed) writes it to the host
  return KHR_OK;
}

// motion detection, part 2: wait for the seed count; without seeds there are no clusters
// (clusterDynamicVoxels loops over seeds only); otherwise sort / run-length encode the pixel keys,
// walk the seed graph on the host and paint the dynamic image.  Returns the number of clusters.
// the seed-pixel count of the latest pixel pass: either the ticket k_motion_pixels' last workgroup writes into pinned
// memory (spin; the stream keeps running), or the event behind the asynchronous copy of the key-import path
// the wait's watchdog: duration of every wait into a histogram; a wait of more than 0.5 ms also leaves the state of the context's
// queues at the moment the count arrived (the "one run in ten" late seed count)
static void seedWaitDone(khr_ctx* c, std::chrono::steady_clock::time_point t0, bool event_path) {
  const uint64_t us = static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
  ++c->n_seed_waits;
  c->seed_wait_max_us = std::max(c->seed_wait_max_us, us);
  static const uint64_t edge[7] = {50, 100, 200, 500, 1000, 2000, 5000};
  int b = 0;
  while (b < 7 && us >= edge[b]) ++b;
  ++c->seed_wait_hist[b];
  if (us > 500) {
    ++c->n_seed_waits_late;
    c->seed_wait_late_us = us;
    c->seed_wait_late_frame = c->n_seed_waits;
    uint64_t st = 0;
    if (hipStreamQuery(c->stream) == hipErrorNotReady) st |= 1u;
    if (c->aux_stream && hipStreamQuery(c->aux_stream) == hipErrorNotReady) st |= 2u;
    if (c->h2d_stream && hipStreamQuery(c->h2d_stream) == hipErrorNotReady) st |= 4u;
    if (c->last_ingest_on_aux) st |= 8u;
    if (event_path) st |= 16u;
    st |= static_cast<uint64_t>(c->ahead_q.size()) << 8;
    c->seed_wait_late_state = st;
  }
}

static int waitSeedCount(khr_ctx* c) {
  const auto t_wait0 = std::chrono::steady_clock::now();
  if (!c->seed_by_ticket) {
    HIP_TRY(hipEventSynchronize(c->ev_seed));
    seedWaitDone(c, t_wait0, true);
    return KHR_OK;
  }
  if (c->seed_publish_pending) {
    hipLaunchKernelGGL(k_publish_seed, dim3(1), dim3(1), 0, c->stream, c->m, c->h_pinned.dev() + 2, c->seed_ticket);
    HIP_TRY(hipGetLastError());
    c->seed_publish_pending = false;
  }
  volatile uint32_t* hp = c->h_pinned;
  uint64_t spins = 0;
  while (hp[3] != c->seed_ticket) {
    __builtin_ia32_pause();
    if ((++spins & 0xffffu) == 0) {  // every ~65k polls: is the stream still alive?
      const hipError_t q = hipStreamQuery(c->stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(KHR_EDEVICE, "stream failed while waiting for the seed count: %s", hipGetErrorString(q));
      if (q == hipSuccess && hp[3] != c->seed_ticket) return fail(KHR_EDEVICE, "seed count was never published");
    }
  }
  c->h_pinned[0] = hp[2];
  seedWaitDone(c, t_wait0, false);
  return KHR_OK;
}

// spin on a ticket word in pinned memory (written by k_publish); keeps an eye on the stream so that a failed launch
// cannot hang the host
static int waitTicket(khr_ctx* c, int word, uint32_t ticket, const char* what, hipStream_t stream = nullptr) {
  volatile uint32_t* hp = c->h_pinned;
  uint64_t spins = 0;
  if (!stream) stream = c->stream;
  while (hp[word] != ticket) {
    __builtin_ia32_pause();
    if ((++spins & 0xffffu) == 0) {
      const hipError_t q = hipStreamQuery(stream);
      if (q != hipSuccess && q != hipErrorNotReady) return fail(KHR_EDEVICE, "stream failed while waiting for %s: %s", what, hipGetErrorString(q));
      if (q == hipSuccess && hp[word] != ticket) return fail(KHR_EDEVICE, "%s was never published", what);
    }
  }
  return KHR_OK;
}

// per-cluster summaries (pixel count, AABB, vertex sum) of the freshly painted dynamic image, queued behind the paint pass
// and published to pinned memory; khr_get_dynamic_clusters only has to wait for the ticket
static int clusterSummaryLaunch(khr_ctx* c, FrameSlot& s, int max_id) {
  const int tiles = ((s.sensor.width + kAccTile - 1) / kAccTile) * ((s.sensor.height + kAccTile - 1) / kAccTile);
  hipLaunchKernelGGL(k_cluster_summary, dim3(tiles), dim3(1024), 0, c->stream, makeDevFrame(c, s), s.dyn, c->d_md_acc,
                     s.dynw_valid ? static_cast<const uint8_t*>(s.dynw) : nullptr);
  if (++c->md_acc_ticket == 0) ++c->md_acc_ticket;
  hipLaunchKernelGGL(k_publish_cluster_acc, dim3(1), dim3(256), 0, c->stream, c->d_md_acc, reinterpret_cast<uint32_t*>(c->h_md_acc_pinned.dev()),
                     static_cast<uint32_t>(std::min(max_id + 1, 256)), c->h_pinned.dev() + 7, c->md_acc_ticket);
  HIP_TRY(hipGetLastError());
  c->md_acc_slot = static_cast<int>(&s - c->slots.data());
  return KHR_OK;
}

// ---- motion detector: the frame finish, the one place where host and device meet on the frame path; stages as motionFinish calls
// them.  What the host decides (cluster order, merge groups, size filter, ids, the seed-graph walk) is in khr_md_host.h, free of HIP.
// Test and A/B hooks, read once per call: tests flip them inside one process (KHR_MD_HOST_WALK / KHR_MD_LDS_MAX: khr_create).
struct MdHooks {
  bool no_device_merge, no_predict, no_prelaunch;
  uint32_t table_log2, prelaunch_px;  // 0 = not set
};
static MdHooks mdHooks() {
  static const bool no_device_merge = std::getenv("KHR_MD_NO_DEVICE_MERGE") != nullptr;  // the host walk decides the merges (once per process)
  MdHooks h{};
  h.no_device_merge = no_device_merge;
  h.no_predict = std::getenv("KHR_MD_NO_PREDICT") != nullptr;      // the lock-free component kernels only after a repeat
  h.no_prelaunch = std::getenv("KHR_MD_NO_PRELAUNCH") != nullptr;  // no chain queued ahead of the seed count
  if (const char* e = std::getenv("KHR_MD_TABLE_LOG2")) h.table_log2 = static_cast<uint32_t>(std::min(30, std::max(4, std::atoi(e))));  // forces the repeat
  if (const char* e = std::getenv("KHR_MD_PRELAUNCH_PX")) h.prelaunch_px = static_cast<uint32_t>(std::max(1, std::atoi(e)));  // a bound that is exceeded
  return h;
}

// A frame that follows a seed frame gets its chain queued BEFORE the host has seen its seed count (mdRunChain), and
// khr_process_frame, which expects seeds then, does not speculate the update kernel: both ask here.
static bool mdQueuesAhead(const khr_ctx* c, const MdHooks& hooks) { return c->md_seed_run && c->seed_by_ticket && !hooks.no_prelaunch; }

// Table size (as a mask) for a seed-pixel count.  The allocation covers the worst case (every pixel its own voxel: 2 M slots at 720p),
// and the clear and the two compaction passes walk the whole table; a seed frame has ~20 pixels per seed voxel, so the optimistic size
// is 2 slots per seed PIXEL (the seed table can then never fill up).  The near / boundary tables (<= nn entries per seed voxel) may: the
// near table switches itself to direct mode on the device, a full boundary table raises the overflow flag and the frame is repeated.
static uint32_t mdMaskFor(const khr_ctx* c, const MdHooks& hooks, uint32_t seed_pixels) {
  uint32_t ts = 1u << 14;
  while (ts < 2ull * std::max<uint32_t>(seed_pixels, 1u) && ts - 1 < c->md_mask) ts <<= 1;
  if (hooks.table_log2) ts = 1u << hooks.table_log2;
  return std::min(ts - 1, c->md_mask);
}

struct MdTables { VoxTable seeds, bnd, near; };  // the views of the voxel tables a chain worked on
struct MdHead { uint32_t S, B, R, overflow; };   // seed voxels, boundary voxels, components, "a table filled up"
// the chain up to the component records, sized for `seed_pixels` seed pixels (the kernels take the counts themselves from device
// memory); *t = the table views it used.  device_merge: also mergeClusters' overlap rows (0 < separation <= 2 voxels: the voxel
// pairs mergeClusters tests are within each other's 27-neighbourhood -- the device can answer)
static int mdLaunchChain(khr_ctx* c, int n, uint32_t seed_pixels, uint32_t mask, bool global_components, bool device_merge, MdTables* t) {
  const uint32_t cap = c->md_list_cap;
  const int nn = c->cfg.md_neighbor_connectivity;
  CompAcc* d_comp_out = reinterpret_cast<CompAcc*>(reinterpret_cast<uint8_t*>(c->d_md_n) + 16);
  const uint32_t seed_px = std::min<uint32_t>(seed_pixels, cap);  // #seed voxels <= #seed pixels
  const size_t tsize = static_cast<size_t>(mask) + 1;
  const VoxTable seeds = t->seeds = VoxTable{c->d_md_keys, c->d_md_counts, c->d_md_ids, mask};
  const VoxTable bnd = t->bnd = VoxTable{c->d_md_keys + tsize, c->d_md_counts + tsize, c->d_md_ids + tsize, mask};
  const VoxTable near = t->near = VoxTable{c->d_md_keys + 2 * tsize, c->d_md_counts + 2 * tsize, c->d_md_ids + 2 * tsize, mask};
  int32_t* const d_box = reinterpret_cast<int32_t*>(c->d_md_scratch4) + 8;  // [0..5] seed voxel box, [6] direct mode, [7] edge count
  hipLaunchKernelGGL(k_md_clear, dim3(1024), dim3(256), 0, c->stream, c->d_md_keys, c->d_md_counts, static_cast<uint32_t>(tsize), c->d_md_n, d_box);
  hipLaunchKernelGGL(k_md_seed_insert, dim3(gridFor(n)), dim3(256), 0, c->stream, c->d_keys, n, seeds, c->d_md_n + 3);
  hipLaunchKernelGGL(k_md_compact, dim3(gridFor(tsize)), dim3(256), 0, c->stream, seeds, c->d_md_seed_keys, c->d_md_seed_counts, c->d_md_n, cap, nullptr);
  // (whether the `near` table can hold nn entries per seed voxel is decided on the device, which knows the voxel count)
  hipLaunchKernelGGL(k_md_near_insert, dim3(256), dim3(256), 0, c->stream, c->d_md_seed_keys, c->d_md_n, cap, nn, near, c->d_md_n + 3, d_box);
  hipLaunchKernelGGL(k_md_boundary_insert, dim3(gridFor(n)), dim3(256), 0, c->stream, c->d_keys, n, near, bnd, seeds, nn, 0, d_box, c->d_md_n + 3);
  hipLaunchKernelGGL(k_md_compact, dim3(gridFor(tsize)), dim3(256), 0, c->stream, bnd, c->d_md_bnd_keys, c->d_md_bnd_counts,
                     c->d_md_n + 1, cap, c->d_md_bnd_final, c->d_md_bnd_deg, c->d_md_bnd_mask);
  uint32_t* const d_n_edges = c->d_md_scratch4 + 15;
  hipLaunchKernelGGL(k_md_adjacency, dim3(1024), dim3(256), 0, c->stream, c->d_md_seed_keys, c->d_md_n, seeds, bnd, nn, cap,
                     c->d_md_adj, c->d_md_edges, cap, d_n_edges);  // (room for `cap` edges)
  // connected components of the seed graph + their order-free summaries, on the device
  hipLaunchKernelGGL(k_md_comp_lds, dim3(1), dim3(1024), 0, c->stream, c->d_md_adj, c->d_md_n, cap, nn, c->d_md_parent, c->d_md_comp_acc,
                     c->md_lds_max, c->d_md_edges, cap, d_n_edges, (c->p.dbg & 16) ? c->d_dbg : nullptr);
  if (global_components) {
    hipLaunchKernelGGL(k_md_comp_init, dim3(64), dim3(256), 0, c->stream, c->d_md_adj, c->d_md_n, cap, nn, c->d_md_parent, c->d_md_comp_acc,
                       c->md_lds_max);
    hipLaunchKernelGGL(k_md_comp_jump, dim3(64), dim3(256), 0, c->stream, c->d_md_n, cap, c->d_md_parent, c->md_lds_max);
    hipLaunchKernelGGL(k_md_comp_union, dim3(1024), dim3(256), 0, c->stream, c->d_md_adj, c->d_md_n, cap, nn, c->d_md_parent, c->md_lds_max);
  }
  hipLaunchKernelGGL(k_md_comp_reduce, dim3(gridFor(seed_px)), dim3(256), 0, c->stream, c->d_md_seed_keys, c->d_md_seed_counts,
                     c->d_md_bnd_keys, c->d_md_bnd_counts, c->d_md_adj, c->d_md_n, cap, nn, c->d_md_parent, c->d_md_comp_acc);
  hipLaunchKernelGGL(k_md_comp_roots, dim3(gridFor(seed_px)), dim3(256), 0, c->stream, c->d_md_n, cap, c->d_md_parent, c->d_md_comp_acc,
                     c->d_md_rootidx, c->d_md_n + 2, d_comp_out, kCompCap);
  // mergeClusters' overlap rows (<= 64 components, separation <= 2 voxels; both kernels leave at once when there is one component)
  if (device_merge) {
    hipLaunchKernelGGL(k_md_bnd_comps, dim3(256), dim3(256), 0, c->stream, c->d_md_bnd_keys, c->d_md_n, cap, nn, seeds, c->d_md_parent,
                       c->d_md_rootidx, c->d_md_bnd_mask);
    hipLaunchKernelGGL(k_md_comp_overlap, dim3(512), dim3(256), 0, c->stream, c->d_md_seed_keys, c->d_md_bnd_keys, c->d_md_n, cap,
                       c->cfg.md_min_separation_distance > 1.f ? 1 : 0, seeds, bnd, c->d_md_parent, c->d_md_rootidx, c->d_md_bnd_mask, d_comp_out);
  }
  HIP_TRY(hipGetLastError());
  // counters + the first component records -> pinned memory by a one-workgroup kernel, the host spins on the ticket
  if (++c->md_head_ticket == 0) ++c->md_head_ticket;
  hipLaunchKernelGGL(k_publish, dim3(1), dim3(1024), 0, c->stream, c->d_md_n, reinterpret_cast<uint32_t*>(c->h_md_head.dev()),
                     static_cast<uint32_t>(sizeof(CompAcc) / 4), kCompHead, c->h_pinned.dev() + 8, c->md_head_ticket, c->d_md_scratch4);
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

// Runs the chain until the head counts are on the host: 1 = *head and *t are this frame's, 0 = the frame has no seeds, < 0 = error.
// Seed frames come in runs (something moves through the view for a while): a frame behind a seed frame has its chain queued
// before the wait for its seed count, sized for twice the previous frame's seed pixels.  The kernels then sit in the stream's queue
// behind the allocation / culling pass instead of arriving one by one after the count's trip to the host (78 us of idle main
// stream in front of the chain and 5 - 15 us between its seventeen launches, profiles/r06_kernel_trace_frames.txt).  A frame without
// seeds runs that chain on empty lists; more seed pixels than the bound: the chain is repeated with this frame's own sizes.  At
// most two more repeats follow: a table filled up, or more seed voxels than the LDS kernel takes (the lock-free component kernels
// are only queued when the previous seed frame came close to needing them).
static int mdRunChain(khr_ctx* c, FrameSlot& s, const MdHooks& hooks, bool device_merge, MdTables* t, MdHead* head) {
  const int n = s.sensor.width * s.sensor.height;
  bool with_global = c->md_host_walk || 2u * c->md_last_seeds > c->md_lds_max || c->md_lds_max < kCompLds;
  if (hooks.no_predict) with_global = false;
  uint32_t pre_px = 0, pre_mask = 0;
  if (mdQueuesAhead(c, hooks)) {
    pre_px = hooks.prelaunch_px ? hooks.prelaunch_px : std::min<uint32_t>(c->md_list_cap, std::max<uint32_t>(4096u, 2u * c->md_prev_seed_px));
    pre_mask = mdMaskFor(c, hooks, pre_px);
    KHR_TRY(mdLaunchChain(c, n, pre_px, pre_mask, with_global, device_merge, t));
    ++c->n_md_prelaunched;
  }
  KHR_TRY(waitSeedCount(c));
  s.clusters.clear();
  c->md_seed_run = c->h_pinned[0] != 0;
  if (c->h_pinned[0] == 0) return 0;
  c->md_prev_seed_px = c->h_pinned[0];
  s.dyn_clean = false;  // clusters may be painted from here on
  bool chain_queued = pre_px != 0 && c->h_pinned[0] <= pre_px;
  if (pre_px != 0 && !chain_queued) ++c->n_md_prelaunch_repeats;
  uint32_t mask = chain_queued ? pre_mask : mdMaskFor(c, hooks, c->h_pinned[0]);
  const uint32_t* cnt = reinterpret_cast<const uint32_t*>(c->h_md_head.get());
  for (int attempt = 0;; ++attempt) {
    if (!chain_queued) KHR_TRY(mdLaunchChain(c, n, c->h_pinned[0], mask, with_global, device_merge, t));
    chain_queued = false;
    KHR_TRY(waitTicket(c, 8, c->md_head_ticket, "the motion detector's component records"));
    const bool table_full = cnt[3] && mask < c->md_mask;                                    // once more with the worst-case size
    const bool lds_short = !table_full && cnt[0] > c->md_lds_max && !with_global;  // more seed voxels than the single-workgroup kernel takes
    if (attempt == 2 || !(table_full || lds_short)) break;
    if (table_full) mask = c->md_mask;
    else with_global = true;
  }
  *head = MdHead{cnt[0], cnt[1], cnt[2], cnt[3]};
  c->md_last_seeds = head->S;
  if (head->overflow) return fail(KHR_ENOMEM, "motion detector: neighbour table overflow (%u seed voxels)", head->S);
  if (head->S > c->md_list_cap || head->B > c->md_list_cap)
    return fail(KHR_ENOMEM, "motion detector: %u seed / %u boundary voxels exceed the list capacity %u", head->S, head->B, c->md_list_cap);
  return 1;
}

// Shared tail of both finishes, behind the final ids on the device: the paint pass, the clusters' summaries (queued here, or left
// to the caller with the largest id in *deferred_summary) and the slot's cluster list.  Returns the number of clusters.
static int mdPaintAndList(khr_ctx* c, FrameSlot& s, const MdTables& t, const mdh::Kept& kept, int* deferred_summary) {
  const int n = s.sensor.width * s.sensor.height;
  hipLaunchKernelGGL(k_md_paint, dim3(gridFor(n)), dim3(256), 0, c->stream, c->d_keys, n, t.seeds, t.bnd, c->d_md_seed_final,
                     c->d_md_bnd_final, s.dyn, c->d_md_bnd_deg, s.dynw);
  s.dyn_clean = false, s.dynw_valid = true;
  HIP_TRY(hipGetLastError());
  if (deferred_summary) *deferred_summary = kept.back().first;
  else KHR_TRY(clusterSummaryLaunch(c, s, kept.back().first));
  s.clusters.assign(kept.size(), khr_cluster{});
  for (size_t i = 0; i < kept.size(); ++i) {
    s.clusters[i].id = kept[i].first;
    s.clusters[i].num_pixels_listed = kept[i].second;
    s.clusters[i].semantic_id = -1;
  }
  return static_cast<int>(kept.size());
}

// Finish from the records: the clusters are the components, or (merge_here) the groups the device's overlap rows connect.  The
// host only numbers them; the ids go back inline or by a copy, and k_md_comp_finals spreads them over the listed voxels.
static int mdFinishFromRecords(khr_ctx* c, FrameSlot& s, const MdTables& t, const CompAcc* comp, uint32_t R, bool merge_here, int* deferred_summary) {
  const std::vector<uint32_t> order = mdh::clusterOrder(comp, R);
  const std::vector<uint32_t> group = merge_here ? mdh::groupsFromRows(comp, R) : mdh::Groups(R).labels();
  std::vector<int32_t> ids;
  const mdh::Kept kept = mdh::numberClusters(order.data(), group.data(), R, [&](uint32_t r) { return comp[r].n_pixels; },
                                             c->cfg.md_min_cluster_size, c->cfg.md_max_cluster_size, &ids);
  if (kept.empty()) return 0;
  CompFinals inl{};
  const int32_t* fin_dev = nullptr;
  if (R <= static_cast<uint32_t>(kCompInline)) {  // the ids travel in the kernel arguments
    std::copy(ids.begin(), ids.end(), inl.id);
  } else {
    int32_t* fin = reinterpret_cast<int32_t*>(c->h_md_head.get());  // the records are no longer needed once ids are taken
    std::copy(ids.begin(), ids.end(), fin);
    HIP_TRY(hipMemcpyAsync(c->d_md_comp_final, fin, sizeof(int32_t) * R, hipMemcpyHostToDevice, c->stream));
    fin_dev = c->d_md_comp_final;
  }
  // (the boundary voxels' final ids were zeroed by the compaction pass)
  hipLaunchKernelGGL(k_md_comp_finals, dim3(1024), dim3(256), 0, c->stream, c->d_md_adj, c->d_md_n, c->md_list_cap, c->cfg.md_neighbor_connectivity,
                     c->d_md_parent, c->d_md_rootidx, fin_dev, inl, c->d_md_seed_final, c->d_md_bnd_final, c->d_md_bnd_deg);
  return mdPaintAndList(c, s, t, kept, deferred_summary);
}

static void mdCopyWords(khr_ctx* c, const void* src, void* dst, size_t words) {
  if (words) hipLaunchKernelGGL(k_copy_words, dim3(static_cast<unsigned>((words + 255) / 256)), dim3(256), 0, c->stream,
                                static_cast<const uint32_t*>(src), static_cast<uint32_t*>(dst), static_cast<uint32_t>(words));
}

// Finish by the host walk.  The lists come down and the final ids go up through a page-locked block that kernels write and read:
// copies through the copy engines -- with a consumer downloading an output's 90 - 190 MB at the same time -- made this frame's
// few kilobytes wait 7 ms (profiles/r05_host_consumer_40.txt).  The walk reads the lists where they land and writes its results
// behind them in the same block, so nothing is copied on the host; the 64-bit lists come first to keep them aligned.
static int mdFinishByWalk(khr_ctx* c, FrameSlot& s, const MdTables& t, const MdHead& head, int* deferred_summary) {
  const size_t S = head.S, B = head.B, nn = static_cast<size_t>(c->cfg.md_neighbor_connectivity);
  const size_t o_sk = 0, o_bk = o_sk + 2 * S, o_sc = o_bk + 2 * B, o_adj = o_sc + S, o_bc = o_adj + S * nn;  // lists, in words
  const size_t o_sf = o_bc + B, o_bf = o_sf + S, o_bd = o_bf + B, walk_words = o_bd + B + 16;                // results
  if (c->ev_md_walk_up) HIP_TRY(hipEventSynchronize(c->ev_md_walk_up));  // (the previous seed frame's upload reads the block)
  if (walk_words > c->h_md_walk.count()) {
    const size_t want = std::max<size_t>(2 * walk_words, 1u << 18);
    if (c->h_md_walk.reserve(want)) return fail(KHR_ENOMEM, "page-locked block of the motion detector's host walk (%zu bytes)", want * 4);
  }
  KHR_TRY(c->ev_md_walk_up.ensure());
  uint32_t *const w = c->h_md_walk, *const w_dev = c->h_md_walk.dev();
  mdCopyWords(c, c->d_md_seed_keys, w_dev + o_sk, 2 * S);
  mdCopyWords(c, c->d_md_bnd_keys, w_dev + o_bk, 2 * B);
  mdCopyWords(c, c->d_md_seed_counts, w_dev + o_sc, S);
  mdCopyWords(c, c->d_md_adj, w_dev + o_adj, S * nn);
  mdCopyWords(c, c->d_md_bnd_counts, w_dev + o_bc, B);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  const mdh::WalkLists lists{reinterpret_cast<const uint64_t*>(w + o_sk), reinterpret_cast<const uint64_t*>(w + o_bk), w + o_sc, w + o_bc, w + o_adj,
                             head.S, head.B, static_cast<int>(nn)};
  const mdh::Kept kept = mdh::walkClusters(lists, c->cfg.md_min_separation_distance, c->cfg.md_min_cluster_size, c->cfg.md_max_cluster_size,
                                        reinterpret_cast<int32_t*>(w + o_sf), reinterpret_cast<int32_t*>(w + o_bf), reinterpret_cast<int32_t*>(w + o_bd));
  if (kept.empty()) return 0;
  mdCopyWords(c, w_dev + o_sf, c->d_md_seed_final, S);
  mdCopyWords(c, w_dev + o_bf, c->d_md_bnd_final, B);
  mdCopyWords(c, w_dev + o_bd, c->d_md_bnd_deg, B);
  HIP_TRY(hipEventRecord(c->ev_md_walk_up, c->stream));
  return mdPaintAndList(c, s, t, kept, deferred_summary);
}

// The clusters of a frame whose seed pixels are being counted; returns their number.  deferred_summary: nullptr = the clusters'
// summaries are queued behind the paint pass; otherwise the caller queues them (clusterSummaryLaunch) and receives the largest
// cluster id here, or -1 when there is nothing to summarise
static int motionFinish(khr_ctx* c, FrameSlot& s, int* deferred_summary = nullptr) {
  if (deferred_summary) *deferred_summary = -1;
  if (!c->cfg.with_tracking) return 0;
  const MdHooks hooks = mdHooks();
  const float sep = c->cfg.md_min_separation_distance;
  const bool device_merge = !hooks.no_device_merge && !c->md_host_walk && sep > 0.f && sep <= 2.f;
  MdTables t{};
  MdHead head{};
  const int rc = mdRunChain(c, s, hooks, device_merge, &t, &head);
  if (rc <= 0) return rc;
  c->stats.n_seeds = head.S;
  if (head.R <= kCompCap && !c->md_host_walk) {
    if (head.R > kCompHead) {  // (the first kCompHead records came with the head counts)
      HIP_TRY(hipMemcpyAsync(c->h_md_head, c->d_md_n, 16 + sizeof(CompAcc) * head.R, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const CompAcc* comp = reinterpret_cast<const CompAcc*>(c->h_md_head + 16);
    // no two boxes closer than the separation: the clusters are the components.  Otherwise the device's overlap rows say who
    // merges (they exist for up to 64 components), or the exact voxel-pair test runs in the host walk below
    const bool may_merge = mdh::mayMerge(comp, head.R, sep);
    const bool merge_here = may_merge && device_merge && head.R <= 64;
    if (merge_here) ++c->n_md_device_merges;
    if (!may_merge || merge_here) return mdFinishFromRecords(c, s, t, comp, head.R, merge_here, deferred_summary);
  }
  ++c->n_md_host_walks;
  return mdFinishByWalk(c, s, t, head, deferred_summary);
}

int khr_detect_motion(khr_ctx* c, int slot) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  int rc = motionLaunch(c, s, false);
  if (rc) return rc;
  return motionFinish(c, s);
}

int khr_motion_keys(khr_ctx* c, int slot, void* keys_out, int on_device, uint32_t* n_seed_pixels) {
  if (!c || !keys_out || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const int n = s.sensor.width * s.sensor.height;
  int rc = motionLaunch(c, s, false);
  if (rc) return rc;
  uint64_t* dst = static_cast<uint64_t*>(keys_out);
  DevTemp holder;
  if (!on_device) {
    KHR_TRY(holder.alloc(sizeof(uint64_t) * n));
    dst = holder.as<uint64_t>();
  }
  hipLaunchKernelGGL(k_md_keys_export, dim3(gridFor(n)), dim3(256), 0, c->stream, c->d_keys, n, dst);
  if (!on_device) {
    HIP_TRY(hipMemcpyAsync(keys_out, dst, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  if (!n_seed_pixels && on_device) {
    // nobody asked for the count and the keys stay on the device: nothing to wait for (a sharded tick calls this once per
    // seed camera; eight host round trips in a row were a third of an 8-camera tick)
    c->seed_publish_pending = false;
    c->seed_by_ticket = false;
    return KHR_OK;
  }
  { const int rcw = waitSeedCount(c); if (rcw) return rcw; }
  if (n_seed_pixels) *n_seed_pixels = c->h_pinned[0];
  return KHR_OK;
}

int khr_detect_motion_from_keys(khr_ctx* c, int slot, const void* keys, int on_device) {
  if (!c || !keys || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const int n = s.sensor.width * s.sensor.height;
  const uint64_t* src = static_cast<const uint64_t*>(keys);
  DevTemp holder;  // (freed when this call returns; hipFree waits for the kernels that read it)
  if (!on_device) {
    KHR_TRY(holder.alloc(sizeof(uint64_t) * n));
    HIP_TRY(hipMemcpyAsync(holder.get(), keys, sizeof(uint64_t) * n, hipMemcpyHostToDevice, c->stream));
    src = holder.as<uint64_t>();
  }
  if (!s.dyn_clean) HIP_TRY(hipMemsetAsync(s.dyn, 0, sizeof(int32_t) * n, c->stream));
  s.dyn_clean = true, s.dynw_valid = false;
  HIP_TRY(hipMemsetAsync(&c->m.counters[C_N_SEEDS], 0, sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_md_keys_import, dim3(gridFor(n)), dim3(256), 0, c->stream, src, n, c->d_keys, &c->m.counters[C_N_SEEDS]);
  HIP_TRY(hipMemcpyAsync(&c->h_pinned[0], &c->m.counters[C_N_SEEDS], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(c->ev_seed, c->stream));
  c->seed_by_ticket = false;
  return motionFinish(c, s);
}

size_t khr_motion_bits_bytes(int64_t n_pixels) { return n_pixels > 0 ? 16u * static_cast<size_t>((n_pixels + 63) / 64) : 0u; }

int khr_motion_bits(khr_ctx* c, int slot, void* bits_device) {
  if (!c || !bits_device || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const int n = s.sensor.width * s.sensor.height;
  int rc = motionLaunch(c, s, false);
  if (rc) return rc;
  hipLaunchKernelGGL(k_md_bits_export, dim3(gridFor((static_cast<size_t>(n) + 63) / 64 * 64)), dim3(256), 0, c->stream, c->d_keys, n,
                     static_cast<unsigned long long*>(bits_device));
  HIP_TRY(hipGetLastError());
  c->seed_publish_pending = false;  // (nobody waits for this pass's count: the ranks' counts were exchanged before)
  c->seed_by_ticket = false;
  return KHR_OK;
}

int khr_detect_motion_from_bits(khr_ctx* c, int slot, const void* bits_device) {
  if (!c || !bits_device || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const int n = s.sensor.width * s.sensor.height;
  if (!s.dyn_clean) HIP_TRY(hipMemsetAsync(s.dyn, 0, sizeof(int32_t) * n, c->stream));
  s.dyn_clean = true, s.dynw_valid = false;
  HIP_TRY(hipMemsetAsync(&c->m.counters[C_N_SEEDS], 0, sizeof(uint32_t), c->stream));
  const float min_z_world = static_cast<float>(s.meta.world_T_sensor[11] + static_cast<double>(c->cfg.md_min_z_coordinate));
  hipLaunchKernelGGL(k_md_keys_from_bits, dim3(gridFor(n)), dim3(256), 0, c->stream, c->p, makeDevFrame(c, s), c->cfg.md_max_range, min_z_world,
                     static_cast<const unsigned long long*>(bits_device), c->d_keys, &c->m.counters[C_N_SEEDS]);
  HIP_TRY(hipMemcpyAsync(&c->h_pinned[0], &c->m.counters[C_N_SEEDS], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(c->ev_seed, c->stream));
  c->seed_by_ticket = false;
  return motionFinish(c, s);
}

int khr_dynamic_pack_bytes(khr_ctx* c, int slot, void* dst_device) {
  if (!c || !dst_device || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const int n4 = (s.sensor.width * s.sensor.height + 3) / 4;  // (the slot's images are allocated for max_frame_pixels, a multiple of 4 or padded)
  hipLaunchKernelGGL(k_dyn_pack_u8, dim3(gridFor(n4)), dim3(256), 0, c->stream, s.dyn, n4, static_cast<uint32_t*>(dst_device));
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

int khr_dynamic_unpack_bytes(khr_ctx* c, int slot, const void* src_device) {
  if (!c || !src_device || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  const int n4 = (s.sensor.width * s.sensor.height + 3) / 4;
  hipLaunchKernelGGL(k_dyn_unpack_u8, dim3(gridFor(n4)), dim3(256), 0, c->stream, static_cast<const uint32_t*>(src_device), n4, s.dyn);
  HIP_TRY(hipGetLastError());
  s.dyn_clean = false;
  s.dynw_valid = false;
  return KHR_OK;
}

// The motion detector's result of frame slot `src` (painted dynamic image, cluster list) also becomes that of slot `dst`: two
// slots that hold the SAME camera frame (sender-side ingest of the sharded tick: the rank's own converted frame, which the
// object half keeps, and its adopted twin in the all-gather buffer, which the tick paints).  Stream-ordered device copy.
int khr_mirror_dynamic(khr_ctx* c, int src, int dst) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!validSlot(c, src) || !validSlot(c, dst)) return fail(KHR_EINVAL, "bad slot");
  if (src == dst) return KHR_OK;
  FrameSlot& a = c->slots[src];
  FrameSlot& b = c->slots[dst];
  if (a.sensor.width != b.sensor.width || a.sensor.height != b.sensor.height) return fail(KHR_EINVAL, "the slots hold frames of different sizes");
  HIP_TRY(hipSetDevice(c->device));
  if (!(a.dyn_clean && b.dyn_clean)) {
    HIP_TRY(hipMemcpyAsync(b.dyn, a.dyn, sizeof(int32_t) * static_cast<size_t>(a.sensor.width) * a.sensor.height, hipMemcpyDeviceToDevice, c->stream));
    if (a.dynw_valid)
      HIP_TRY(hipMemcpyAsync(b.dynw, a.dynw, static_cast<size_t>(a.sensor.width) * a.sensor.height, hipMemcpyDeviceToDevice, c->stream));
  }
  b.dyn_clean = a.dyn_clean;
  b.dynw_valid = a.dynw_valid;
  b.clusters = a.clusters;
  return KHR_OK;
}

int khr_get_dynamic_clusters(khr_ctx* c, int slot, khr_cluster* out, int cap) {
  if (!c || cap < 0 || (!out && cap > 0)) return fail(KHR_EINVAL, "bad argument");
  if (!validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  const int n = static_cast<int>(c->slots[slot].clusters.size());
  if (n == 0) return 0;
  // the summaries (the tracker's bounding boxes, max_iou_tracker.cpp:466-476) were queued behind the paint pass and
  // published to pinned memory; for an older slot (only the latest frame's are kept) they are recomputed here
  FrameSlot& s = c->slots[slot];
  const ClusterAcc* acc = c->h_md_acc_pinned;
  if (c->md_acc_slot == slot) {
    const int rcw = waitTicket(c, 7, c->md_acc_ticket, "the dynamic cluster summaries");
    if (rcw) return rcw;
  } else {
    const int rcs = clusterSummaryLaunch(c, s, 255);
    if (rcs) return rcs;
    const int rcw = waitTicket(c, 7, c->md_acc_ticket, "the dynamic cluster summaries");
    if (rcw) return rcw;
  }
  for (int i = 0; i < n && i < cap; ++i) {
    khr_cluster k = s.clusters[i];
    const ClusterAcc& a = acc[k.id];
    k.num_pixels_painted = a.n_pixels;
    for (int d = 0; d < 3; ++d) {
      k.bbox_min[d] = a.n_pixels ? orderedToFloat(a.bmin[d]) : 0.f;
      k.bbox_max[d] = a.n_pixels ? orderedToFloat(a.bmax[d]) : 0.f;
      // the centroid the reference's consumers compute: the mean over cluster.pixels, which lists a boundary voxel's pixels once
      // per adjacent seed (mesh_object_extractor.cpp:136-147, max_iou_tracker.cpp:541-548)
      k.centroid[d] = a.n_listed ? a.wsum[d] / static_cast<float>(a.n_listed) : (a.n_pixels ? a.sum[d] / static_cast<float>(a.n_pixels) : 0.f);
    }
    out[i] = k;
  }
  return n;
}

// ---------------------------------------------------------------------------------------------
// object detection (ConnectedSemantics role) and per-cluster voxel sets (MaxIoUTracker measurement role)
// ---------------------------------------------------------------------------------------------
static int ensureGv(khr_ctx* c) {
  if (c->d_gv_keys) return KHR_OK;
  const size_t npx = c->cfg.max_frame_pixels;
  size_t ts = 1024;
  while (ts < 2 * npx) ts <<= 1;
  c->gv_mask = static_cast<uint32_t>(ts - 1);
  c->obj_root_cap = 1u << 16;
  int rc = KHR_OK;
  KHR_CHAIN(devAlloc(c, &c->d_gv_keys, ts, false));
  KHR_CHAIN(devAlloc(c, &c->d_gv_parent, ts, false));  // >= npx: also the per-pixel parent array of the 2D mode
  KHR_CHAIN(devAlloc(c, &c->d_gv_rootidx, ts, false));
  KHR_CHAIN(devAlloc(c, &c->d_gv_node, npx, false));
  KHR_CHAIN(devAlloc(c, &c->d_gv_owners, npx, false));
  KHR_CHAIN(devAlloc(c, &c->d_gv_done, 4));
  {
    // counters and cluster records are contiguous: one small copy brings both to the host
    uint8_t* head = nullptr;
    KHR_CHAIN(devAlloc(c, &head, 16 + sizeof(ObjAcc) * c->obj_root_cap));
    c->d_gv_n = reinterpret_cast<uint32_t*>(head);
    c->d_obj_acc = head ? reinterpret_cast<ObjAcc*>(head + 16) : nullptr;
  }
  KHR_CHAIN(devAlloc(c, &c->d_obj_final, c->obj_root_cap, false));
  for (int w = 0; w < 3; ++w) {
    uint8_t* head = nullptr;
    KHR_CHAIN(devAlloc(c, &head, 16 + sizeof(uint64_t) * npx));
    c->d_cv_n[w] = reinterpret_cast<uint32_t*>(head);
    c->d_cv_keys[w] = head ? reinterpret_cast<uint64_t*>(head + 16) : nullptr;
    KHR_CHAIN(c->h_cv[w].alloc(16 + sizeof(uint64_t) * npx));
    KHR_CHAIN(c->ev_cv[w].ensure());
  }
  KHR_CHAIN(c->h_obj_head.alloc(16 + sizeof(ObjAcc) * c->obj_root_cap));
  KHR_CHAIN(c->ev_obj.ensure());
  if (rc == KHR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = KHR_EDEVICE;  // zero-fills above vs the auxiliary stream
  return rc;
}

// voxel of the sensor position on a grid: the origin of the relative voxel window
static int3 windowOrigin(const DevFrame& f, float inv) {
  return make_int3(static_cast<int>(std::floor(f.tw[0] * inv)), static_cast<int>(std::floor(f.tw[1] * inv)),
                   static_cast<int>(std::floor(f.tw[2] * inv)));
}

int khr_configure_object_detector(khr_ctx* c, const khr_object_detector_config* cfg) {
  if (!c || !cfg) return fail(KHR_EINVAL, "null argument");
  if (cfg->n_object_labels < 0 || (cfg->n_object_labels > 0 && !cfg->object_labels)) return fail(KHR_EINVAL, "bad object label list");
  if (cfg->use_3d && !(cfg->grid_size > 0.f)) return fail(KHR_EINVAL, "grid_size must be > 0");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensureGv(c);
  if (rc) return rc;
  c->obj_cfg = *cfg;
  c->obj_labels.assign(cfg->object_labels, cfg->object_labels + cfg->n_object_labels);
  std::sort(c->obj_labels.begin(), c->obj_labels.end());
  c->obj_labels.erase(std::unique(c->obj_labels.begin(), c->obj_labels.end()), c->obj_labels.end());
  if (c->obj_labels.size() > kGvMaxGroup) return fail(KHR_EINVAL, "more than %u object labels", kGvMaxGroup);
  c->obj_cfg.object_labels = nullptr;
  c->obj_cfg.n_object_labels = static_cast<int32_t>(c->obj_labels.size());
  if (c->d_obj_labels) HIP_TRY(hipStreamSynchronize(c->stream));
  KHR_TRY(c->d_obj_labels.alloc(std::max<size_t>(c->obj_labels.size(), 1)));
  if (!c->obj_labels.empty()) {
    HIP_TRY(hipMemcpyAsync(c->d_obj_labels, c->obj_labels.data(), sizeof(int32_t) * c->obj_labels.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  c->obj_configured = true;
  return KHR_OK;
}

// ConnectedSemantics, part 1: everything up to the per-cluster records, and their copy to pinned memory.  No host
// wait: khr_process_frame issues this right after the frame ingest and looks at the records when the rest of the
// frame's kernels are queued.
static int objectsLaunch(khr_ctx* c, int slot) {
  FrameSlot& s = c->slots[slot];
  const int n = s.sensor.width * s.sensor.height;
  const khr_object_detector_config& oc = c->obj_cfg;
  s.sem_clusters.clear();
  s.objects_done = false;
  s.has_obj = true;
  s.aux_seq = c->obj_seq = ++c->aux_seq_issued;
  c->obj_pending_slot = -1;
  if (c->obj_cv_slot == slot) c->obj_cv_slot = -1;  // (the slot's object image is about to be rewritten)
  const int n_labels = static_cast<int>(c->obj_labels.size());
  if (!s.has_label || n_labels == 0) {
    HIP_TRY(hipMemsetAsync(s.obj, 0, sizeof(int32_t) * n, c->aux_stream));
    s.objects_done = true;
    return KHR_OK;
  }
  const DevFrame f = makeDevFrame(c, s);
  GvTable t{c->d_gv_keys, c->gv_mask};
  const uint32_t tsize = c->gv_mask + 1;
  // (the object image needs no clearing: the paint pass writes every pixel)
  if (oc.use_3d) {
    const float inv = 1.f / oc.grid_size;  // connected_semantics.cpp:75
    // (the counters were zeroed by the k_publish of the previous request, unless that one never got that far)
    if (!c->gv_clean) hipLaunchKernelGGL(k_gv_clear, dim3(gridFor(tsize / 2)), dim3(256), 0, c->aux_stream, c->d_gv_keys, tsize, c->d_gv_n);
    else if (!c->gv_counters_clean[0]) HIP_TRY(hipMemsetAsync(c->d_gv_n, 0, sizeof(uint32_t) * 4, c->aux_stream));
    c->gv_clean = false;
    c->gv_counters_clean[0] = false;
    hipLaunchKernelGGL(k_obj_insert3d, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, f, c->d_obj_labels, n_labels, oc.max_range, inv,
                       windowOrigin(f, inv), t, c->d_gv_parent, c->d_gv_node, c->d_gv_n + 1, c->d_gv_owners, c->d_gv_n + 2);
    hipLaunchKernelGGL(k_obj_union3d, dim3(1024), dim3(256), 0, c->aux_stream, c->d_gv_owners, c->d_gv_n + 2, t, c->d_gv_parent,
                       oc.use_full_connectivity ? 13 : 3);
    hipLaunchKernelGGL(k_obj_roots3d, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, c->d_gv_owners, c->d_gv_n + 2, c->d_gv_parent,
                       c->d_gv_rootidx, c->d_gv_n, c->obj_root_cap, c->d_obj_acc, c->d_gv_keys);
    // (the keys are not needed any more -- the paint pass goes through pix_node -> parent -> root_idx --: the table is given
    //  back by the chain's last launch, together with the publish)
  } else {
    HIP_TRY(hipMemsetAsync(c->d_gv_n, 0, sizeof(uint32_t) * 4, c->aux_stream));
    hipLaunchKernelGGL(k_obj_init2d, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, f, c->d_obj_labels, n_labels, c->d_gv_parent, c->d_gv_node);
    hipLaunchKernelGGL(k_obj_union2d, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, f, c->d_gv_node, c->d_gv_parent,
                       oc.use_full_connectivity ? 1 : 0);
    hipLaunchKernelGGL(k_obj_roots, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, c->d_gv_node, n, c->d_gv_parent, c->d_gv_rootidx, c->d_gv_n,
                       c->obj_root_cap, c->d_obj_acc, nullptr, s.vLabel(), c->d_obj_labels, n_labels);
  }
  const int obj_tiles = ((s.sensor.width + kObjTile - 1) / kObjTile) * ((s.sensor.height + kObjTile - 1) / kObjTile);
  hipLaunchKernelGGL(k_obj_paint, dim3(obj_tiles), dim3(1024), 0, c->aux_stream, f, c->d_gv_node, c->d_gv_parent, c->d_gv_rootidx,
                     c->obj_root_cap, s.obj, c->d_obj_acc);
  HIP_TRY(hipGetLastError());
  if (++c->obj_ticket == 0) ++c->obj_ticket;
  if (oc.use_3d) {
    hipLaunchKernelGGL(k_gv_release_publish, dim3(kGvReleaseGrid), dim3(256), 0, c->aux_stream, c->d_gv_owners, c->d_gv_n + 2, c->d_gv_keys,
                       c->d_gv_done, c->d_gv_n, reinterpret_cast<uint32_t*>(c->h_obj_head.dev()), static_cast<uint32_t>(sizeof(ObjAcc) / 4), kObjHead,
                       c->h_pinned.dev() + 4, c->obj_ticket, c->d_gv_n);
    c->gv_clean = true;
  } else {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(1024), 0, c->aux_stream, c->d_gv_n, reinterpret_cast<uint32_t*>(c->h_obj_head.dev()),
                       static_cast<uint32_t>(sizeof(ObjAcc) / 4), kObjHead, c->h_pinned.dev() + 4, c->obj_ticket, c->d_gv_n);
  }
  HIP_TRY(hipGetLastError());
  c->gv_counters_clean[0] = oc.use_3d != 0;  // (the 2D path resets them itself)
  c->obj_pending_slot = slot;
  return KHR_OK;
}

// ticket word of a voxel result set in h_pinned
static int cvTicketWord(int set) { return set == 2 ? 12 : 5 + set; }

// tail of a voxel-set request: the table is given back empty, the result set's head goes to pinned memory
static int cvReleasePublish(khr_ctx* c, int set) {
  c->gv_clean = true;
  if (++c->cv_ticket[set] == 0) ++c->cv_ticket[set];
  hipLaunchKernelGGL(k_gv_release_publish, dim3(kGvReleaseGrid), dim3(256), 0, c->aux_stream, c->d_gv_owners, c->d_cv_n[set], c->d_gv_keys,
                     c->d_gv_done, c->d_cv_n[set], reinterpret_cast<uint32_t*>(c->h_cv[set].dev()), 2u,
                     static_cast<uint32_t>(std::min<size_t>(kCvHead, c->cfg.max_frame_pixels)), c->h_pinned.dev() + cvTicketWord(set),
                     c->cv_ticket[set], c->d_cv_n[set]);
  HIP_TRY(hipGetLastError());
  c->gv_counters_clean[1 + set] = true;
  return KHR_OK;
}

// ConnectedSemantics, part 2: order / filter the clusters on the host, remap the provisional ids.  Returns the
// number of semantic clusters.
static int objectsFinish(khr_ctx* c, int slot) {
  FrameSlot& s = c->slots[slot];
  if (s.objects_done) return static_cast<int>(s.sem_clusters.size());
  if (c->obj_pending_slot != slot) return fail(KHR_ESTATE, "object detection was not launched for this slot");
  c->obj_pending_slot = -1;
  const int n = s.sensor.width * s.sensor.height;
  const khr_object_detector_config& oc = c->obj_cfg;
  {
    const int rcw = waitTicket(c, 4, c->obj_ticket, "the object detector's cluster records", c->aux_stream);
    if (rcw) return rcw;
    c->aux_seq_done = std::max(c->aux_seq_done, c->obj_seq);
  }
  const uint32_t* cnt = reinterpret_cast<const uint32_t*>(c->h_obj_head.get());
  if (cnt[1] & 1u) return fail(KHR_EINVAL, "object detector: a measured point lies more than %d grid cells from the sensor", kGvWindow);
  const uint32_t R = cnt[0];
  if (R > c->obj_root_cap) return fail(KHR_ENOMEM, "object detector: %u clusters exceed the capacity %u", R, c->obj_root_cap);
  s.objects_done = true;
  if (R == 0) return 0;
  if (R > kObjHead) {
    HIP_TRY(hipMemcpyAsync(c->h_obj_head, c->d_gv_n, 16 + sizeof(ObjAcc) * R, hipMemcpyDeviceToHost, c->aux_stream));
    HIP_TRY(hipStreamSynchronize(c->aux_stream));
  }
  const ObjAcc* acc = reinterpret_cast<const ObjAcc*>(c->h_obj_head + 16);
  // cluster order: 3D mode = by semantic id (std::map, connected_semantics.h:87), then by first pixel in scan order
  // (ASSUMPTIONS.md C.4); 2D mode = discovery order of the column-major scan (:147-160)
  std::vector<uint32_t> order(R);
  for (uint32_t i = 0; i < R; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (oc.use_3d && acc[a].group != acc[b].group) return acc[a].group < acc[b].group;
    return acc[a].first_cm < acc[b].first_cm;
  });
  std::vector<int32_t> fin(R, 0);
  int next_id = 1;
  for (uint32_t r : order) {
    const ObjAcc& a = acc[r];
    const int size = static_cast<int>(a.n_pixels);
    int id;
    if (oc.use_3d) {  // size filter before the id is taken (:104-110)
      if (size < oc.min_cluster_size || (oc.max_cluster_size > 0 && size > oc.max_cluster_size)) continue;
      id = next_id++;
    } else {          // ids are taken by every component, small ones are erased afterwards (filterClusters, :200-216)
      id = next_id++;
      if (size < oc.min_cluster_size) continue;
    }
    fin[r] = id;
    khr_cluster k{};
    k.id = id;
    k.num_pixels_listed = a.n_pixels;
    k.num_pixels_painted = a.n_pixels;
    for (int d = 0; d < 3; ++d) {
      k.bbox_min[d] = orderedToFloat(a.bmin[d]);
      k.bbox_max[d] = orderedToFloat(a.bmax[d]);
      k.centroid[d] = a.sum[d] / static_cast<float>(a.n_pixels);
    }
    k.semantic_id = c->obj_labels[a.group];
    s.sem_clusters.push_back(k);
  }
  // the records are consumed: the pinned block now carries the final ids to the device
  if (R <= static_cast<uint32_t>(kRemapTab)) {  // the usual case: the table rides in the kernel arguments
    RemapTab tab{};
    std::memcpy(tab.v, fin.data(), sizeof(int32_t) * R);
    if (c->obj_cv_size > 0.f) {
      // the tracker's voxel sets of this object image in the same pass, into the result set that no fetch is reading; a
      // khr_cluster_voxels_launch(slot, 1, obj_cv_size) adopts it
      const int set = 3 - c->cv_set_obj;
      const DevFrame f = makeDevFrame(c, s);
      const float inv = 1.f / c->obj_cv_size;
      s.aux_seq = c->cv_seq[set] = ++c->aux_seq_issued;
      c->cv_origin[set] = windowOrigin(f, inv);
      GvTable t{c->d_gv_keys, c->gv_mask};
      const uint32_t tsize = c->gv_mask + 1;
      if (!c->gv_clean) hipLaunchKernelGGL(k_gv_clear, dim3(gridFor(tsize / 2)), dim3(256), 0, c->aux_stream, c->d_gv_keys, tsize, c->d_cv_n[set]);
      else if (!c->gv_counters_clean[1 + set]) HIP_TRY(hipMemsetAsync(c->d_cv_n[set], 0, sizeof(uint32_t) * 4, c->aux_stream));
      c->gv_clean = false;
      c->gv_counters_clean[1 + set] = false;
      hipLaunchKernelGGL(k_obj_remap_cluster_voxels, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, f, s.obj, tab, inv, c->cv_origin[set], t,
                         c->d_cv_keys[set], c->d_cv_n[set], static_cast<uint32_t>(c->cfg.max_frame_pixels), c->d_cv_n[set] + 1, c->d_gv_owners);
      HIP_TRY(hipGetLastError());
      const int rcp = cvReleasePublish(c, set);
      if (rcp) return rcp;
      c->obj_cv_slot = slot;
    } else {
      hipLaunchKernelGGL(k_obj_remap_tab, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, s.obj, n, tab);
    }
  } else {
    std::memcpy(c->h_obj_head, fin.data(), sizeof(int32_t) * R);
    HIP_TRY(hipMemcpyAsync(c->d_obj_final, c->h_obj_head, sizeof(int32_t) * R, hipMemcpyHostToDevice, c->aux_stream));
    hipLaunchKernelGGL(k_obj_remap, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, s.obj, n, c->d_obj_final);
  }
  HIP_TRY(hipGetLastError());
  return static_cast<int>(s.sem_clusters.size());
}

int khr_detect_objects(khr_ctx* c, int slot) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  if (!c->obj_configured) return fail(KHR_ESTATE, "khr_configure_object_detector has not been called");
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  if (s.objects_done) return static_cast<int>(s.sem_clusters.size());  // already done inside khr_process_frame
  if (c->obj_pending_slot != slot) {
    int rc = auxAfterMain(c);  // the slot's ingest (and whatever else the caller queued) comes first
    if (!rc) rc = objectsLaunch(c, slot);
    if (rc) return rc;
  }
  return objectsFinish(c, slot);
}

// first half of khr_detect_objects: the detector's kernels are queued on the auxiliary stream (behind the slot's ingest),
// nothing is awaited; khr_detect_objects(slot) later only collects the result.  Lets a caller that has other device work to
// queue first (the sharded tick) overlap it with the detection of its own camera's frame.
int khr_detect_objects_launch(khr_ctx* c, int slot) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  if (!c->obj_configured) return KHR_ESTATE;  // (no detector configured: not an error here, nothing to launch)
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& s = c->slots[slot];
  if (s.objects_done || c->obj_pending_slot == slot) return KHR_OK;
  int rc = auxAfterMain(c);
  if (!rc) rc = objectsLaunch(c, slot);
  return rc;
}

int khr_get_semantic_clusters(khr_ctx* c, int slot, khr_cluster* out, int cap) {
  if (!c || cap < 0 || (!out && cap > 0)) return fail(KHR_EINVAL, "bad argument");
  if (!validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  const FrameSlot& s = c->slots[slot];
  if (!s.objects_done) return fail(KHR_ESTATE, "khr_detect_objects has not run for this frame");
  const int n = static_cast<int>(s.sem_clusters.size());
  for (int i = 0; i < n && i < cap; ++i) out[i] = s.sem_clusters[i];
  return n;
}

int khr_configure_object_voxel_sets(khr_ctx* c, float voxel_size) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!(voxel_size >= 0.f) || !std::isfinite(voxel_size)) return fail(KHR_EINVAL, "voxel_size must be >= 0 (0 = off)");
  if (voxel_size != c->obj_cv_size) c->obj_cv_slot = -1;  // (sets queued ahead at the old size are not adopted)
  c->obj_cv_size = voxel_size;
  return KHR_OK;
}

int khr_cluster_voxels_launch(khr_ctx* c, int slot, int which, float voxel_size) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  if (!(voxel_size > 0.f) || (which != 0 && which != 1)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensureGv(c);
  if (rc) return rc;
  FrameSlot& s = c->slots[slot];
  c->cv_pending_slot[which] = slot;
  if (which == 1 && c->obj_cv_slot == slot && c->obj_cv_size == voxel_size && s.has_obj) {
    // objectsFinish queued exactly this request with the id remap: its result set becomes the one the fetch reads
    c->cv_set_obj = 3 - c->cv_set_obj;
    c->obj_cv_slot = -1;
    return KHR_OK;
  }
  const int set = which == 0 ? 0 : c->cv_set_obj;
  uint32_t* hc = reinterpret_cast<uint32_t*>(c->h_cv[set].get());
  if (which == 1 && !s.has_obj) {  // no object image: nothing to look at
    hc[0] = hc[1] = 0;
    c->cv_ticket[set] = c->h_pinned[cvTicketWord(set)];  // nothing in flight: the fetch sees the current ticket
    return KHR_OK;
  }
  const int n = s.sensor.width * s.sensor.height;
  const DevFrame f = makeDevFrame(c, s);
  const float inv = 1.f / voxel_size;  // spatial_hash::Grid(voxel_size)
  if (which == 0) {  // the dynamic image is painted on the main stream
    rc = auxAfterMain(c);
    if (rc) return rc;
  }
  s.aux_seq = c->cv_seq[set] = ++c->aux_seq_issued;
  c->cv_origin[set] = windowOrigin(f, inv);
  GvTable t{c->d_gv_keys, c->gv_mask};
  const uint32_t tsize = c->gv_mask + 1;
  if (!c->gv_clean) hipLaunchKernelGGL(k_gv_clear, dim3(gridFor(tsize / 2)), dim3(256), 0, c->aux_stream, c->d_gv_keys, tsize, c->d_cv_n[set]);
  else if (!c->gv_counters_clean[1 + set]) HIP_TRY(hipMemsetAsync(c->d_cv_n[set], 0, sizeof(uint32_t) * 4, c->aux_stream));
  c->gv_clean = false;
  c->gv_counters_clean[1 + set] = false;
  hipLaunchKernelGGL(k_cluster_voxels, dim3(gridFor(n)), dim3(256), 0, c->aux_stream, f, which == 0 ? s.dyn : s.obj, inv, c->cv_origin[set], t,
                     c->d_cv_keys[set], c->d_cv_n[set], static_cast<uint32_t>(c->cfg.max_frame_pixels), c->d_cv_n[set] + 1,
                     c->d_gv_owners);
  HIP_TRY(hipGetLastError());
  return cvReleasePublish(c, set);
}

int64_t khr_cluster_voxels_fetch(khr_ctx* c, int which, int32_t* ids_out, int64_t* voxels_out, int64_t cap) {
  if (!c || (which != 0 && which != 1) || cap < 0 || (cap > 0 && (!ids_out || !voxels_out))) return fail(KHR_EINVAL, "bad argument");
  if (c->cv_pending_slot[which] < 0) return fail(KHR_ESTATE, "khr_cluster_voxels_launch has not been called");
  const int set = which == 0 ? 0 : c->cv_set_obj;
  {
    const int rcw = waitTicket(c, cvTicketWord(set), c->cv_ticket[set], "the cluster voxel sets", c->aux_stream);
    if (!rcw) c->aux_seq_done = std::max(c->aux_seq_done, c->cv_seq[set]);
    if (rcw) return rcw;
  }
  const uint32_t* cnt = reinterpret_cast<const uint32_t*>(c->h_cv[set].get());
  if (cnt[1] & 1u) return fail(KHR_EINVAL, "cluster voxels: a measured point lies more than %d voxels from the sensor", kGvWindow);
  if (cnt[1] & 2u) return fail(KHR_EINVAL, "cluster voxels: cluster id above %u", kGvMaxGroup);
  const uint32_t N = cnt[0];
  if (N == 0) return 0;
  if (N > kCvHead) {
    HIP_TRY(hipMemcpyAsync(c->h_cv[set], c->d_cv_n[set], 16 + sizeof(uint64_t) * N, hipMemcpyDeviceToHost, c->aux_stream));
    HIP_TRY(hipStreamSynchronize(c->aux_stream));
  }
  const uint64_t* keys = reinterpret_cast<const uint64_t*>(c->h_cv[set] + 16);
  const int3 origin = c->cv_origin[set];
  struct E { int32_t id; int64_t v[3]; };
  std::vector<E> e(N);
  for (uint32_t i = 0; i < N; ++i) {
    uint32_t g;
    int x, y, z;
    gvUnpack(keys[i], &g, &x, &y, &z);
    e[i].id = static_cast<int32_t>(g);
    if (gvIsOrigin(keys[i])) {
      e[i].v[0] = e[i].v[1] = e[i].v[2] = 0;
    } else {
      e[i].v[0] = static_cast<int64_t>(x) + origin.x;
      e[i].v[1] = static_cast<int64_t>(y) + origin.y;
      e[i].v[2] = static_cast<int64_t>(z) + origin.z;
    }
  }
  std::sort(e.begin(), e.end(), [](const E& a, const E& b) {
    if (a.id != b.id) return a.id < b.id;
    if (a.v[0] != b.v[0]) return a.v[0] < b.v[0];
    if (a.v[1] != b.v[1]) return a.v[1] < b.v[1];
    return a.v[2] < b.v[2];
  });
  for (int64_t i = 0; i < static_cast<int64_t>(N) && i < cap; ++i) {
    ids_out[i] = e[i].id;
    for (int d = 0; d < 3; ++d) voxels_out[3 * i + d] = e[i].v[d];
  }
  return static_cast<int64_t>(N);
}

int64_t khr_cluster_voxels(khr_ctx* c, int slot, int which, float voxel_size, int32_t* ids_out, int64_t* voxels_out, int64_t cap) {
  if (cap < 0 || (cap > 0 && (!ids_out || !voxels_out))) return fail(KHR_EINVAL, "bad argument");
  const int rc = khr_cluster_voxels_launch(c, slot, which, voxel_size);
  if (rc) return rc;
  return khr_cluster_voxels_fetch(c, which, ids_out, voxels_out, cap);
}

int khr_pixel_iou(khr_ctx* c, int slot, const khr_pixel_ref* refs, int n_refs, int max_id, uint32_t* n_points, uint32_t* inter) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  if (n_refs < 0 || n_refs > kPixRefs || (n_refs > 0 && (!refs || !n_points || !inter)) || max_id < 1 || max_id > 65535)
    return fail(KHR_EINVAL, "bad argument (at most %d references per call)", kPixRefs);
  if (n_refs == 0) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  FrameSlot& cur = c->slots[slot];
  if (!cur.has_obj) return fail(KHR_ESTATE, "the frame has no object image (run the object detector first)");
  const size_t npx = c->cfg.max_frame_pixels;
  const size_t words = npx + kPixRefs + static_cast<size_t>(kPixRefs) * (static_cast<size_t>(max_id) + 1);
  if (c->d_pix_scratch.count() < words) {
    if (c->d_pix_scratch) HIP_TRY(hipStreamSynchronize(c->stream));
    KHR_TRY(c->d_pix_scratch.reserve(words));
  }
  uint32_t* const d_mask = c->d_pix_scratch;
  uint32_t* const d_np = d_mask + npx;
  uint32_t* const d_inter = d_np + kPixRefs;
  const int n = cur.sensor.width * cur.sensor.height;
  // the object image of this frame and the id images of the source frames come from the auxiliary stream
  HIP_TRY(hipEventRecord(c->ev_aux_done, c->aux_stream));
  HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_aux_done, 0));
  HIP_TRY(hipMemsetAsync(d_mask, 0, words * sizeof(uint32_t), c->stream));
  PixCamera cam{};
  for (int k = 0; k < 12; ++k) cam.T[k] = cur.meta.world_T_sensor[k];
  cam.fx = cur.sensor.fx; cam.fy = cur.sensor.fy; cam.cx = cur.sensor.cx; cam.cy = cur.sensor.cy;
  cam.W = cur.sensor.width; cam.H = cur.sensor.height;
  // one pass per distinct (slot, image) among the references
  std::vector<char> done(static_cast<size_t>(n_refs), 0);
  for (int a = 0; a < n_refs; ++a) {
    if (done[a]) continue;
    const khr_pixel_ref& ra = refs[a];
    if (!validSlot(c, ra.slot) || (ra.which != 0 && ra.which != 1)) return fail(KHR_EINVAL, "bad reference %d", a);
    FrameSlot& src = c->slots[ra.slot];
    if (src.sensor.width != cur.sensor.width || src.sensor.height != cur.sensor.height)
      return fail(KHR_EINVAL, "reference frames must have the current frame's image size");
    PixRefs pr{};
    for (int b = a; b < n_refs; ++b)
      if (!done[b] && refs[b].slot == ra.slot && refs[b].which == ra.which) {
        pr.id[pr.n] = refs[b].id;
        pr.bit[pr.n] = b;
        ++pr.n;
        done[b] = 1;
      }
    const DevFrame fs = makeDevFrame(c, src);
    hipLaunchKernelGGL(k_pix_reproject, dim3(gridFor(n)), dim3(256), 0, c->stream, fs, ra.which == 0 ? src.dyn : src.obj, pr, cam,
                       d_mask, d_np);
  }
  hipLaunchKernelGGL(k_pix_intersect, dim3(gridFor(n)), dim3(256), 0, c->stream, cur.obj, d_mask, n, n_refs, max_id, d_inter);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(n_points, d_np, sizeof(uint32_t) * n_refs, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(inter, d_inter, sizeof(uint32_t) * static_cast<size_t>(n_refs) * (static_cast<size_t>(max_id) + 1),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

int khr_forward_instances(khr_ctx* c, int slot, float max_range, const int32_t* background_ids, int n_background, int max_id,
                          khr_cluster* out) {
  if (!c || !validSlot(c, slot)) return fail(KHR_EINVAL, "bad slot");
  if (!out || max_id < 1 || max_id > 65535 || n_background < 0 || (n_background > 0 && !background_ids)) return fail(KHR_EINVAL, "bad argument");
  FrameSlot& s = c->slots[slot];
  if (!s.has_label) return fail(KHR_ESTATE, "the frame has no label image to forward");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n_acc = static_cast<size_t>(max_id) + 1;
  const size_t bytes = sizeof(ObjAcc) * n_acc + 16 + sizeof(int32_t) * static_cast<size_t>(std::max(n_background, 1));
  if (c->d_inst.count() < bytes) {
    if (c->d_inst) HIP_TRY(hipStreamSynchronize(c->stream));
    KHR_TRY(c->d_inst.reserve(bytes));
  }
  ObjAcc* const d_acc = reinterpret_cast<ObjAcc*>(c->d_inst.get());
  uint32_t* const d_flags = reinterpret_cast<uint32_t*>(c->d_inst + sizeof(ObjAcc) * n_acc);
  int32_t* const d_bg = reinterpret_cast<int32_t*>(c->d_inst + sizeof(ObjAcc) * n_acc + 16);
  if (n_background) HIP_TRY(hipMemcpyAsync(d_bg, background_ids, sizeof(int32_t) * n_background, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_inst_clear, dim3(gridFor(n_acc)), dim3(256), 0, c->stream, d_acc, static_cast<int>(n_acc), d_flags);
  const DevFrame f = makeDevFrame(c, s);
  const int tiles = ((f.W + kObjTile - 1) / kObjTile) * ((f.H + kObjTile - 1) / kObjTile);
  hipLaunchKernelGGL(k_inst_forward, dim3(tiles), dim3(1024), 0, c->stream, f, s.obj, max_range, d_bg, n_background, max_id, d_acc, d_flags);
  HIP_TRY(hipGetLastError());
  std::vector<ObjAcc> acc(n_acc);
  uint32_t flags = 0;
  HIP_TRY(hipMemcpyAsync(acc.data(), d_acc, sizeof(ObjAcc) * n_acc, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  s.has_obj = true;
  if (c->obj_cv_slot == slot) c->obj_cv_slot = -1;
  s.objects_done = true;
  s.sem_clusters.clear();
  if (flags & 1u) return fail(KHR_EINVAL, "an instance id of the label image is outside 1..%d", max_id);
  int present = 0;
  for (size_t id = 0; id < n_acc; ++id) {
    khr_cluster k{};
    const ObjAcc& a = acc[id];
    k.id = static_cast<int32_t>(id);
    k.num_pixels_listed = a.n_pixels;
    k.num_pixels_painted = a.n_pixels;
    k.semantic_id = static_cast<int32_t>(id);
    if (a.n_pixels) {
      ++present;
      for (int d = 0; d < 3; ++d) {
        k.bbox_min[d] = orderedToFloat(a.bmin[d]);
        k.bbox_max[d] = orderedToFloat(a.bmax[d]);
        k.centroid[d] = a.sum[d] / static_cast<float>(a.n_pixels);
      }
    }
    out[id] = k;
  }
  return present;
}

// marching cubes on stream `st`: the context's (khr_generate_mesh), or khr_process_frame's mesh stream beside the tracking pass
static int generateMesh(khr_ctx* c, hipStream_t st, int only_mesh_updated, int clear_flag) {
  HIP_TRY(hipSetDevice(c->device));
  DevMap& m = c->m;
  const size_t cap = m.capacity;
  ScopedTimer tm(c, 5, st);
  uint32_t* const n_work = c->d_mesh_nwork + (c->mesh_nwork_par ? 4 : 0);
  c->mesh_nwork_last = c->mesh_nwork_par ? 4 : 0;
  c->mesh_nwork_par ^= 1;
  hipLaunchKernelGGL(k_mesh_prepare, dim3(gridFor(cap + 1)), dim3(256), 0, st, m, only_mesh_updated ? BLK_MESH_UPDATED : 0u,
                     c->d_work, n_work, c->d_mesh_nwork + (c->mesh_nwork_par ? 4 : 0), c->d_regen, c->d_mesh_count, c->d_mesh_old_off);
  MeshBuffers src = c->mesh[c->mesh_cur], dst = c->mesh[c->mesh_cur ^ 1];
  RemoteMeshHalo rmh{};
  if (c->mh_n) {
    rmh.recs = c->mh_view;
    rmh.ht_keys = c->d_mh_keys;
    rmh.ht_vals = c->d_mh_vals;
    rmh.ht_mask = c->mh_mask;
    if (c->mh_compact) {
      rmh.ht_keys = c->d_mh2_keys;
      rmh.ht_offs = c->d_mh2_offs;
    }
  }
  const uint32_t maxv = static_cast<uint32_t>(std::min<uint64_t>(c->cfg.max_mesh_vertices, 0xfffffff0ull));
  int rc = dispatchVps(c, [&](auto vps) {
    constexpr int V = decltype(vps)::value;
    KHR_LAUNCH_TIMED_ON(8, st, (k_marching_cubes<V, false>), dim3(kStreamGrid), dim3(256), m, c->p, c->d_work,
                     n_work, c->d_mesh_count, c->d_mesh_offset, dst, clear_flag, maxv, rmh, 0xffffffffu,
                     static_cast<const uint8_t*>(nullptr), MeshBuffers{}, static_cast<const uint32_t*>(nullptr));
    size_t tb = c->cub_temp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_cub_temp, tb, c->d_mesh_count, c->d_mesh_offset,
                                             static_cast<int>(cap + 1), st));
    // no host round trip: the capacity check happens on the device (C_MESH_OVERFLOW), totals are read lazily
    // emit pass + the copy of the kept blocks' vertices in ONE launch (the trailing kMoveWgs workgroups copy)
    // (no copy workgroups for the first mesh of an emptied map: no block holds vertices yet)
    const uint32_t kMoveWgs = c->mesh_made ? 1024u : 0u;
    KHR_LAUNCH_TIMED_ON(9, st, (k_marching_cubes<V, true>), dim3(kStreamGrid + kMoveWgs), dim3(256), m, c->p, c->d_work,
                     n_work, c->d_mesh_count, c->d_mesh_offset, dst, clear_flag, maxv, rmh, static_cast<uint32_t>(kStreamGrid),
                     static_cast<const uint8_t*>(c->d_regen), src, static_cast<const uint32_t*>(c->d_mesh_old_off));
    return KHR_OK;
  });
  if (rc) return rc;
  c->mesh_cur ^= 1;
  c->mesh_stale = true;
  c->mesh_made = true;
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

int khr_generate_mesh(khr_ctx* c, int only_mesh_updated, int clear_flag) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  return generateMesh(c, c->stream, only_mesh_updated, clear_flag);
}

// archival kernels; no host round trip: the hash table / free list rebuild is conditional on the device
// the archival's list ahead of the archival (khr_process_frame at output frames, behind the tracking pass)
static int removedPublishLaunch(khr_ctx* c) {
  if (!c->h_removed_early) {
    if (c->h_removed_early.alloc(c->m.capacity))
      return fail(KHR_ENOMEM, "page-locked list of archived blocks (%zu bytes)", sizeof(int4) * static_cast<size_t>(c->m.capacity));
    int rc = devAlloc(c, &c->d_removed_early_n, 2);
    if (rc) return rc;
  }
  if (++c->removed_early_ticket == 0) ++c->removed_early_ticket;
  hipLaunchKernelGGL(k_removed_publish, dim3(gridFor(c->m.capacity)), dim3(256), 0, c->stream, c->m, c->h_removed_early.dev(),
                     c->d_removed_early_n, c->h_pinned.dev() + 10, c->removed_early_ticket);
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

// counter_zeroed: k_removed_publish, queued before on the same stream, has zeroed the removed counter; clear_mask: block flags the
// surviving blocks lose in the same pass (khr_process_frame's output stage: BLK_UPDATED)
static int resetInactiveLaunch(khr_ctx* c, bool counter_zeroed = false, uint32_t clear_mask = 0u) {
  DevMap& m = c->m;
  c->removed_early = false;
  if (!counter_zeroed) HIP_TRY(hipMemsetAsync(&m.counters[C_N_REMOVED], 0, sizeof(uint32_t), c->stream));
  int rc = dispatchVps(c, [&](auto vps) {
    hipLaunchKernelGGL((k_reset_inactive<decltype(vps)::value>), dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m, c->d_removed, clear_mask);
    return KHR_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_rehash_clear, dim3(gridFor(static_cast<size_t>(m.ht_mask) + 1)), dim3(256), 0, c->stream, m);
  hipLaunchKernelGGL(k_rehash, dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m);
  c->host_index_valid = false, ++c->map_gen;
  c->removed_pending = true;
  HIP_TRY(hipGetLastError());
  return KHR_OK;
}

static int fetchRemoved(khr_ctx* c, int32_t* removed, int64_t cap, int64_t* n_removed) {
  if (c->removed_early) {  // the last archival was queued by khr_process_frame: its list was published behind the tracking pass
    const int rcw = waitTicket(c, 11, c->removed_early_ticket, "the list of archived blocks");
    if (rcw) return rcw;
    const uint32_t ne = c->h_pinned[10];
    c->removed_pending = false;
    if (n_removed) *n_removed = ne;
    if (ne && removed && cap > 0) {
      std::vector<int4> tmp(c->h_removed_early.get(), c->h_removed_early + ne);
      std::sort(tmp.begin(), tmp.end(), [](const int4& a, const int4& b) {
        return a.x != b.x ? a.x < b.x : (a.y != b.y ? a.y < b.y : a.z < b.z);
      });
      for (int64_t i = 0; i < std::min<int64_t>(ne, cap); ++i) {
        removed[3 * i] = tmp[i].x;
        removed[3 * i + 1] = tmp[i].y;
        removed[3 * i + 2] = tmp[i].z;
      }
    }
    return KHR_OK;
  }
  uint32_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, &c->m.counters[C_N_REMOVED], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->removed_pending = false;
  if (n_removed) *n_removed = n;
  if (n && removed && cap > 0) {
    std::vector<int4> tmp(n);
    HIP_TRY(hipMemcpy(tmp.data(), c->d_removed, sizeof(int4) * n, hipMemcpyDeviceToHost));
    std::sort(tmp.begin(), tmp.end(), [](const int4& a, const int4& b) {
      return a.x != b.x ? a.x < b.x : (a.y != b.y ? a.y < b.y : a.z < b.z);
    });
    for (int64_t i = 0; i < std::min<int64_t>(n, cap); ++i) {
      removed[3 * i] = tmp[i].x;
      removed[3 * i + 1] = tmp[i].y;
      removed[3 * i + 2] = tmp[i].z;
    }
  }
  return KHR_OK;
}

int khr_mesh_halo_requests(khr_ctx* c, void* keys_out, int64_t cap, int only_mesh_updated, int on_device) {
  if (!c || !keys_out || cap < 1) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  DevMap& m = c->m;
  uint64_t* dst = static_cast<uint64_t*>(keys_out);
  DevTemp holder;
  uint64_t* tmp = nullptr;
  if (!on_device) {
    KHR_TRY(holder.alloc(sizeof(uint64_t) * cap));
    dst = tmp = holder.as<uint64_t>();
  }
  HIP_TRY(hipMemsetAsync(dst, 0, sizeof(uint64_t) * cap, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_mesh_nwork + 1, 0, sizeof(uint32_t) * 2, c->stream));
  hipLaunchKernelGGL(k_list_live, dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m, c->d_work, c->d_mesh_nwork + 1,
                     only_mesh_updated ? BLK_MESH_UPDATED : 0u);
  hipLaunchKernelGGL(k_mesh_halo_requests, dim3(512), dim3(256), 0, c->stream, m, c->p, c->d_work, c->d_mesh_nwork + 1, dst,
                     static_cast<uint32_t>(cap), c->d_mesh_nwork + 2);
  uint32_t n_req = 0;
  HIP_TRY(hipMemcpyAsync(&n_req, c->d_mesh_nwork + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (!on_device) HIP_TRY(hipMemcpyAsync(keys_out, tmp, sizeof(uint64_t) * cap, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_req > cap) return fail(KHR_ENOMEM, "%u mesh halo requests exceed the capacity %lld", n_req, static_cast<long long>(cap));
  return static_cast<int>(n_req);
}

int khr_mesh_halo_export(khr_ctx* c, const void* requests, int64_t n_requests, void* records, int64_t cap_records, int on_device) {
  if (!c || !records || cap_records < 1 || n_requests < 0 || (!requests && n_requests > 0)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  DevMap& m = c->m;
  const size_t words = c->p.vps == 16 ? MeshHalo<16>::kWords : MeshHalo<8>::kWords;
  const size_t bytes = static_cast<size_t>(cap_records) * words * 4;
  const uint64_t* req = static_cast<const uint64_t*>(requests);
  uint32_t* dst = static_cast<uint32_t*>(records);
  DevTemp req_holder, rec_holder;
  uint32_t* rec_tmp = nullptr;
  if (!on_device) {
    if (n_requests) {
      KHR_TRY(req_holder.alloc(sizeof(uint64_t) * n_requests));
      HIP_TRY(hipMemcpyAsync(req_holder.get(), requests, sizeof(uint64_t) * n_requests, hipMemcpyHostToDevice, c->stream));
      req = req_holder.as<uint64_t>();
    }
    KHR_TRY(rec_holder.alloc(bytes));
    dst = rec_tmp = rec_holder.as<uint32_t>();
  }
  HIP_TRY(hipMemsetAsync(c->d_mh_flag, 0, m.capacity, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_mesh_nwork + 3, 0, sizeof(uint32_t), c->stream));
  if (n_requests)
    hipLaunchKernelGGL(k_mesh_halo_mark, dim3(gridFor(n_requests)), dim3(256), 0, c->stream, m, c->p, req,
                       static_cast<uint32_t>(n_requests), c->d_mh_flag);
  hipLaunchKernelGGL(k_list_marked, dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m, c->d_mh_flag, c->d_new, c->d_mesh_nwork + 3);
  int rc = dispatchVps(c, [&](auto vps) {
    hipLaunchKernelGGL((k_mesh_halo_export<decltype(vps)::value>), dim3(static_cast<unsigned>(std::min<int64_t>(cap_records, 2048))),
                       dim3(256), 0, c->stream, m, c->p, c->d_new, c->d_mesh_nwork + 3, dst, static_cast<uint32_t>(cap_records));
    return KHR_OK;
  });
  hipError_t e = hipSuccess;
  uint32_t n_rec = 0;
  if (rc == KHR_OK) e = hipMemcpyAsync(&n_rec, c->d_mesh_nwork + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && rc == KHR_OK && !on_device) e = hipMemcpyAsync(records, rec_tmp, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(KHR_EDEVICE, "mesh halo export failed: %s", hipGetErrorString(e));
  if (rc != KHR_OK) return rc;
  return static_cast<int>(std::min<uint64_t>(n_rec, static_cast<uint64_t>(cap_records)));  // records written (the rest are empty)
}

int khr_mesh_halo_import(khr_ctx* c, const void* records, int64_t n_records, int on_device) {
  if (!c || n_records < 0 || (!records && n_records > 0)) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  c->mh_compact = false;
  if (n_records == 0) {
    c->mh_n = 0;
    return KHR_OK;
  }
  const size_t words = c->p.vps == 16 ? MeshHalo<16>::kWords : MeshHalo<8>::kWords;
  const bool in_place = on_device == 2;  // the records stay in the caller's device buffer (valid until the mesh has been generated)
  uint32_t ht = 1;
  while (ht < static_cast<uint64_t>(n_records) * 4) ht <<= 1;
  if (static_cast<uint64_t>(n_records) > c->mh_cap_total) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_mh_recs.reset(), c->d_mh_keys.reset(), c->d_mh_vals.reset();
    // (in-place imports only need the index; the record copy buffer is allocated by the first copying import)
    KHR_TRY(c->d_mh_keys.alloc(ht));
    KHR_TRY(c->d_mh_vals.alloc(ht));
    c->mh_cap_total = static_cast<uint32_t>(n_records);
  }
  c->mh_mask = ht - 1;  // (a smaller import clears and probes a smaller part of the table)
  const uint32_t* view = static_cast<const uint32_t*>(records);
  if (!in_place) {
    if (!c->d_mh_recs) KHR_TRY(c->d_mh_recs.alloc(static_cast<size_t>(c->mh_cap_total) * words));
    HIP_TRY(hipMemcpyAsync(c->d_mh_recs, records, static_cast<size_t>(n_records) * words * 4,
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    view = c->d_mh_recs;
  }
  c->mh_view = view;
  HIP_TRY(hipMemsetAsync(c->d_mh_keys, 0xff, sizeof(uint64_t) * (static_cast<size_t>(c->mh_mask) + 1), c->stream));
  hipLaunchKernelGGL(k_mesh_halo_import, dim3(gridFor(n_records)), dim3(256), 0, c->stream, view,
                     static_cast<uint32_t>(n_records), static_cast<int>(words), c->cfg.rank, c->cfg.world_size, c->d_mh_keys,
                     c->d_mh_vals, c->mh_mask);
  HIP_TRY(hipGetLastError());
  if (!on_device) HIP_TRY(hipStreamSynchronize(c->stream));
  c->mh_n = static_cast<uint32_t>(n_records);
  return KHR_OK;
}

// ---- compact mesh halo (round 5) -------------------------------------------------------------------------------------
// The layout both sides derive from the all-gathered request headers: answers travel owner -> requester only, grouped by
// requester, inside a group by relation (1 .. 7) in request order.  Counts and displacements are in u32 words.
int khr_mesh_halo_plan(int world, int rank, int vps, const uint64_t* headers, uint64_t* sendcounts, uint64_t* sdispls,
                       uint64_t* recvcounts, uint64_t* rdispls) {
  if (world < 1 || world > kMeshHaloMaxWorld || rank < 0 || rank >= world || (vps != 8 && vps != 16) || !headers || !sendcounts || !sdispls ||
      !recvcounts || !rdispls)
    return fail(KHR_EINVAL, "khr_mesh_halo_plan: bad argument (world <= %d)", kMeshHaloMaxWorld);
  uint64_t so = 0, ro = 0;
  for (int q = 0; q < world; ++q) {
    uint64_t sw = 0, rw = 0;
    for (int sel = 1; sel < 8; ++sel) {
      const uint64_t aw = static_cast<uint64_t>(meshHaloAnswerWords(sel, vps));
      sw += headers[static_cast<size_t>(q) * 8 * world + static_cast<size_t>(rank) * 8 + sel] * aw;     // q asked me
      rw += headers[static_cast<size_t>(rank) * 8 * world + static_cast<size_t>(q) * 8 + sel] * aw;     // I asked q
    }
    sendcounts[q] = sw;
    sdispls[q] = so;
    so += sw;
    recvcounts[q] = rw;
    rdispls[q] = ro;
    ro += rw;
  }
  return KHR_OK;
}

int khr_mesh_halo_requests_sorted(khr_ctx* c, void* requests_device, int64_t cap, int only_mesh_updated) {
  if (!c || !requests_device || cap < 1) return fail(KHR_EINVAL, "bad argument");
  const int world = c->cfg.world_size;
  if (world > kMeshHaloMaxWorld) return fail(KHR_EINVAL, "the compact mesh halo is laid out for at most %d ranks", kMeshHaloMaxWorld);
  HIP_TRY(hipSetDevice(c->device));
  DevMap& m = c->m;
  constexpr int NB = 8 * kMeshHaloMaxWorld;
  if (!c->d_mh2_scratch) KHR_TRY(c->d_mh2_scratch.alloc(3 * NB + 1));
  uint32_t* const cnt = c->d_mh2_scratch;
  uint32_t* const base = cnt + NB;
  uint32_t* const cursor = base + NB;
  uint32_t* const total = cursor + NB;
  uint64_t* const req = static_cast<uint64_t*>(requests_device);
  const uint32_t hw = 8u * static_cast<uint32_t>(world);
  HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * NB, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_mesh_nwork + 1, 0, sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_list_live, dim3(gridFor(m.capacity)), dim3(256), 0, c->stream, m, c->d_work, c->d_mesh_nwork + 1,
                     only_mesh_updated ? BLK_MESH_UPDATED : 0u);
  hipLaunchKernelGGL((k_mesh_halo_req_sorted<false>), dim3(512), dim3(256), 0, c->stream, m, c->p, c->d_work, c->d_mesh_nwork + 1, cnt,
                     base, cursor, req, hw, static_cast<uint32_t>(cap));
  hipLaunchKernelGGL(k_mesh_halo_req_plan, dim3(1), dim3(64), 0, c->stream, cnt, base, cursor, req, world, total);
  hipLaunchKernelGGL((k_mesh_halo_req_sorted<true>), dim3(512), dim3(256), 0, c->stream, m, c->p, c->d_work, c->d_mesh_nwork + 1, cnt,
                     base, cursor, req, hw, static_cast<uint32_t>(cap));
  uint32_t n_req = 0;
  HIP_TRY(hipMemcpyAsync(&n_req, total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (n_req > cap) return fail(KHR_ENOMEM, "%u mesh halo requests exceed the capacity %lld", n_req, static_cast<long long>(cap));
  return static_cast<int>(n_req);
}

namespace {
// exclusive prefix of one rank's header in bucket order (owner major, relation minor)
uint64_t bucketBase(const uint64_t* header, int owner, int sel) {
  uint64_t b = 0;
  for (int i = 1; i < owner * 8 + sel; ++i) b += header[i];  // (word 0 carries the total, not a bucket)
  return b;
}
}  // namespace

int khr_mesh_halo_answer(khr_ctx* c, const void* all_requests_device, int64_t cap, const uint64_t* headers, void* records_device,
                         int64_t cap_words) {
  if (!c || !all_requests_device || cap < 1 || !headers || !records_device || cap_words < 1) return fail(KHR_EINVAL, "bad argument");
  const int world = c->cfg.world_size, rank = c->cfg.rank;
  if (world > kMeshHaloMaxWorld) return fail(KHR_EINVAL, "the compact mesh halo is laid out for at most %d ranks", kMeshHaloMaxWorld);
  HIP_TRY(hipSetDevice(c->device));
  const int vps = c->p.vps;
  const uint64_t stride = 8ull * world + static_cast<uint64_t>(cap);
  MeshHaloRuns runs{};
  uint64_t words = 0, items = 0;
  for (int q = 0; q < world; ++q) {
    const uint64_t* hq = headers + static_cast<size_t>(q) * 8 * world;
    if (hq[0] > static_cast<uint64_t>(cap)) return fail(KHR_ENOMEM, "rank %d listed %llu mesh halo requests, capacity %lld", q,
                                                        static_cast<unsigned long long>(hq[0]), static_cast<long long>(cap));
    for (int sel = 1; sel < 8; ++sel) {
      const uint64_t n = hq[rank * 8 + sel];
      if (!n) continue;
      const uint32_t r = runs.n_runs++;
      runs.first[r] = static_cast<uint32_t>(items);
      runs.req_off[r] = static_cast<uint32_t>(static_cast<uint64_t>(q) * stride + 8ull * world + bucketBase(hq, rank, sel));
      runs.rec_off[r] = static_cast<uint32_t>(words);
      runs.sel[r] = static_cast<uint8_t>(sel);
      // (the runs carry 32-bit word offsets, 0xffffffff is the "no answer" mark of the adopted table: ADVICE r05)
      if (static_cast<uint64_t>(q) * stride + 8ull * world + bucketBase(hq, rank, sel) >= 0xffffffffull)
        return fail(KHR_EINVAL, "mesh halo: the gathered request lists exceed 2^32 - 1 entries (capacity %lld x %d ranks)", static_cast<long long>(cap), world);
      items += n;
      words += n * static_cast<uint64_t>(meshHaloAnswerWords(sel, vps));
      if (words >= 0xffffffffull || items >= 0xffffffffull)
        return fail(KHR_ENOMEM, "mesh halo: the answers of this output exceed 2^32 - 1 words");
    }
  }
  runs.first[runs.n_runs] = static_cast<uint32_t>(items);
  runs.n_items = static_cast<uint32_t>(items);
  if (words > static_cast<uint64_t>(cap_words))
    return fail(KHR_ENOMEM, "the mesh halo answers of this output need %llu words, the buffer holds %lld", static_cast<unsigned long long>(words),
                static_cast<long long>(cap_words));
  if (!items) return 0;
  const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((items + 3) / 4, 4096));
  int rc = dispatchVps(c, [&](auto vps_c) {
    hipLaunchKernelGGL((k_mesh_halo_answer<decltype(vps_c)::value>), dim3(grid), dim3(256), 0, c->stream, c->m, c->p,
                       static_cast<const uint64_t*>(all_requests_device), runs, static_cast<uint32_t*>(records_device));
    return KHR_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return static_cast<int>(std::min<uint64_t>(items, 0x7fffffffull));
}

int khr_mesh_halo_adopt(khr_ctx* c, const void* own_requests_device, const uint64_t* own_header, const void* records_device,
                        const uint64_t* rdispls) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  c->mh_compact = false;
  c->mh_n = 0;
  if (!own_requests_device) return KHR_OK;  // (forget the last output's answers)
  if (!own_header || !records_device || !rdispls) return fail(KHR_EINVAL, "bad argument");
  const int world = c->cfg.world_size;
  if (world > kMeshHaloMaxWorld) return fail(KHR_EINVAL, "the compact mesh halo is laid out for at most %d ranks", kMeshHaloMaxWorld);
  HIP_TRY(hipSetDevice(c->device));
  const int vps = c->p.vps;
  MeshHaloRuns runs{};
  uint64_t items = 0;
  for (int r = 0; r < world; ++r) {
    uint64_t words = rdispls[r];
    for (int sel = 1; sel < 8; ++sel) {
      const uint64_t n = own_header[r * 8 + sel];
      if (!n) continue;
      const uint32_t k = runs.n_runs++;
      runs.first[k] = static_cast<uint32_t>(items);
      runs.req_off[k] = static_cast<uint32_t>(8ull * world + bucketBase(own_header, r, sel));
      runs.rec_off[k] = static_cast<uint32_t>(words);
      runs.sel[k] = static_cast<uint8_t>(sel);
      items += n;
      words += n * static_cast<uint64_t>(meshHaloAnswerWords(sel, vps));
      // (32-bit word offsets into the receive buffer, 0xffffffff marks "no answer": a buffer of rec_cap x world >= 2^32 words would wrap)
      if (words >= 0xffffffffull || items >= 0xffffffffull)
        return fail(KHR_ENOMEM, "mesh halo: the answers received from rank %d end beyond word 2^32 - 1 of the receive buffer", r);
    }
  }
  runs.first[runs.n_runs] = static_cast<uint32_t>(items);
  runs.n_items = static_cast<uint32_t>(items);
  if (!items) return KHR_OK;
  uint32_t ht = 1024;
  while (ht < items * 2) ht <<= 1;
  if (ht > c->mh2_ht) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->mh2_ht = 0;
    c->d_mh2_keys.reset(), c->d_mh2_offs.reset();  // (both go before either comes back)
    KHR_TRY(c->d_mh2_keys.reserve(ht));
    KHR_TRY(c->d_mh2_offs.reserve(8 * static_cast<size_t>(ht)));
    c->mh2_ht = ht;
  }
  HIP_TRY(hipMemsetAsync(c->d_mh2_keys, 0xff, sizeof(uint64_t) * ht, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_mh2_offs, 0xff, sizeof(uint32_t) * 8 * static_cast<size_t>(ht), c->stream));
  hipLaunchKernelGGL(k_mesh_halo_adopt, dim3(gridFor(items)), dim3(256), 0, c->stream, static_cast<const uint64_t*>(own_requests_device), runs,
                     static_cast<const uint32_t*>(records_device), vps, c->d_mh2_keys, c->d_mh2_offs, ht - 1);
  HIP_TRY(hipGetLastError());
  c->mh_view = static_cast<const uint32_t*>(records_device);
  c->mh_mask = ht - 1;
  c->mh_n = static_cast<uint32_t>(items);
  c->mh_compact = true;
  return KHR_OK;
}

int khr_reset_inactive(khr_ctx* c, int32_t* removed, int64_t cap, int64_t* n_removed) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (n_removed) *n_removed = 0;
  if (!c->cfg.with_tracking) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  int rc = resetInactiveLaunch(c);
  if (rc) return rc;
  if (!removed && !n_removed) return KHR_OK;  // asynchronous form; fetch later with khr_last_removed
  return fetchRemoved(c, removed, cap, n_removed);
}

int khr_last_removed(khr_ctx* c, int32_t* removed, int64_t cap, int64_t* n_removed) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  return fetchRemoved(c, removed, cap, n_removed);
}

constexpr size_t kMaxAhead = 2;
// drop the frames handed over by khr_ingest_ahead[_host] that will not be processed (their leases, a pending object-detector request)
static void cancelAhead(khr_ctx* c) {
  for (const auto& e : c->ahead_q) {
    c->slot_leases[e.slot].fetch_sub(1, std::memory_order_acq_rel);
    c->slots[e.slot].valid = false;  // (converted, but nobody may integrate it any more)
    if (c->obj_pending_slot == e.slot) c->obj_pending_slot = -1;
    if (e.host && c->ev_ahead_h2d[e.ev]) hipEventSynchronize(c->ev_ahead_h2d[e.ev]);  // (the caller owns its buffers again)
  }
  c->ahead_q.clear();
}

// is `p` what the caller says it is?  where = 1: device memory (or managed), 0: page-locked host memory
static bool pointerIs(const void* p, int where) {
  if (!p) return true;
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // (pageable host memory: "invalid value")
    return false;
  }
  if (where == 1) return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeUnified;
  return at.type == hipMemoryTypeHost;
}

static int ingestAhead(khr_ctx* c, const khr_sensor* sensor, const khr_frame* frame, int on_device) {
  if (!c || !sensor || !frame) return fail(KHR_EINVAL, "null argument");
  if (c->ahead_q.size() >= kMaxAhead)
    return fail(KHR_ESTATE, "%zu frames handed over by khr_ingest_ahead are still waiting for khr_process_frame (khr_ingest_cancel drops them)", c->ahead_q.size());
  // the same conditions as the early ingest inside khr_process_frame, plus a ring with slots to spare: the slot of the frame
  // being processed and the one before it may still be read
  const int next = peekSlot(c);
  if (!c->cfg.with_tracking || c->slots.size() < 3 + c->ahead_q.size() || next < 0 || next == c->last_frame_slot) return KHR_ENOTFOUND;
  HIP_TRY(hipSetDevice(c->device));
  // the buffers are read asynchronously: they have to be what the entry point says they are
  if (!pointerIs(frame->depth, on_device) || !pointerIs(frame->color, on_device) || !pointerIs(frame->label, on_device))
    return fail(KHR_EINVAL, on_device ? "khr_ingest_ahead: the frame's buffers must be device memory" : "khr_ingest_ahead_host: the frame's buffers must be page-locked host memory (hipHostMalloc / hipHostRegister)");
  const int evi = c->ahead_ev_next;
  for (const auto& e : c->ahead_q)
    if (e.ev == evi) return fail(KHR_ESTATE, "look-ahead event ring out of step");
  // a host frame is converted on the host-to-device stream itself, right behind its planes: on the auxiliary stream the conversion
  // -- which waits ~205 us for a 720p frame's planes -- would sit in front of the CURRENT frame's object-detector kernels, whose
  // results the host waits for at the end of khr_process_frame (seen in the rocprofv3 timeline: main stream idle for 250 us)
  hipStream_t conv_stream = c->aux_stream;
  if (!on_device) {
    if (!c->h2d_stream) KHR_TRY(createStream(c, c->h2d_stream));
    conv_stream = c->h2d_stream;
  }
  IngestOpts opts;
  opts.stream = conv_stream;
  opts.pinned = !on_device;
  opts.h2d_event = &c->ev_ahead_h2d[evi];
  const int slot = uploadFrame(c, sensor, frame, on_device, opts);
  if (slot < 0) return slot;
  auto undo = [&](int rc) {  // nothing published yet: the slot simply is not a frame
    c->slots[slot].valid = false;
    if (!on_device && c->ev_ahead_h2d[evi]) hipEventSynchronize(c->ev_ahead_h2d[evi]);
    return rc;
  };
  if (c->ev_ahead[evi].ensure()) return undo(fail(KHR_EDEVICE, "hipEventCreate failed"));
  if (hipEventRecord(c->ev_ahead[evi], conv_stream) != hipSuccess) return undo(fail(KHR_EDEVICE, "hipEventRecord failed"));
  if (on_device) c->slots[slot].aux_seq = ++c->aux_seq_issued;
  // The object detector only reads the frame: its kernels are queued right behind the conversion.  They then run beside the
  // current frame's tracking pass and the next frame's pixel / allocation / culling kernels -- all of them small -- instead of
  // beside the next frame's update kernel, whose persistent grid fills every CU's register file: the two cannot share a CU,
  // and whichever starts second waits for the other (~55 us of the main stream per frame, profiles/r04_kernel_trace_frames_s2.txt).
  // Queued BEFORE the slot is published as handed over: a failure here leaves no state behind.  Only when no other
  // request of the detector is outstanding (its result block is single): a second frame in the look-ahead gets its detector
  // kernels from its own khr_process_frame call -- and only for the frame that will be processed NEXT (empty queue): the older frame's
  // khr_process_frame call would otherwise launch its own request over this one, which then ran twice.
  // Not for host frames: their planes are still travelling, and the auxiliary stream -- in order -- would hold the CURRENT frame's
  // detector kernels, queued later by its khr_process_frame call, behind that wait.
  if (on_device && c->obj_configured && c->obj_pending_slot < 0 && c->ahead_q.empty()) {
    const int rco = objectsLaunch(c, slot);
    if (rco) {
      if (c->obj_pending_slot == slot) c->obj_pending_slot = -1;
      return undo(rco);
    }
  }
  c->slot_leases[slot].fetch_add(1, std::memory_order_acq_rel);  // (nobody else may take the slot before it is processed)
  c->ahead_q.push_back({slot, evi, !on_device});
  c->ahead_ev_next ^= 1;
  return slot;
}

int khr_ingest_ahead(khr_ctx* c, const khr_sensor* sensor, const khr_frame* frame) { return ingestAhead(c, sensor, frame, 1); }
int khr_ingest_ahead_host(khr_ctx* c, const khr_sensor* sensor, const khr_frame* frame) { return ingestAhead(c, sensor, frame, 0); }
int khr_ingest_cancel(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (c->ahead_q.empty()) return KHR_ENOTFOUND;
  cancelAhead(c);
  return KHR_OK;
}

static int snapshotUpdated(khr_ctx* c, hipStream_t st, uint32_t fields, int64_t cap_blocks, khr_snapshot** out);  // (with the snapshots, below)

// One call per frame.  What it chooses for its own frame -- the ingest's stream, the deferred fold, the deferred cluster summaries, the
// mesh kernels' fork point and stream, the snapshot's stream -- goes to the functions the step-wise entry points use as arguments; the
// context only keeps what lives between calls.
int khr_process_frame(khr_ctx* c, const khr_sensor* sensor, const khr_frame* frame, int on_device, uint32_t flags,
                      int* n_clusters) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  HT("pf_enter");
  if (n_clusters) *n_clusters = 0;
  const bool motion = (flags & KHR_PF_MOTION) != 0;
  const bool objects = (flags & KHR_PF_OBJECTS) != 0;
  // KHR_PF_INPUT_READY (the caller's buffers are complete): the ingest only writes the frame slot, so it runs on the
  // auxiliary stream: queued as soon as this call starts, it
  // executes beside the tail of the previous frame (tracking, ever-free, output) instead of after it.  Only with the
  // motion detector on: its per-frame host wait is what keeps the host from queueing frames whose slot an earlier
  // frame still reads.  The per-frame counter reset moves to the first main-stream kernel (k_motion_pixels).
  // Not when the ring hands back the slot of the frame queued just before (everything else is retained): that frame's
  // update / summary / tracking kernels may still be running on the main stream, and the auxiliary stream is not ordered
  // behind them -- the ingest then stays on the main stream.
  const bool ahead = (flags & KHR_PF_INGESTED) != 0;
  if (ahead && (c->ahead_q.empty() || !frame || !motion || !(flags & KHR_PF_INPUT_READY) ||
                c->slots[c->ahead_q.front().slot].meta.timestamp_ns != frame->timestamp_ns)) {
    // a rejected call must not leave the context wedged: the handed-over frames are dropped with their leases, the
    // caller processes its frame the usual way
    cancelAhead(c);
    return fail(KHR_ESTATE, "KHR_PF_INGESTED: the oldest frame handed over by khr_ingest_ahead does not carry this stamp (or flags are missing); the handed-over frames were dropped");
  }
  if (!ahead && !c->ahead_q.empty()) return fail(KHR_ESTATE, "the frames handed over by khr_ingest_ahead have to be processed first (khr_ingest_cancel drops them)");
  const bool pinned_in = !on_device && (flags & KHR_PF_INPUT_PINNED) != 0;
  if (pinned_in && !ahead && frame && (!pointerIs(frame->depth, 0) || !pointerIs(frame->color, 0) || !pointerIs(frame->label, 0)))
    return fail(KHR_EINVAL, "KHR_PF_INPUT_PINNED: the frame's buffers must be page-locked host memory (hipHostMalloc / hipHostRegister)");
  // whatever happens below: the deferred fold of the update kernel's item records does not outlive this call, and a
  // pinned input's copy has finished when the call returns (the caller then owns its buffers again)
  struct Leave {
    khr_ctx* c;
    bool ok = false;
    ~Leave() {
      if (!ok && c->fold_pending) {  // an error between the update launch and the tracking pass: fold now, nobody else will
        hipLaunchKernelGGL(k_fuse_fold, dim3((c->m.capacity + 255) / 256), dim3(256), 0, c->stream, c->m.blk_flags, c->m.blk_band,
                           &c->m.counters[C_MAX_SLOT], static_cast<const uint32_t*>(nullptr));
        c->fold_pending = false;
      }
      if (c->h2d_pending) {
        hipEventSynchronize(c->ev_h2d);
        c->h2d_pending = false;
      }
      if (own_h2d) hipEventSynchronize(own_h2d);  // (a handed-over host frame: ITS planes, not those of a frame handed over after it)
    }
    hipEvent_t own_h2d = nullptr;
  } leave{c};
  // pinned host frames qualify for the early ingest like device frames: the planes travel on the host-to-device stream, the
  // ingest runs on the second stream behind them.  Their copy REWRITES the slot's raw planes and nothing orders the copy stream
  // behind the slot's last readers: with a ring of two the slot is that of the frame before last, whose tail may still be queued
  //  -- three slots, as the look-ahead requires, or the ingest (and with it the copy) stays ordered on the main stream
  const bool early = ahead || ((flags & KHR_PF_INPUT_READY) && (on_device || pinned_in) && motion && c->cfg.with_tracking &&
                               c->slots.size() >= (pinned_in ? 3u : 2u) && peekSlot(c) != c->last_frame_slot);
  int slot;
  int ahead_ev = 0;
  if (ahead) {
    const khr_ctx::AheadEntry e = c->ahead_q.front();
    c->ahead_q.erase(c->ahead_q.begin());
    slot = e.slot;
    ahead_ev = e.ev;
    if (e.host) leave.own_h2d = c->ev_ahead_h2d[e.ev];
    c->slot_leases[slot].fetch_sub(1, std::memory_order_acq_rel);  // (the look-ahead's own lease)
  } else {
    c->last_ingest_on_aux = early;
    IngestOpts opts;
    opts.stream = early ? static_cast<hipStream_t>(c->aux_stream) : nullptr;
    opts.pinned = pinned_in;
    opts.begin = !early;  // (main-stream ingest: k_begin_integrate folded into it)
    slot = uploadFrame(c, sensor, frame, on_device, opts);
    if (slot < 0) return slot;
  }
  c->last_frame_slot = slot;
  FrameSlot& s = c->slots[slot];
  const DevFrame f = makeDevFrame(c, s);
  int rc = KHR_OK;
  if (ahead) {
    c->begun = false;
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_ahead[ahead_ev], 0));
  } else if (early) {
    c->begun = false;
    s.aux_seq = ++c->aux_seq_issued;
    HIP_TRY(hipEventRecord(c->ev_aux_done, c->aux_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_aux_done, 0));
  }
  if (objects && !c->obj_configured) return fail(KHR_ESTATE, "KHR_PF_OBJECTS needs khr_configure_object_detector");
  if (objects && !early) {  // main-stream ingest: the object kernels (auxiliary stream) start behind it, not behind (1) - (2)
    KHR_TRY(c->ev_ingest.ensure());
    HIP_TRY(hipEventRecord(c->ev_ingest, c->stream));
  }
  // (1) per-pixel motion pass; its seed count comes back asynchronously ...
  if (motion && (rc = motionLaunch(c, s, true, early))) return rc;
  // (2) ... while block allocation / culling, which do not depend on the dynamic mask, keep the GPU busy
  if ((rc = integrateAlloc(c, s, f, 1))) return rc;
  HT("pf_alloc_launched");
  // (2b) object detection kernels (they only read the frame) on the auxiliary stream, queued while the host would
  //      otherwise wait for the seed count: the main stream's next kernels are already in its queue.  Their cluster
  //      records reach the host while the volumetric kernels run, and are looked at in (6)
  if (objects) {
    if (!(ahead && c->obj_pending_slot == slot)) {  // (not already queued by khr_ingest_ahead)
      if (!early) HIP_TRY(hipStreamWaitEvent(c->aux_stream, c->ev_ingest, 0));  // (early: same stream, in order)
      if (ahead) HIP_TRY(hipStreamWaitEvent(c->aux_stream, c->ev_ahead[ahead_ev], 0));  // (a host frame was converted on the copy stream)
      if ((rc = objectsLaunch(c, slot))) return rc;
    }
    HT("pf_objects_launched");
  }
  // (2c) the update kernel, speculatively: most frames have no motion seeds, and for those the dynamic mask is empty and the
  //      update does not depend on anything the host is about to learn.  It is queued now, gated on the device-side seed
  //      counter (k_motion_pixels finished long before it in stream order): no seeds -> it runs; seeds -> it returns at once
  //      and the real launch follows the clustering chain below.  (Before: the main stream idled ~35 us per frame between
  //      the culling pass and the update kernel, for the seed count's trip to the host and the launch's trip back.)
  bool speculated = false;
  size_t spec_timer = static_cast<size_t>(-1), spec_end = 0;
  // the update kernel's item records are folded into the block flags by the tracking pass's first kernel when it follows directly
  const bool tracking = (flags & KHR_PF_TRACKING) && c->cfg.with_tracking;
  const bool defer_fold = tracking;  // (`leave` folds if an error exit comes between the update launch and the tracking pass)
  // (not behind a seed frame: the frame is expected to have seeds, its clustering chain is queued ahead of the count instead)
  if (motion && c->cfg.with_tracking && !mdQueuesAhead(c, mdHooks())) {
    const size_t n_pending = c->pending.size();
    rc = integrateUpdate(c, s, f, 1, 0, -1, defer_fold, nullptr, &c->m.counters[C_N_SEEDS]);
    if (rc) return rc;
    if (c->pending.size() > n_pending) spec_timer = n_pending;  // (first of the launch's timer samples)
    spec_end = c->pending.size();
    speculated = true;
  }
  // (3) host looks at the seed count (clusters only exist when there are seeds)
  bool have_seeds = false;
  int summary_pending = -1;  // largest id of the dynamic clusters whose summaries are queued behind the update kernels
  if (motion) {
    const int nc = motionFinish(c, s, &summary_pending);
    if (nc < 0) return nc;
    if (n_clusters) *n_clusters = nc;
    have_seeds = c->cfg.with_tracking && c->h_pinned[0] != 0;
  }
  HT("pf_motion_done");
  // (4) TSDF / label update with the dynamic mask, tracking + ever-free
  if (speculated && have_seeds && spec_timer != static_cast<size_t>(-1))  // the gated launches did nothing: not samples
    for (size_t i = spec_timer; i < spec_end && i < c->pending.size(); ++i) c->pending[i].which = -1;
  if (!speculated || have_seeds) {
    rc = integrateUpdate(c, s, f, 1, motion ? 1 : 0, -1, defer_fold);
    if (rc) return rc;
  }
  // the dynamic clusters' summaries: nothing on the frame's critical path reads them
  if (summary_pending >= 0 && (rc = clusterSummaryLaunch(c, s, summary_pending))) return rc;
  // Output frames: marching cubes read distance / weight / colour / label / stamps, which the tracking pass does not touch
  // (it writes voxel flags, last_occupied, free bits and -- atomically -- block flags): the mesh kernels are forked onto
  // their own stream behind k_tracking_select (which has folded the update's block flags) and joined before archival.
  const bool mc_fork = (flags & KHR_PF_OUTPUT) && tracking;
  if (mc_fork) {
    if (!c->mc_stream) KHR_TRY(createStream(c, c->mc_stream));
    KHR_TRY(c->ev_mc_fork.ensure());
    KHR_TRY(c->ev_mc_join.ensure());
  }
  if (tracking) {  // (khr_update_tracking, with the mesh kernels' fork point behind k_tracking_select)
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = trackingPhase(c, frame->timestamp_ns, 3, mc_fork ? static_cast<hipEvent_t>(c->ev_mc_fork) : nullptr))) return rc;
  }
  // output frames: which blocks the archival below will drop is decided now (the tracking pass has set the block flags it looks at);
  // their list goes to the host at once, the archival itself has to wait for the mesh kernels and the snapshot
  const bool early_list = (flags & KHR_PF_OUTPUT) && c->cfg.with_tracking;
  if (mc_fork) {
    HIP_TRY(hipStreamWaitEvent(c->mc_stream, c->ev_mc_fork, 0));
    if ((rc = generateMesh(c, c->mc_stream, 1, 1))) return rc;
    HIP_TRY(hipEventRecord(c->ev_mc_join, c->mc_stream));
  }
  HT("pf_update_launched");
  // (5) output cadence (ActiveWindow::extractOutputData, active_window.cpp:217-249 + :169-171)
  if (flags & KHR_PF_OUTPUT) {
    const bool snap = (flags & KHR_PF_SNAPSHOT) != 0;
    if (snap) {
      // cloneUpdated (active_window.cpp:229; between the tracking pass and archival).  The clone (184 MB of plain copies at
      // c3) and marching cubes (a few dependent round trips per block) both only READ the voxel layers and write different
      // things: the clone is forked onto its own stream beside the mesh kernels and joined before archival changes the map
      if (c->pending_snapshot) khr_snapshot_release(c->pending_snapshot);
      c->pending_snapshot = nullptr;
      if (!c->snap_stream) KHR_TRY(createStream(c, c->snap_stream));
      KHR_TRY(c->ev_snap_fork.ensure());
      KHR_TRY(c->ev_snap_join.ensure());
      HIP_TRY(hipEventRecord(c->ev_snap_fork, c->stream));
      HIP_TRY(hipStreamWaitEvent(c->snap_stream, c->ev_snap_fork, 0));
      const int64_t snap_cap = c->cfg.max_snapshot_blocks ? c->cfg.max_snapshot_blocks : 8192;  // (100 KB per block)
      if ((rc = snapshotUpdated(c, c->snap_stream, KHR_SNAP_ALL, snap_cap, &c->pending_snapshot))) return rc;
      HIP_TRY(hipEventRecord(c->ev_snap_join, c->snap_stream));
    }
    // (the list kernel on the main stream BEHIND the fork points: it runs beside the mesh kernels and the snapshot, not in front of them)
    if (early_list && (rc = removedPublishLaunch(c))) return rc;
    if (mc_fork) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_mc_join, 0));
    else if ((rc = generateMesh(c, c->stream, 1, 1))) return rc;
    if (snap) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_snap_join, 0));
    if (c->cfg.with_tracking) {
      if ((rc = resetInactiveLaunch(c, early_list, BLK_UPDATED))) return rc;  // (archival + the flag clearing of :169-171 in one pass)
    } else if ((rc = khr_clear_updated(c))) {
      return rc;
    }
    c->removed_early = early_list;
    HT("pf_output_launched");
  }
  // (6) ConnectedSemantics, host part (the records arrived long ago) + id remap queued behind everything else
  if (objects) {
    const int ns = objectsFinish(c, slot);
    if (ns < 0) return ns;
  }
  HT("pf_exit");
  leave.ok = true;
  return slot;
}

int khr_mark_all_inactive(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  hipLaunchKernelGGL(k_block_flag_op, dim3(gridFor(c->m.capacity)), dim3(256), 0, c->stream, c->m, ~BLK_HAS_ACTIVE, BLK_TRACK_DIRTY);
  HIP_TRY(hipGetLastError());
  c->host_index_valid = false, ++c->map_gen;
  return KHR_OK;
}

int khr_clear_updated(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  hipLaunchKernelGGL(k_block_flag_op, dim3(gridFor(c->m.capacity)), dim3(256), 0, c->stream, c->m, ~BLK_UPDATED, 0u);
  HIP_TRY(hipGetLastError());
  c->host_index_valid = false, ++c->map_gen;
  return KHR_OK;
}

int khr_allocate_blocks(khr_ctx* c, const int32_t* indices, int64_t n) {
  if (!c || (!indices && n > 0)) return fail(KHR_EINVAL, "null argument");
  if (n <= 0) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  // de-duplicate on the host: the device insert requires unique keys per launch
  std::vector<std::array<int32_t, 3>> v(n);
  for (int64_t i = 0; i < n; ++i) v[i] = {indices[3 * i], indices[3 * i + 1], indices[3 * i + 2]};
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  // asynchronous: the indices travel through a pinned buffer owned by the context (no hipMalloc /
  // hipFree, which stall every stream of the device); the buffer is reused only after the previous upload was consumed
  const size_t bytes = sizeof(int32_t) * 3 * v.size();
  HT("ab_enter");
  if (c->ev_up) HIP_TRY(hipEventSynchronize(c->ev_up));
  KHR_TRY(c->ev_up.ensure());
  HT("ab_prev_upload_consumed");
  if (bytes > c->h_up.count()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t want = std::max<size_t>(2 * bytes, 1u << 16);
    if (c->h_up.reserve(want)) return fail(KHR_ENOMEM, "block index staging of %zu bytes", want);
  }
  std::memcpy(c->h_up, v.data(), bytes);
  // the kernel reads the indices straight out of the page-locked staging block (a few tens of KB over the link): round 5 -- a
  // hipMemcpyAsync here, issued from an extraction worker's thread, did not return for 7 ms while the window's thread kept the
  // copy path busy with its frames' planes (KHR_PF_INPUT_PINNED; profiles/r05_host_input_marks.txt)
  HIP_TRY(hipMemsetAsync(&c->m.counters[C_N_NEW], 0, sizeof(uint32_t), c->stream));
  c->explicit_blocks += v.size();
  hipLaunchKernelGGL(k_alloc_list, dim3(gridFor(v.size())), dim3(256), 0, c->stream, c->m, static_cast<const int*>(c->h_up.dev()),
                     static_cast<int>(v.size()), c->d_new);
  HIP_TRY(hipEventRecord(c->ev_up, c->stream));  // (the staging block is free again once the kernel has read it)
  hipLaunchKernelGGL(k_init_blocks, dim3(2048), dim3(256), 0, c->stream, c->m, c->p, c->d_new);
  HIP_TRY(hipGetLastError());
  c->host_index_valid = false, ++c->map_gen;
  return KHR_OK;
}

int khr_begin_object_map(khr_ctx* c, float voxel_size, float truncation_distance, const int32_t lo[3], const int32_t hi[3]) {
  if (!c || !lo || !hi) return fail(KHR_EINVAL, "null argument");
  uint64_t n = 1;
  for (int d = 0; d < 3; ++d) {
    if (hi[d] < lo[d]) return fail(KHR_EINVAL, "empty block box");
    const uint64_t side = static_cast<uint64_t>(static_cast<int64_t>(hi[d]) - lo[d] + 1);
    if (side > 0xffffffffull / n) return fail(KHR_EINVAL, "block box too large");
    n *= side;
  }
  int rc = resetMap(c, voxel_size, truncation_distance);
  if (rc) return rc;
  if (n > c->m.capacity) {  // more blocks than the pool has: the step-wise allocation hands out what there is and counts the rest
    std::vector<int32_t> idx;
    for (int x = lo[0]; x <= hi[0]; ++x)
      for (int y = lo[1]; y <= hi[1]; ++y)
        for (int z = lo[2]; z <= hi[2]; ++z) idx.insert(idx.end(), {x, y, z});
    return khr_allocate_blocks(c, idx.data(), static_cast<int64_t>(n));
  }
  BoxSetupZero zero{};
  if (c->d_multi_list) {  // the counters of k_multi_order (8^3 maps)
    zero.w = reinterpret_cast<uint32_t*>(c->d_multi_list + 2 * static_cast<size_t>(c->item_cap));
    zero.n = 8;
  }
  hipLaunchKernelGGL(k_setup_box, dim3(static_cast<unsigned>(n)), dim3(256), 0, c->stream, c->m, c->p, make_int3(lo[0], lo[1], lo[2]),
                     make_int3(hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1), static_cast<uint32_t>(n), c->d_work,
                     FuseList{c->d_work4, c->d_work4 + c->item_cap, c->item_cap, &c->m.counters[C_N_ITEMS0]}, c->wpb, c->d_wg_stats, zero);
  HIP_TRY(hipGetLastError());
  c->explicit_blocks = n;
  c->host_index_valid = false, ++c->map_gen;
  c->box_gen = c->map_gen;
  c->box_listed = true;  // (the per-call reset and the block list of the next integration are done)
  c->multi_counts_zeroed = static_cast<bool>(c->d_multi_list);
  c->pruned_zeroed = true;  // (k_reset_map)
  return KHR_OK;
}

int khr_object_prune(khr_ctx* c, float min_confidence, float min_observations, int64_t* n_pruned) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->cfg.with_semantics || c->p.K < 2) return fail(KHR_ESTATE, "object pruning needs a binary semantic layer");
  if (!(c->pruned_zeroed && c->box_gen == c->map_gen)) HIP_TRY(hipMemsetAsync(&c->m.stats[S_PRUNED], 0, sizeof(unsigned long long), c->stream));
  c->pruned_zeroed = false;
  int rc = dispatchVps(c, [&](auto vps) {
    hipLaunchKernelGGL((k_object_prune<decltype(vps)::value>), dim3(kStreamGrid), dim3(256), 0, c->stream, c->m, c->p,
                       min_confidence, min_observations);
    return KHR_OK;
  });
  if (rc) return rc;
  return n_pruned ? readPruned(c, n_pruned) : KHR_OK;  // (asynchronous without a count request)
}

static int refreshMeshTotals(khr_ctx* c);

// sticky count of dropped records / failed allocations (khr_stats.pool_exhausted) without the rest of khr_get_stats (which
// rebuilds the host-side block index: ~1 ms for a 1 cm map)
int64_t khr_pool_exhausted(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  const int rc = readCounters(c);
  if (rc) return rc;
  return static_cast<int64_t>(c->h_counters[C_POOL_EXHAUSTED]);
}

int khr_get_stats(khr_ctx* c, khr_stats* out) {
  if (!c || !out) return fail(KHR_EINVAL, "null argument");
  int rc = readCounters(c);
  if (rc) return rc;
  unsigned long long st[S_COUNT];
  HIP_TRY(hipMemcpy(st, c->m.stats, sizeof(st), hipMemcpyDeviceToHost));
  // live-block count
  rc = ensureHostIndex(c);
  if (rc) return rc;
  rc = refreshMeshTotals(c);
  if (rc) return rc;
  khr_stats s = c->stats;
  s.n_allocated_blocks = c->host_index.size();
  s.n_visible_blocks = c->h_counters[C_N_VISIBLE];
  s.n_new_blocks = c->h_counters[C_N_NEW];
  s.n_visited_voxels = static_cast<uint64_t>(c->h_counters[C_N_VISIBLE]) * c->p.nvox;
  // k_fuse's per-workgroup partial sums since the last per-call reset (beginIntegrate folds them into the totals)
  std::vector<uint32_t> wgs(2 * kUpdateStatSlots);
  HIP_TRY(hipMemcpy(wgs.data(), c->d_wg_stats, sizeof(uint32_t) * wgs.size(), hipMemcpyDeviceToHost));
  uint64_t cur_upd = 0, cur_band = 0;
  for (int i = 0; i < kUpdateStatSlots; ++i) {
    cur_upd += wgs[2 * i];
    cur_band += wgs[2 * i + 1];
  }
  s.n_updated_voxels = cur_upd;
  s.n_band_voxels = cur_band;
  s.n_tracking_updated_blocks = c->h_counters[c->ef_cur ? C_N_EF2 : C_N_EF_A];
  s.pool_exhausted = c->h_counters[C_POOL_EXHAUSTED];
  s.n_tsdf_blocks = c->h_counters[C_N_TSDF];
  s.n_fuse_items = static_cast<uint64_t>(c->h_counters[C_N_ITEMS0]) + c->h_counters[C_N_ITEMS1] + c->h_counters[C_N_ITEMS2] +
                   c->h_counters[C_N_ITEMS3];
  s.n_seed_waits = c->n_seed_waits;
  s.n_seed_waits_late = c->n_seed_waits_late;
  s.seed_wait_max_us = c->seed_wait_max_us;
  for (int i = 0; i < 8; ++i) s.seed_wait_hist[i] = c->seed_wait_hist[i];
  s.seed_wait_late_us = c->seed_wait_late_us;
  s.seed_wait_late_frame = c->seed_wait_late_frame;
  s.seed_wait_late_state = c->seed_wait_late_state;
  s.n_md_device_merges = c->n_md_device_merges;
  s.n_md_host_walks = c->n_md_host_walks;
  s.n_md_prelaunched = c->n_md_prelaunched;
  s.n_md_prelaunch_repeats = c->n_md_prelaunch_repeats;
  s.band_overflow = 0;  // (no update kernel keeps a global record list)
  s.n_tracking_processed_blocks = c->h_counters[c->ef_cur ? C_N_PROC2 : C_N_PROC];
  s.cum_updated_voxels = st[S_CUM_UPD] + cur_upd;
  s.cum_band_voxels = st[S_CUM_BAND] + cur_band;
  s.cum_visited_voxels = st[S_CUM_VISITED] + s.n_visited_voxels;
  s.cum_integrate_calls = st[S_CUM_CALLS];
  *out = s;
  return KHR_OK;
}

int64_t khr_num_blocks(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  int rc = ensureHostIndex(c);
  if (rc) return rc;
  return static_cast<int64_t>(c->host_index.size());
}

int64_t khr_block_indices(khr_ctx* c, int32_t* out, int64_t cap, int only_updated) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  int rc = ensureHostIndex(c);
  if (rc) return rc;
  int64_t n = 0;
  for (auto& kv : c->host_index) {  // std::map => sorted (x, y, z)
    if (only_updated && !(c->host_flags[kv.second] & BLK_UPDATED)) continue;
    if (out && n < cap) {
      out[3 * n] = kv.first[0];
      out[3 * n + 1] = kv.first[1];
      out[3 * n + 2] = kv.first[2];
    }
    ++n;
  }
  return n;
}

int khr_download_block(khr_ctx* c, int32_t bx, int32_t by, int32_t bz, float* distance, float* weight,
                       uint8_t* color_rgba, uint64_t* last_observed, uint64_t* last_occupied, uint8_t* voxel_flags,
                       uint32_t* sem_label, float* likelihoods, uint8_t* block_flags) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  int rc = ensureHostIndex(c);
  if (rc) return rc;
  auto it = c->host_index.find({bx, by, bz});
  if (it == c->host_index.end()) return fail(KHR_ENOTFOUND, "block (%d,%d,%d) not allocated", bx, by, bz);
  const size_t slot = it->second, nv = c->p.nvox;
  const DevMap& m = c->m;
  auto D = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream); };
  if (distance) HIP_TRY(D(distance, m.dist + slot * nv, nv * 4));
  if (weight) HIP_TRY(D(weight, m.weight + slot * nv, nv * 4));
  if (color_rgba) HIP_TRY(D(color_rgba, m.color + slot * nv, nv * 4));
  std::vector<uint8_t> raw_flags;
  if (voxel_flags || (last_occupied && c->cfg.with_tracking)) {
    raw_flags.resize(nv);
    HIP_TRY(D(raw_flags.data(), m.vflags + slot * nv, nv));
  }
  std::vector<uint64_t> obs_words;  // lazily stored last_observed (DevMap::obs): {bits, stamp} per 64 voxels
  if (last_observed) {
    if (c->cfg.with_tracking) {
      HIP_TRY(D(last_observed, m.last_obs + slot * nv, nv * 8));
      obs_words.resize(2 * (nv / 64));
      HIP_TRY(D(obs_words.data(), m.obs + slot * (nv / 64), (nv / 64) * 16));
    } else std::memset(last_observed, 0, nv * 8);
  }
  if (last_occupied) {
    if (c->cfg.with_tracking) HIP_TRY(D(last_occupied, m.last_occ + slot * nv, nv * 8));
    else std::memset(last_occupied, 0, nv * 8);
  }
  if (sem_label) {
    if (c->cfg.with_semantics) HIP_TRY(D(sem_label, m.sem_label + slot * nv, nv * 4));
    else std::memset(sem_label, 0, nv * 4);
  }
  std::vector<float> lik_vm;  // device layout is voxel-major [voxel][K]; the API hands out [k][voxel]
  if (likelihoods && c->cfg.with_semantics) {
    lik_vm.resize(nv * c->p.KS);
    HIP_TRY(D(lik_vm.data(), m.lik + slot * nv * c->p.KS, nv * c->p.KS * 4));
  }
  uint32_t bf = 0;
  if (block_flags) HIP_TRY(D(&bf, m.blk_flags + slot, 4));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (block_flags) *block_flags = static_cast<uint8_t>(bf & 0xfu);
  for (size_t w = 0; w < obs_words.size() / 2; ++w)
    for (int b = 0; b < 64; ++b)
      if ((obs_words[2 * w] >> b) & 1ull) last_observed[64 * w + b] = obs_words[2 * w + 1];
  // lazily stored last_occupied (k_tracking_update): an occupied voxel's stamp is the latest pass's stamp
  if (last_occupied && c->cfg.with_tracking)
    for (size_t i = 0; i < nv; ++i)
      if (raw_flags[i] & VOX_OCC) last_occupied[i] = c->last_track_stamp;
  if (voxel_flags)
    for (size_t i = 0; i < nv; ++i) voxel_flags[i] = raw_flags[i] & VOX_PUBLIC_MASK;
  if (likelihoods && c->cfg.with_semantics)
    for (size_t i = 0; i < nv; ++i)
      for (int k = 0; k < c->p.K; ++k) likelihoods[static_cast<size_t>(k) * nv + i] = lik_vm[i * c->p.KS + k];
  // voxels whose semantic entry is still empty carry undefined likelihood storage: report zeros
  if (likelihoods && c->cfg.with_semantics) {
    std::vector<uint8_t> fl(nv);
    const uint8_t* f = voxel_flags;
    if (!f) {
      HIP_TRY(hipMemcpy(fl.data(), m.vflags + slot * nv, nv, hipMemcpyDeviceToHost));
      f = fl.data();
    }
    for (size_t i = 0; i < nv; ++i)
      if (!(f[i] & VOX_SEM_VALID))
        for (int k = 0; k < c->p.K; ++k) likelihoods[static_cast<size_t>(k) * nv + i] = 0.f;
  }
  return KHR_OK;
}

// ---- one z-plane of the live map (khr_map_slice; ActiveWindowVisualizer's map slices, active_window_visualizer.cpp:345-520) ----
// getVoxelKey((0, 0, height)).z as a global voxel index: ASSUMPTIONS.md A.10 (hydra::sliceVoxelZ and capi.slice_voxel_z are
// the same rule)
int khr_slice_voxel_z(float height, float voxel_size, int32_t voxels_per_side, int64_t* voxel_z) {
  if (!voxel_z || !(voxel_size > 0.f) || voxels_per_side < 1 || !std::isfinite(height)) return fail(KHR_EINVAL, "bad argument");
  const float bs = voxel_size * static_cast<float>(voxels_per_side), bs_inv = 1.f / bs, vs_inv = 1.f / voxel_size;
  const float fb = std::floor(height * bs_inv);
  if (!(std::fabs(fb) < 1e15f)) return fail(KHR_EINVAL, "slice height %g is out of range", static_cast<double>(height));
  const int64_t bz = static_cast<int64_t>(fb);
  const float origin = static_cast<float>(bz) * bs;
  const int64_t v = static_cast<int64_t>(std::floor((height - origin) * vs_inv));
  *voxel_z = bz * voxels_per_side + v;
  return KHR_OK;
}

// byte offsets of the fields inside the slice staging of `cap` blocks (device staging and page-locked mirror alike)
struct SliceLayout {
  size_t xy, pos, dist, weight, obs, flags, bytes;
  SliceLayout(size_t cap, size_t np) {
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    xy = 256;  // (the mirror's first word takes the count)
    pos = xy + al(cap * 8);
    dist = pos + al(cap * np * 12);
    weight = dist + al(cap * np * 4);
    obs = weight + al(cap * np * 4);
    flags = obs + al(cap * np * 8);
    bytes = flags + al(cap * np);
  }
};

// the sort keys of khr_map_slice and khr_checkpoint_save (one u64 per pool slot, padded to a power of two) + their count word
static int ensureSortKeys(khr_ctx* c) {
  if (c->d_slice_keys) return KHR_OK;
  const uint32_t sort_len = slicePadded(c->m.capacity);
  if (c->d_slice_keys.alloc(sort_len) || c->d_slice_count.alloc(1)) {
    c->d_slice_keys.reset();
    return fail(KHR_ENOMEM, "sort keys (%u words)", sort_len);
  }
  return KHR_OK;
}
// ascending bitonic sort of d_slice_keys[0, *d_slice_count) on the context's stream (khr_kernels_slice.h)
static int sortKeys(khr_ctx* c) {
  const uint32_t sort_len = slicePadded(c->m.capacity);
  hipLaunchKernelGGL(k_slice_sort_tile, dim3(std::max(1u, sort_len / kSliceSortTile)), dim3(kSliceSortThreads), 0, c->stream,
                     c->d_slice_keys, c->d_slice_count, 0u);
  HIP_TRY(hipGetLastError());
  for (uint32_t k = 2 * kSliceSortTile; k <= sort_len; k <<= 1) {  // multi-pass: stages beyond the count's length exit on the device
    for (uint32_t j = k / 2; j >= kSliceSortTile; j >>= 1) {
      hipLaunchKernelGGL(k_slice_sort_step, dim3(std::min(gridFor(sort_len / 2), 1024)), dim3(256), 0, c->stream, c->d_slice_keys,
                         c->d_slice_count, k, j);
      HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_slice_sort_tile, dim3(sort_len / kSliceSortTile), dim3(kSliceSortThreads), 0, c->stream, c->d_slice_keys,
                       c->d_slice_count, k);
    HIP_TRY(hipGetLastError());
  }
  return KHR_OK;
}

static int sliceGrow(khr_ctx* c, uint32_t need) {
  const uint32_t cap = std::min<uint32_t>(std::max<uint32_t>(need + need / 2, 64u), c->m.capacity);
  const SliceLayout L(cap, static_cast<size_t>(c->p.vps) * c->p.vps);
  c->slice_cap = 0;
  KHR_TRY(reserveStagePair(c->d_slice_stage, c->h_slice_stage, L.bytes, "slice"));
  c->slice_cap = cap;
  return KHR_OK;
}

int khr_map_slice(khr_ctx* c, int64_t voxel_z, int64_t cap, int32_t* block_xy, float* positions, float* distance, float* weight,
                  uint64_t* last_observed, uint8_t* voxel_flags, int64_t* n_voxels) {
  if (!c || !n_voxels || cap < 0) return fail(KHR_EINVAL, "bad argument");
  *n_voxels = 0;
  HIP_TRY(hipSetDevice(c->device));
  if (c->m.capacity >= (1u << kSliceSlotBits)) return fail(KHR_EINVAL, "map slices need max_blocks < %u", 1u << kSliceSlotBits);
  const int64_t vps = c->p.vps, np = vps * vps;
  const int64_t bz = (voxel_z >= 0 ? voxel_z : voxel_z - (vps - 1)) / vps, lz = voxel_z - bz * vps;  // floor division
  if (bz < -(1 << 20) || bz >= (1 << 20)) return KHR_OK;  // (beyond the block index range: no block lies there)
  {
    const int rc = ensureSortKeys(c);
    if (rc) return rc;
  }
  if (!c->d_slice_stage) {
    const int rc = sliceGrow(c, 64u);
    if (rc) return rc;
  }
  const bool want[6] = {block_xy != nullptr, positions != nullptr, distance != nullptr, weight != nullptr, last_observed != nullptr,
                        voxel_flags != nullptr};
  auto outFor = [&]() {
    const SliceLayout L(c->slice_cap, static_cast<size_t>(np));
    uint8_t* d = c->d_slice_stage;
    SliceOut o{};
    o.block_xy = want[0] ? reinterpret_cast<int32_t*>(d + L.xy) : nullptr;
    o.pos = want[1] ? reinterpret_cast<float*>(d + L.pos) : nullptr;
    o.dist = want[2] ? reinterpret_cast<float*>(d + L.dist) : nullptr;
    o.weight = want[3] ? reinterpret_cast<float*>(d + L.weight) : nullptr;
    o.last_obs = want[4] ? reinterpret_cast<uint64_t*>(d + L.obs) : nullptr;
    o.vflags = want[5] ? d + L.flags : nullptr;
    o.cap_blocks = c->slice_cap;
    return o;
  };
  const int gather_grid = static_cast<int>(std::min<uint32_t>(c->m.capacity, 2048u));
  auto gather = [&]() {
    return dispatchVps(c, [&](auto vps_c) {
      constexpr int V = decltype(vps_c)::value;
      hipLaunchKernelGGL((k_slice_gather<V>), dim3(gather_grid), dim3(V * V), 0, c->stream, c->m, c->p, c->d_slice_keys,
                         c->d_slice_count, static_cast<int>(bz), static_cast<int>(lz), outFor());
      HIP_TRY(hipGetLastError());
      return KHR_OK;
    });
  };
  // per-block bytes of each field and its offset: copies of the blocks [b0, b1) into the mirror
  auto copies = [&](uint32_t b0, uint32_t b1) {
    const SliceLayout L(c->slice_cap, static_cast<size_t>(np));
    const size_t off[6] = {L.xy, L.pos, L.dist, L.weight, L.obs, L.flags};
    const size_t per[6] = {8, static_cast<size_t>(np) * 12, static_cast<size_t>(np) * 4, static_cast<size_t>(np) * 4,
                           static_cast<size_t>(np) * 8, static_cast<size_t>(np)};
    for (int f = 0; f < 6; ++f)
      if (want[f] && b1 > b0)
        HIP_TRY(hipMemcpyAsync(c->h_slice_stage + off[f] + b0 * per[f], c->d_slice_stage + off[f] + b0 * per[f], (b1 - b0) * per[f],
                               hipMemcpyDeviceToHost, c->stream));
    return KHR_OK;
  };
  // select -> sort -> gather, all on the device; then the count and the hinted number of blocks of every requested field in one batch
  HIP_TRY(hipMemsetAsync(c->d_slice_count, 0, sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_slice_select, dim3(std::min(gridFor(c->m.capacity), 1024)), dim3(256), 0, c->stream, c->m, static_cast<int>(bz),
                     c->d_slice_count, c->d_slice_keys);
  HIP_TRY(hipGetLastError());
  int rc = sortKeys(c);
  if (rc) return rc;
  rc = gather();
  if (rc) return rc;
  uint32_t n_copied = std::min(c->slice_cap, c->slice_hint);
  HIP_TRY(hipMemcpyAsync(c->h_slice_stage, c->d_slice_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if ((rc = copies(0, n_copied))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  const uint32_t n = *reinterpret_cast<const uint32_t*>(c->h_slice_stage.get());
  if (n > c->slice_cap) {  // (the staging was too small and the gather wrote nothing: grow, gather again)
    if ((rc = sliceGrow(c, n))) return rc;
    if ((rc = gather())) return rc;
    n_copied = 0;
  }
  if (n > n_copied) {  // (more blocks than the hint: the rest)
    if ((rc = copies(n_copied, n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  c->slice_hint = n + n / 4 + 16;
  *n_voxels = static_cast<int64_t>(n) * np;
  if (*n_voxels > cap)
    return fail(KHR_ENOMEM, "the slice holds %lld voxels, cap %lld", static_cast<long long>(*n_voxels), static_cast<long long>(cap));
  const SliceLayout L(c->slice_cap, static_cast<size_t>(np));
  const uint8_t* h = c->h_slice_stage;
  const size_t nv = static_cast<size_t>(*n_voxels);
  if (block_xy) std::memcpy(block_xy, h + L.xy, static_cast<size_t>(n) * 8);
  if (positions) std::memcpy(positions, h + L.pos, nv * 12);
  if (distance) std::memcpy(distance, h + L.dist, nv * 4);
  if (weight) std::memcpy(weight, h + L.weight, nv * 4);
  if (last_observed) std::memcpy(last_observed, h + L.obs, nv * 8);
  if (voxel_flags) std::memcpy(voxel_flags, h + L.flags, nv);
  return KHR_OK;
}

// ---- the live map seen from a pose (khr_render_view; ASSUMPTIONS.md A.12, device side: khr_kernels_render.h) -------------------
int khr_render_view(khr_ctx* c, const khr_render_request* rq, int on_device, float* depth, float* normal, uint8_t* color_rgba,
                    uint32_t* label, uint8_t* vflags, uint8_t* status, khr_render_stats* stats) {
  if (!c || !rq) return fail(KHR_EINVAL, "null argument");
  const khr_sensor& sn = rq->sensor;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(rq->world_T_sensor[i])) return fail(KHR_EINVAL, "world_T_sensor is not finite");
  if (sn.width <= 0 || sn.height <= 0 || static_cast<int64_t>(sn.width) * sn.height > (int64_t(1) << 30))
    return fail(KHR_EINVAL, "bad image size %d x %d", sn.width, sn.height);
  if (!std::isfinite(sn.fx) || !std::isfinite(sn.fy) || sn.fx == 0.f || sn.fy == 0.f || !std::isfinite(sn.cx) || !std::isfinite(sn.cy))
    return fail(KHR_EINVAL, "bad intrinsics");
  if (!std::isfinite(sn.min_range) || !std::isfinite(sn.max_range) || sn.min_range < 0.f || sn.max_range < sn.min_range)
    return fail(KHR_EINVAL, "bad range limits [%g, %g]", static_cast<double>(sn.min_range), static_cast<double>(sn.max_range));
  if (!(rq->step_voxels >= 0.f) || !std::isfinite(rq->step_voxels)) return fail(KHR_EINVAL, "bad step_voxels %g", static_cast<double>(rq->step_voxels));
  if (!(rq->min_weight >= 0.f)) return fail(KHR_EINVAL, "bad min_weight %g", static_cast<double>(rq->min_weight));
  const float dt = (rq->step_voxels == 0.f ? 0.5f : rq->step_voxels) * c->p.vs;
  const float n_steps = std::floor((sn.max_range - sn.min_range) / dt);
  if (!(n_steps < 65536.f)) return fail(KHR_EINVAL, "more than 65536 samples per ray (step %g m over %g m)", static_cast<double>(dt),
                                        static_cast<double>(sn.max_range - sn.min_range));
  if (c->cfg.world_size > 1) return fail(KHR_ESTATE, "khr_render_view needs the whole map: world_size is %d", c->cfg.world_size);
  HIP_TRY(hipSetDevice(c->device));
  RenderView r{};
  r.W = sn.width;
  r.H = sn.height;
  r.K = static_cast<int>(n_steps) + 1;
  r.fx = sn.fx;
  r.fy = sn.fy;
  r.cx = sn.cx;
  r.cy = sn.cy;
  r.min_range = sn.min_range;
  r.dt = dt;
  r.min_weight = rq->min_weight == 0.f ? c->cfg.mesh_min_weight : rq->min_weight;
  {
    float R[9], t[3];
    makePose(rq->world_T_sensor, R, t, r.Rw, r.tw);
  }
  const size_t n_px = static_cast<size_t>(sn.width) * sn.height;
  // the images of the host form, one after the other in the device staging and its page-locked mirror
  void* const host[6] = {depth, normal, color_rgba, label, vflags, status};
  const size_t per_px[6] = {4, 12, 4, 4, 1, 1};
  size_t off[6], stage_bytes = 0;
  for (int f = 0; f < 6; ++f) {
    off[f] = stage_bytes;
    if (host[f]) stage_bytes += (n_px * per_px[f] + 255) / 256 * 256;
  }
  void* dev[6] = {depth, normal, color_rgba, label, vflags, status};
  if (!on_device && stage_bytes) {
    KHR_TRY(reserveStagePair(c->d_render_stage, c->h_render_stage, stage_bytes, "render"));
    for (int f = 0; f < 6; ++f) dev[f] = host[f] ? c->d_render_stage + off[f] : nullptr;
  }
  r.depth = static_cast<float*>(dev[0]);
  r.normal = static_cast<float*>(dev[1]);
  r.color = static_cast<uint32_t*>(dev[2]);
  r.label = static_cast<uint32_t*>(dev[3]);
  r.vflags = static_cast<uint8_t*>(dev[4]);
  r.status = static_cast<uint8_t*>(dev[5]);
  if (stats) {
    if (!c->d_render_stats && c->d_render_stats.alloc(RS_COUNT)) return fail(KHR_ENOMEM, "render counters");
    HIP_TRY(hipMemsetAsync(c->d_render_stats, 0, sizeof(unsigned long long) * RS_COUNT, c->stream));
    r.stats = c->d_render_stats;
  }
  const dim3 grid(static_cast<unsigned>((sn.width + 15) / 16), static_cast<unsigned>((sn.height + 15) / 16));
  int rc = dispatchVps(c, [&](auto vps) {
    hipLaunchKernelGGL((k_render_view<decltype(vps)::value>), grid, dim3(256), 0, c->stream, c->m, c->p, r);
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
  if (rc) return rc;
  unsigned long long h_stats[RS_COUNT] = {0, 0, 0, 0};
  if (stats) HIP_TRY(hipMemcpyAsync(h_stats, c->d_render_stats, sizeof(h_stats), hipMemcpyDeviceToHost, c->stream));
  if (!on_device && stage_bytes)
    HIP_TRY(hipMemcpyAsync(c->h_render_stage, c->d_render_stage, stage_bytes, hipMemcpyDeviceToHost, c->stream));
  if (stats || (!on_device && stage_bytes)) HIP_TRY(hipStreamSynchronize(c->stream));
  if (!on_device)
    for (int f = 0; f < 6; ++f)
      if (host[f]) std::memcpy(host[f], c->h_render_stage + off[f], n_px * per_px[f]);
  if (stats) {
    stats->n_hit = h_stats[RS_HIT];
    stats->n_blocked = h_stats[RS_BLOCKED];
    stats->n_samples_total = static_cast<uint64_t>(r.K) * n_px;
    stats->n_samples_evaluated = h_stats[RS_VISITED];
  }
  return KHR_OK;
}

// ---- the live map at world points (khr_query_points; ASSUMPTIONS.md A.13, device side: khr_kernels_query.h) --------------------
int khr_query_points(khr_ctx* c, int64_t n, const float* points, float min_weight, int on_device, float* distance, float* gradient,
                     float* weight, uint8_t* color_rgba, uint32_t* label, uint8_t* vflags, uint64_t* last_observed, uint8_t* status,
                     khr_query_stats* stats) {
  if (!c) return fail(KHR_EINVAL, "null argument");
  if (n < 0) return fail(KHR_EINVAL, "negative point count %lld", static_cast<long long>(n));
  if (n > 0 && !points) return fail(KHR_EINVAL, "null points");
  if (!(min_weight >= 0.f) || !std::isfinite(min_weight)) return fail(KHR_EINVAL, "bad min_weight %g", static_cast<double>(min_weight));
  if (c->cfg.world_size > 1) return fail(KHR_ESTATE, "khr_query_points needs the whole map: world_size is %d", c->cfg.world_size);
  if (n == 0) {
    if (stats) *stats = khr_query_stats{0, 0, 0};
    return KHR_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t np = static_cast<size_t>(n);
  // the host form: the points, then the outputs, one after the other in the device staging and its page-locked mirror
  void* const host[8] = {distance, gradient, weight, color_rgba, label, vflags, last_observed, status};
  const size_t per_pt[8] = {4, 12, 4, 4, 4, 1, 8, 1};
  size_t off[8], stage_bytes = (np * 12 + 255) / 256 * 256;
  const size_t out_begin = stage_bytes;
  for (int f = 0; f < 8; ++f) {
    off[f] = stage_bytes;
    if (host[f]) stage_bytes += (np * per_pt[f] + 255) / 256 * 256;
  }
  void* dev[8] = {distance, gradient, weight, color_rgba, label, vflags, last_observed, status};
  const float* d_points = points;
  if (!on_device) {
    KHR_TRY(reserveStagePair(c->d_query_stage, c->h_query_stage, stage_bytes, "query"));
    std::memcpy(c->h_query_stage, points, np * 12);
    HIP_TRY(hipMemcpyAsync(c->d_query_stage, c->h_query_stage, np * 12, hipMemcpyHostToDevice, c->stream));
    d_points = reinterpret_cast<const float*>(c->d_query_stage.get());
    for (int f = 0; f < 8; ++f) dev[f] = host[f] ? c->d_query_stage + off[f] : nullptr;
  }
  if (stats) {
    if (!c->d_query_stats && c->d_query_stats.alloc(QS_COUNT)) return fail(KHR_ENOMEM, "query counters");
    HIP_TRY(hipMemsetAsync(c->d_query_stats, 0, sizeof(unsigned long long) * QS_COUNT, c->stream));
  }
  constexpr size_t kChunk = size_t(1) << 30;  // points per launch (the grid's x extent)
  for (size_t first = 0; first < np; first += kChunk) {
    QueryPoints q{};
    q.n = static_cast<long long>(np - first < kChunk ? np - first : kChunk);
    q.points = d_points + 3 * first;
    q.min_weight = min_weight == 0.f ? c->cfg.mesh_min_weight : min_weight;
    q.distance = dev[0] ? static_cast<float*>(dev[0]) + first : nullptr;
    q.gradient = dev[1] ? static_cast<float*>(dev[1]) + 3 * first : nullptr;
    q.weight = dev[2] ? static_cast<float*>(dev[2]) + first : nullptr;
    q.color = dev[3] ? static_cast<uint32_t*>(dev[3]) + first : nullptr;
    q.label = dev[4] ? static_cast<uint32_t*>(dev[4]) + first : nullptr;
    q.vflags = dev[5] ? static_cast<uint8_t*>(dev[5]) + first : nullptr;
    q.last_observed = dev[6] ? static_cast<uint64_t*>(dev[6]) + first : nullptr;
    q.status = dev[7] ? static_cast<uint8_t*>(dev[7]) + first : nullptr;
    q.stats = stats ? c->d_query_stats : nullptr;
    const dim3 grid(static_cast<unsigned>((q.n + 255) / 256));
    int rc = dispatchVps(c, [&](auto vps) {
      hipLaunchKernelGGL((k_query_points<decltype(vps)::value>), grid, dim3(256), 0, c->stream, c->m, c->p, q);
      HIP_TRY(hipGetLastError());
      return KHR_OK;
    });
    if (rc) return rc;
  }
  unsigned long long h_stats[QS_COUNT] = {0, 0, 0, 0};
  if (stats) HIP_TRY(hipMemcpyAsync(h_stats, c->d_query_stats, sizeof(h_stats), hipMemcpyDeviceToHost, c->stream));
  const bool copy_back = !on_device && stage_bytes > out_begin;
  if (copy_back)
    HIP_TRY(hipMemcpyAsync(c->h_query_stage + out_begin, c->d_query_stage + out_begin, stage_bytes - out_begin, hipMemcpyDeviceToHost, c->stream));
  if (stats || !on_device) HIP_TRY(hipStreamSynchronize(c->stream));  // (host form: the point staging is free again on return)
  if (copy_back)
    for (int f = 0; f < 8; ++f)
      if (host[f]) std::memcpy(host[f], c->h_query_stage + off[f], np * per_pt[f]);
  if (stats) {
    stats->n_value = h_stats[QS_VALUE];
    stats->n_gradient = h_stats[QS_GRADIENT];
    stats->n_voxel = h_stats[QS_VOXEL];
  }
  return KHR_OK;
}

// ---- the exact Euclidean distance field of a box of the live map (khr_distance_field; ASSUMPTIONS.md A.15, device side:
// khr_kernels_distance.h) -----------------------------------------------------------------------------------------------------
namespace {

// what khr_distance_field and khr_voronoi_field share: the checks of A.15's box and cell classes (KHR_EINVAL; `cells` and the
// range R in cells on success), and the launch of k_df_gather over the blocks the box overlaps (g.box is filled here)
int dfCheckBox(khr_ctx* c, const char* who, const int32_t origin[3], const int32_t dims[3], int ratio, float min_weight, float max_distance,
               float surface_distance, size_t* n_cells, int* range) {
  const int vps = c->cfg.voxels_per_side;
  if (ratio != 1 && ratio != 2 && ratio != 4) return fail(KHR_EINVAL, "ratio %d: 1, 2 or 4", ratio);
  if (vps % ratio != 0) return fail(KHR_EINVAL, "ratio %d does not divide voxels_per_side %d", ratio, vps);
  KHR_TRY(checkBox(who, origin, dims, ratio, n_cells));
  if (!std::isfinite(surface_distance)) return fail(KHR_EINVAL, "surface_distance is not finite");
  if (!(min_weight >= 0.f) || !std::isfinite(min_weight)) return fail(KHR_EINVAL, "bad min_weight %g", static_cast<double>(min_weight));
  if (!(max_distance > 0.f) || !std::isfinite(max_distance)) return fail(KHR_EINVAL, "bad max_distance %g", static_cast<double>(max_distance));
  const float reach = max_distance / (c->p.vs * static_cast<float>(ratio));
  if (!(reach < 32768.f)) return fail(KHR_EINVAL, "max_distance %g m is %g cells: fewer than 32768", static_cast<double>(max_distance), static_cast<double>(reach));
  *range = static_cast<int>(std::floor(reach));
  return KHR_OK;
}

int dfLaunchGather(khr_ctx* c, const int32_t origin[3], const int32_t dims[3], int ratio, DfGather& g) {
  auto floorDiv = [](int64_t a, int64_t b) { return static_cast<int>(a >= 0 ? a / b : -((-a + b - 1) / b)); };
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  g.box.ox = origin[0], g.box.oy = origin[1], g.box.oz = origin[2];
  g.box.nx = nx, g.box.ny = ny, g.box.nz = nz;
  const int cps = c->cfg.voxels_per_side / ratio;  // cells per block side
  g.box.bx0 = floorDiv(origin[0], cps), g.box.by0 = floorDiv(origin[1], cps), g.box.bz0 = floorDiv(origin[2], cps);
  const dim3 blocks(static_cast<unsigned>(floorDiv(static_cast<int64_t>(origin[0]) + nx - 1, cps) - g.box.bx0 + 1),
                    static_cast<unsigned>(floorDiv(static_cast<int64_t>(origin[1]) + ny - 1, cps) - g.box.by0 + 1),
                    static_cast<unsigned>(floorDiv(static_cast<int64_t>(origin[2]) + nz - 1, cps) - g.box.bz0 + 1));
  return dispatchVps(c, [&](auto vps_c) {
    constexpr int VPS = decltype(vps_c)::value;
    if (ratio == 1) hipLaunchKernelGGL((k_df_gather<VPS, 1>), blocks, dim3(256), 0, c->stream, c->m, g);
    else if (ratio == 2) hipLaunchKernelGGL((k_df_gather<VPS, 2>), blocks, dim3(256), 0, c->stream, c->m, g);
    else hipLaunchKernelGGL((k_df_gather<VPS, 4>), blocks, dim3(256), 0, c->stream, c->m, g);
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
}

}  // namespace

int khr_distance_field(khr_ctx* c, const khr_df_request* rq, int on_device, float* distance, int32_t* d2, uint8_t* status, khr_df_stats* stats) {
  if (!c || !rq) return fail(KHR_EINVAL, "null argument");
  const int ratio = rq->ratio;
  size_t n = 0;
  int R = 0;
  KHR_TRY(dfCheckBox(c, "khr_distance_field", rq->origin, rq->dims, ratio, rq->min_weight, rq->max_distance, rq->surface_distance, &n, &R));
  const float cell_size = c->p.vs * static_cast<float>(ratio);
  if (c->cfg.world_size > 1) return fail(KHR_ESTATE, "khr_distance_field needs the whole map: world_size is %d", c->cfg.world_size);
  HIP_TRY(hipSetDevice(c->device));
  const bool with_inner = rq->positive_only == 0;
  // the work grids grow on demand; what may still read the old ones is waited for first
  if (c->d_df_outer.count() < n || (with_inner && c->d_df_inner.count() < n)) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_df_outer.reserve(n) || (with_inner && c->d_df_inner.reserve(n))) return fail(KHR_ENOMEM, "distance field work grids of %zu cells", n);
  }
  // the host form: the outputs one after the other in the device staging and its page-locked mirror
  void* const host[3] = {distance, d2, status};
  const size_t per_cell[3] = {4, 4, 1};
  Arena stage;
  size_t off[3];
  for (int f = 0; f < 3; ++f) off[f] = host[f] ? stage.take(n * per_cell[f]) : 0;
  const size_t stage_bytes = stage.bytes();
  void* dev[3] = {distance, d2, status};
  if (!on_device && stage_bytes) {
    if (stage_bytes > c->d_df_stage.count() || stage_bytes > c->h_df_stage.count()) HIP_TRY(hipStreamSynchronize(c->stream));
    KHR_TRY(reserveStagePair(c->d_df_stage, c->h_df_stage, stage_bytes, "distance field"));
    for (int f = 0; f < 3; ++f) dev[f] = host[f] ? c->d_df_stage + off[f] : nullptr;
  }
  if (stats) {
    if (!c->d_df_stats && c->d_df_stats.alloc(DFS_COUNT)) return fail(KHR_ENOMEM, "distance field counters");
    HIP_TRY(hipMemsetAsync(c->d_df_stats, 0, sizeof(unsigned long long) * DFS_COUNT, c->stream));
  }
  const int nx = rq->dims[0], ny = rq->dims[1], nz = rq->dims[2];
  DfGather g{};
  g.min_weight = rq->min_weight == 0.f ? c->cfg.mesh_min_weight : rq->min_weight;
  g.surface_distance = rq->surface_distance;
  g.unknown_is_obstacle = rq->unknown_is_obstacle;
  g.outer = c->d_df_outer;
  g.inner = with_inner ? c->d_df_inner.get() : nullptr;
  g.status = static_cast<uint8_t*>(dev[2]);
  g.stats = stats ? c->d_df_stats.get() : nullptr;
  KHR_TRY(dfLaunchGather(c, rq->origin, rq->dims, ratio, g));
  // three in-place passes per grid; a pass along an axis of one cell (or with R = 0) changes nothing and is left out
  for (int32_t* grid : {g.outer, g.inner}) {
    if (!grid || R < 1) continue;
    auto pass = [&](auto axis) {
      constexpr int A = decltype(axis)::value;
      const PassGrid p = axisPassGrid(A, nx, ny, nz, kDfTileCells, kDfStrip);
      hipLaunchKernelGGL((k_df_pass<A>), dim3(p.gx, p.gy), dim3(256), 0, c->stream, grid, nx, ny, nz, R, p.per_wg);
    };
    if (nx > 1) pass(std::integral_constant<int, 0>());
    if (ny > 1) pass(std::integral_constant<int, 1>());
    if (nz > 1) pass(std::integral_constant<int, 2>());
    HIP_TRY(hipGetLastError());
  }
  DfFinish f{};
  f.n = static_cast<long long>(n);
  f.outer = g.outer, f.inner = g.inner;
  f.r2 = R * R;
  f.cell_size = cell_size, f.max_distance = rq->max_distance;
  f.distance = static_cast<float*>(dev[0]), f.d2 = static_cast<int32_t*>(dev[1]), f.status = static_cast<uint8_t*>(dev[2]);
  f.stats = g.stats;
  if (f.distance || f.d2 || f.status || f.stats) {
    hipLaunchKernelGGL(k_df_finish, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, c->stream, f);
    HIP_TRY(hipGetLastError());
  }
  unsigned long long h_stats[DFS_COUNT] = {0, 0, 0, 0};
  if (stats) HIP_TRY(hipMemcpyAsync(h_stats, c->d_df_stats, sizeof(h_stats), hipMemcpyDeviceToHost, c->stream));
  const bool copy_back = !on_device && stage_bytes > 0;
  if (copy_back) HIP_TRY(hipMemcpyAsync(c->h_df_stage, c->d_df_stage, stage_bytes, hipMemcpyDeviceToHost, c->stream));
  if (stats || copy_back) HIP_TRY(hipStreamSynchronize(c->stream));
  if (copy_back)
    for (int k = 0; k < 3; ++k)
      if (host[k]) std::memcpy(host[k], c->h_df_stage + off[k], n * per_cell[k]);
  if (stats) {
    stats->n_observed = h_stats[DFS_OBSERVED];
    stats->n_obstacle = h_stats[DFS_OBSTACLE];
    stats->n_free = h_stats[DFS_OBSERVED] - h_stats[DFS_OBSTACLE];
    stats->n_in_range = h_stats[DFS_IN_RANGE];
  }
  return KHR_OK;
}

// ---- nearest obstacle cell and generalized Voronoi cells of a box of the live map (khr_voronoi_field; ASSUMPTIONS.md A.20,
// device side: khr_kernels_voronoi.h; the layouts of its buffers: vorDense and vorList of khr_box_host.h) -----------------------

int khr_voronoi_field(khr_ctx* c, const khr_voronoi_request* rq, khr_voronoi_stats* stats) {
  if (stats) *stats = khr_voronoi_stats{};
  if (!c || !rq) return fail(KHR_EINVAL, "khr_voronoi_field: null argument");
  // KHR_EINVAL / KHR_ESTATE: nothing is done, an earlier result stays
  const int ratio = rq->ratio;
  size_t n = 0;
  int R = 0;
  KHR_TRY(dfCheckBox(c, "khr_voronoi_field", rq->origin, rq->dims, ratio, rq->min_weight, rq->max_distance, rq->surface_distance, &n, &R));
  if (!(rq->min_distance >= 0.f) || !std::isfinite(rq->min_distance)) return fail(KHR_EINVAL, "khr_voronoi_field: bad min_distance %g", static_cast<double>(rq->min_distance));
  if (rq->mode != KHR_VOR_L1 && rq->mode != KHR_VOR_ANGLE && rq->mode != KHR_VOR_L1_THEN_ANGLE)
    return fail(KHR_EINVAL, "khr_voronoi_field: mode %d: KHR_VOR_L1, KHR_VOR_ANGLE or KHR_VOR_L1_THEN_ANGLE", rq->mode);
  if (rq->mode != KHR_VOR_ANGLE && rq->parent_l1_separation < 1)
    return fail(KHR_EINVAL, "khr_voronoi_field: parent_l1_separation is %d, must be >= 1", rq->parent_l1_separation);
  if (rq->mode != KHR_VOR_L1 && !(rq->parent_cos_angle_separation >= -1.f && rq->parent_cos_angle_separation <= 1.f))
    return fail(KHR_EINVAL, "khr_voronoi_field: parent_cos_angle_separation is %g, must lie in [-1, 1]", static_cast<double>(rq->parent_cos_angle_separation));
  if (rq->min_basis != 0 && (rq->min_basis < 2 || rq->min_basis > KHR_VOR_MAX_BASIS))
    return fail(KHR_EINVAL, "khr_voronoi_field: min_basis is %d: 0, 2, 3 or 4", rq->min_basis);
  if (c->cfg.world_size > 1) return fail(KHR_ESTATE, "khr_voronoi_field needs the whole map: world_size is %d", c->cfg.world_size);
  // from here on a failure discards the earlier result
  c->vor.valid = false;
  c->vor_stats = khr_voronoi_stats{};
  if (c->pl_from_voronoi) c->pl.valid = false;  // (khr_places_graph: its graph belongs to the field this call replaces)
  if (c->tf_from_voronoi) c->tf.valid = c->tfp_valid = false;  // (khr_travel_field: so does its travel field)
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int nx = rq->dims[0], ny = rq->dims[1], nz = rq->dims[2];
  const uint32_t n_wg = static_cast<uint32_t>(gridFor(n));
  const VorDense D = vorDense(n);
  size_t cub_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<int>(n_wg + 1), st));
  cub_bytes = std::max<size_t>(cub_bytes, 256);
  if (c->d_df_outer.count() < n || c->d_vor_keys.count() < n || c->d_vor_dense.count() < D.bytes || c->d_vor_cub.count() < cub_bytes || !c->d_vor_ctr || !c->h_vor) {
    HIP_TRY(hipStreamSynchronize(st));  // (whatever still reads the old blocks)
    if (c->d_df_outer.reserve(n) || c->d_vor_keys.reserve(n) || c->d_vor_dense.reserve(D.bytes) || c->d_vor_cub.reserve(cub_bytes) ||
        c->d_vor_ctr.reserve(VS_COUNT) || c->h_vor.reserve(VS_COUNT))
      return fail(KHR_ENOMEM, "khr_voronoi_field: work grids and outputs of %zu cells (%zu bytes)", n, 12 * n + D.bytes + cub_bytes);
  }
  uint8_t* const db = c->d_vor_dense;
  HIP_TRY(hipMemsetAsync(c->d_vor_ctr, 0, sizeof(unsigned long long) * VS_COUNT, st));
  DfGather g{};
  g.min_weight = rq->min_weight == 0.f ? c->cfg.mesh_min_weight : rq->min_weight;
  g.surface_distance = rq->surface_distance;
  g.unknown_is_obstacle = rq->unknown_is_obstacle;
  g.outer = c->d_df_outer;
  g.inner = nullptr;
  g.status = db + D.status;
  g.stats = c->d_vor_ctr;
  KHR_TRY(dfLaunchGather(c, rq->origin, rq->dims, ratio, g));
  // the x pass turns the seeds into keys and always runs; a y / z pass along one cell (or with R = 0) changes nothing
  uint64_t* const keys = c->d_vor_keys;
  auto pass = [&](auto axis, const int32_t* seeds) {
    constexpr int A = decltype(axis)::value;
    const PassGrid p = axisPassGrid(A, nx, ny, nz, kVorTileCells, kDfStrip);
    hipLaunchKernelGGL((k_vor_pass<A>), dim3(p.gx, p.gy), dim3(256), 0, st, seeds, keys, nx, ny, nz, R, p.per_wg);
  };
  pass(std::integral_constant<int, 0>(), g.outer);
  if (ny > 1 && R >= 1) pass(std::integral_constant<int, 1>(), nullptr);
  if (nz > 1 && R >= 1) pass(std::integral_constant<int, 2>(), nullptr);
  HIP_TRY(hipGetLastError());
  VorField f{};
  f.ox = rq->origin[0], f.oy = rq->origin[1], f.oz = rq->origin[2];
  f.nx = nx, f.ny = ny, f.nz = nz;
  f.keys = keys;
  f.rule.r2 = R * R;
  f.rule.cell_size = c->p.vs * static_cast<float>(ratio), f.rule.max_distance = rq->max_distance, f.rule.min_distance = rq->min_distance;
  f.rule.mode = rq->mode, f.rule.l1_sep = rq->parent_l1_separation, f.rule.cos_sep = rq->parent_cos_angle_separation;
  f.rule.min_basis = rq->min_basis == 0 ? 2 : rq->min_basis;
  f.distance = reinterpret_cast<float*>(db + D.distance), f.d2 = reinterpret_cast<int32_t*>(db + D.d2), f.status = db + D.status;
  f.site = reinterpret_cast<int32_t*>(db + D.site), f.basis = db + D.basis;
  f.wg_count = reinterpret_cast<uint32_t*>(db + D.wg_count);
  f.stats = c->d_vor_ctr;
  HIP_TRY(hipMemsetAsync(f.wg_count + n_wg, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_vor_classify, dim3(n_wg), dim3(256), 0, st, f);
  HIP_TRY(hipGetLastError());
  size_t tb = c->d_vor_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_vor_cub.get(), tb, f.wg_count, f.wg_count, static_cast<int>(n_wg + 1), st));
  // the one host wait: the counters
  unsigned long long* const h = c->h_vor;
  KHR_TRY(readWords(c, c->d_vor_ctr, h, sizeof(unsigned long long) * VS_COUNT));
  khr_voronoi_stats s{};
  s.n_observed = h[DFS_OBSERVED], s.n_obstacle = h[DFS_OBSTACLE], s.n_free = h[DFS_OBSERVED] - h[DFS_OBSTACLE], s.n_in_range = h[DFS_IN_RANGE];
  s.n_eligible = h[VS_ELIGIBLE], s.n_basis2 = h[VS_BASIS2], s.n_basis3 = h[VS_BASIS3], s.n_basis4 = h[VS_BASIS4], s.n_listed = h[VS_LISTED];
  if (s.n_listed > n || s.n_basis2 + s.n_basis3 + s.n_basis4 > s.n_eligible || s.n_eligible > s.n_in_range)
    return fail(KHR_EDEVICE, "khr_voronoi_field: inconsistent counts (%llu listed of %zu cells)", static_cast<unsigned long long>(s.n_listed), n);
  // the list; nothing is queued on the stream here (the wait above), so a growth frees nothing in use
  const VorList L = vorList(static_cast<size_t>(s.n_listed));
  if (c->d_vor_list.reserve(L.bytes)) return fail(KHR_ENOMEM, "khr_voronoi_field: a list of %llu cells (%zu bytes)", static_cast<unsigned long long>(s.n_listed), L.bytes);
  if (s.n_listed > 0) {
    uint8_t* const lb = c->d_vor_list;
    f.n_listed = static_cast<uint32_t>(s.n_listed);
    f.cells = reinterpret_cast<int32_t*>(lb + L.cells), f.cell_distance = reinterpret_cast<float*>(lb + L.distance), f.cell_basis = lb + L.basis;
    f.cell_sites = reinterpret_cast<int32_t*>(lb + L.sites);
    hipLaunchKernelGGL(k_vor_emit, dim3(n_wg), dim3(256), 0, st, f);
    HIP_TRY(hipGetLastError());
  }
  c->vor_stats = s;
  c->vor_cell_size = f.rule.cell_size;
  c->vor.set(rq->origin, rq->dims, n);
  if (stats) *stats = s;
  return KHR_OK;
}

int khr_voronoi_field_into(khr_ctx* c, int on_device, float* distance, int32_t* d2, uint8_t* status, int32_t* site, uint8_t* basis, int32_t* cells,
                           float* cell_distance, uint8_t* cell_basis, int32_t* cell_sites) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->vor.valid) return fail(KHR_ESTATE, "no successful khr_voronoi_field before khr_voronoi_field_into");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = c->vor.cells, m = static_cast<size_t>(c->vor_stats.n_listed);
  const VorDense D = vorDense(n);
  const VorList L = vorList(m);
  const uint8_t* const db = c->d_vor_dense;
  const uint8_t* const lb = c->d_vor_list;
  void* const dst[9] = {distance, d2, status, site, basis, cells, cell_distance, cell_basis, cell_sites};
  const void* const src[9] = {db + D.distance, db + D.d2, db + D.status, db + D.site, db + D.basis, lb + L.cells, lb + L.distance, lb + L.basis, lb + L.sites};
  const size_t bytes[9] = {4 * n, 4 * n, n, 4 * n, n, 12 * m, 4 * m, m, 12 * KHR_VOR_MAX_BASIS * m};
  return copyOut(c, c->h_vor_stage, on_device, dst, src, bytes, "khr_voronoi_field_into");
}

// ---- places and their links from the Voronoi cells of a box (khr_places_graph / khr_places_graph_from; ASSUMPTIONS.md A.21,
// device side: khr_kernels_places.h; the layouts of its buffers: plIn, plDense, plWork and plOut of khr_box_host.h) -------------
namespace {

// the request checks both calls share (KHR_EINVAL / KHR_ESTATE: nothing is done)
int plCheckRequest(khr_ctx* c, const khr_places_request* rq, const char* who) {
  if (rq->min_basis != 0 && (rq->min_basis < 2 || rq->min_basis > KHR_VOR_MAX_BASIS)) return fail(KHR_EINVAL, "%s: min_basis is %d: 0, 2, 3 or 4", who, rq->min_basis);
  if (rq->compression < 1 || rq->compression > KHR_PL_MAX_COMPRESSION)
    return fail(KHR_EINVAL, "%s: compression is %d cells: 1 .. %d", who, rq->compression, KHR_PL_MAX_COMPRESSION);
  if (!(rq->min_node_distance >= 0.f) || !std::isfinite(rq->min_node_distance))
    return fail(KHR_EINVAL, "%s: bad min_node_distance %g", who, static_cast<double>(rq->min_node_distance));
  if (c->cfg.world_size > 1) return fail(KHR_ESTATE, "%s needs the whole map: world_size is %d", who, c->cfg.world_size);
  return KHR_OK;
}

// the stage itself, on device arrays of the box's cells; two host waits
int plRun(khr_ctx* c, const khr_places_request* rq, const int32_t origin[3], const int32_t dims[3], const float* distance, const int32_t* d2,
          const uint8_t* basis, const int32_t* site, const PlDense& D, khr_places_stats* stats) {
  hipStream_t st = c->stream;
  const int nx = dims[0], ny = dims[1], nz = dims[2];
  const size_t n = static_cast<size_t>(nx) * ny * nz;
  uint8_t* const db = c->d_pl_dense;
  PlField f{};
  f.ox = origin[0], f.oy = origin[1], f.oz = origin[2];
  f.nx = nx, f.ny = ny, f.nz = nz;
  f.distance = distance, f.d2 = d2, f.basis = basis, f.site = site;
  f.min_basis = rq->min_basis == 0 ? 2 : rq->min_basis;
  f.min_node_distance = rq->min_node_distance;
  f.compression = rq->compression, f.edge = plTileBuckets(rq->compression) * rq->compression;
  f.tx0 = plFloorDiv(origin[0], f.edge), f.ty0 = plFloorDiv(origin[1], f.edge), f.tz0 = plFloorDiv(origin[2], f.edge);
  f.ntx = plFloorDiv(origin[0] + nx - 1, f.edge) - f.tx0 + 1, f.nty = plFloorDiv(origin[1] + ny - 1, f.edge) - f.ty0 + 1;
  f.ntz = plFloorDiv(origin[2] + nz - 1, f.edge) - f.tz0 + 1;
  f.label = reinterpret_cast<uint32_t*>(db + D.label), f.number = reinterpret_cast<uint32_t*>(db + D.number);
  f.pair_count = reinterpret_cast<uint32_t*>(db + D.pair_count);
  f.rec_key = reinterpret_cast<uint64_t*>(db + D.rec_key), f.rec_acc = reinterpret_cast<uint64_t*>(db + D.rec_acc);
  f.ctr = c->d_pl_ctr;
  const uint32_t n_wg = static_cast<uint32_t>(gridFor(n));
  HIP_TRY(hipMemsetAsync(c->d_pl_ctr, 0, sizeof(unsigned long long) * PLC_COUNT, st));
  HIP_TRY(hipMemsetAsync(f.label, 0xff, 4 * n, st));
  HIP_TRY(hipMemsetAsync(f.number, 0, 4 * (n + 1), st));
  HIP_TRY(hipMemsetAsync(f.pair_count + n, 0, 4, st));
  hipLaunchKernelGGL(k_pl_label, dim3(static_cast<unsigned>(f.ntx) * f.nty * f.ntz), dim3(256), 0, st, f);
  HIP_TRY(hipGetLastError());
  size_t tb = c->d_pl_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_pl_cub.get(), tb, f.number, f.number, static_cast<int>(n + 1), st));
  hipLaunchKernelGGL((k_pl_pairs<0>), dim3(n_wg), dim3(256), 0, st, f, static_cast<uint64_t*>(nullptr), static_cast<int32_t*>(nullptr), 0u);
  HIP_TRY(hipGetLastError());
  tb = c->d_pl_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_pl_cub.get(), tb, f.pair_count, f.pair_count, static_cast<int>(n + 1), st));
  // host wait 1: members, places, adjacent pairs
  unsigned long long* const h = c->h_pl;
  KHR_TRY(readWords(c, c->d_pl_ctr, h, sizeof(unsigned long long) * PLC_COUNT));
  khr_places_stats s{};
  s.n_members = h[PLC_MEMBERS], s.n_places_all = h[PLC_PLACES_ALL];
  const size_t m = static_cast<size_t>(h[PLC_PAIRS]), P = static_cast<size_t>(s.n_places_all);
  if (h[PLC_ERR] != 0)
    return fail(KHR_EDEVICE, "khr_places_graph: %llu tiles hold more than %d places", static_cast<unsigned long long>(h[PLC_ERR]), kPlSlots);
  if (s.n_members > n || P > s.n_members || m > 13 * n)
    return fail(KHR_EDEVICE, "khr_places_graph: inconsistent counts (%llu places of %llu members of %zu cells)", static_cast<unsigned long long>(P),
                static_cast<unsigned long long>(s.n_members), n);
  // the work lists and the sort's storage; nothing is queued on the stream here, so a growth frees nothing in use
  const PlWork W = plWork(m, P);
  size_t sort_bytes = 0, scan_bytes = 0;
  int end_bit = 33;
  while (end_bit < 64 && (P >> (end_bit - 32)) != 0) ++end_bit;
  if (m > 0)
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), static_cast<const int32_t*>(nullptr),
                                               static_cast<int32_t*>(nullptr), static_cast<int>(m), 0, end_bit, st));
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<int>(std::max(m, P) + 1), st));
  const size_t cub_bytes = std::max(sort_bytes, scan_bytes);
  if (c->d_pl_work.reserve(std::max<size_t>(W.bytes, 256)) || c->d_pl_cub.reserve(cub_bytes))
    return fail(KHR_ENOMEM, "khr_places_graph: work lists of %zu adjacent pairs and %zu places (%zu bytes)", m, P, W.bytes + cub_bytes);
  uint8_t* const wb = c->d_pl_work;
  PlGraph g{};
  g.n_pairs = static_cast<uint32_t>(m), g.n_places = static_cast<uint32_t>(P);
  g.keys = reinterpret_cast<const uint64_t*>(wb + W.keys_sorted), g.vals = reinterpret_cast<const int32_t*>(wb + W.vals_sorted);
  g.head = reinterpret_cast<uint32_t*>(wb + W.head), g.n_unique = reinterpret_cast<uint32_t*>(wb + W.n_unique);
  g.edge_a = reinterpret_cast<uint32_t*>(wb + W.edge_a), g.edge_b = reinterpret_cast<uint32_t*>(wb + W.edge_b);
  g.edge_clear = reinterpret_cast<int32_t*>(wb + W.edge_clear), g.edge_contacts = reinterpret_cast<uint32_t*>(wb + W.edge_contacts);
  g.edge_new = reinterpret_cast<uint32_t*>(wb + W.edge_new);
  g.parent = reinterpret_cast<uint32_t*>(wb + W.parent), g.root = reinterpret_cast<uint32_t*>(wb + W.root), g.size = reinterpret_cast<uint32_t*>(wb + W.size);
  g.place_new = reinterpret_cast<uint32_t*>(wb + W.place_new), g.comp_new = reinterpret_cast<uint32_t*>(wb + W.comp_new);
  g.min_size = static_cast<uint32_t>(std::max<int32_t>(rq->min_component_size, 1));
  g.ctr = c->d_pl_ctr;
  if (P > 0) {
    const unsigned wide = static_cast<unsigned>(gridFor(std::max(m, P)));
    HIP_TRY(hipMemsetAsync(g.n_unique, 0, 4, st));
    HIP_TRY(hipMemsetAsync(g.head + m, 0, 4, st));
    HIP_TRY(hipMemsetAsync(g.edge_new + m, 0, 4, st));
    HIP_TRY(hipMemsetAsync(g.size, 0, 4 * P, st));
    HIP_TRY(hipMemsetAsync(g.place_new + P, 0, 4, st));
    HIP_TRY(hipMemsetAsync(g.comp_new + P, 0, 4, st));
    if (m > 0) {
      HIP_TRY(hipMemsetAsync(g.edge_clear, 0, 4 * m, st));
      HIP_TRY(hipMemsetAsync(g.edge_contacts, 0, 4 * m, st));
      uint64_t* const keys = reinterpret_cast<uint64_t*>(wb + W.keys);
      int32_t* const vals = reinterpret_cast<int32_t*>(wb + W.vals);
      hipLaunchKernelGGL((k_pl_pairs<1>), dim3(n_wg), dim3(256), 0, st, f, keys, vals, g.n_pairs);
      HIP_TRY(hipGetLastError());
      tb = c->d_pl_cub.count();
      HIP_TRY(hipcub::DeviceRadixSort::SortPairs(c->d_pl_cub.get(), tb, static_cast<const uint64_t*>(keys), reinterpret_cast<uint64_t*>(wb + W.keys_sorted),
                                                 static_cast<const int32_t*>(vals), reinterpret_cast<int32_t*>(wb + W.vals_sorted), static_cast<int>(m), 0, end_bit, st));
    }
    hipLaunchKernelGGL(k_pl_edge_heads, dim3(wide), dim3(256), 0, st, g);
    HIP_TRY(hipGetLastError());
    if (m > 0) {
      tb = c->d_pl_cub.count();
      HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_pl_cub.get(), tb, g.head, g.head, static_cast<int>(m + 1), st));
      hipLaunchKernelGGL(k_pl_edge_reduce, dim3(gridFor(m)), dim3(256), 0, st, g);
      hipLaunchKernelGGL(k_pl_comp_union, dim3(gridFor(m)), dim3(256), 0, st, g);
    }
    hipLaunchKernelGGL(k_pl_comp_flatten, dim3(gridFor(P)), dim3(256), 0, st, g);
    hipLaunchKernelGGL(k_pl_comp_keep, dim3(wide), dim3(256), 0, st, g);
    HIP_TRY(hipGetLastError());
    tb = c->d_pl_cub.count();
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_pl_cub.get(), tb, g.place_new, g.place_new, static_cast<int>(P + 1), st));
    tb = c->d_pl_cub.count();
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_pl_cub.get(), tb, g.comp_new, g.comp_new, static_cast<int>(P + 1), st));
    tb = c->d_pl_cub.count();
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_pl_cub.get(), tb, g.edge_new, g.edge_new, static_cast<int>(m + 1), st));
    // host wait 2: the kept counts
    KHR_TRY(readWords(c, c->d_pl_ctr, h, sizeof(unsigned long long) * PLC_COUNT));
    s.n_edges_all = h[PLC_EDGES_ALL], s.n_components_all = h[PLC_COMPS_ALL], s.n_places = h[PLC_PLACES], s.n_edges = h[PLC_EDGES], s.n_components = h[PLC_COMPS];
    if (s.n_places > P || s.n_edges > s.n_edges_all || s.n_edges_all > m || s.n_components > s.n_components_all || s.n_components_all > P)
      return fail(KHR_EDEVICE, "khr_places_graph: inconsistent counts (%llu of %zu places, %llu of %llu edges)", static_cast<unsigned long long>(s.n_places), P,
                  static_cast<unsigned long long>(s.n_edges), static_cast<unsigned long long>(s.n_edges_all));
  }
  const PlOut L = plOut(static_cast<size_t>(s.n_places), static_cast<size_t>(s.n_edges));
  if (c->d_pl_out.reserve(L.bytes)) return fail(KHR_ENOMEM, "khr_places_graph: %llu places and %llu edges (%zu bytes)", static_cast<unsigned long long>(s.n_places),
                                                static_cast<unsigned long long>(s.n_edges), L.bytes);
  uint8_t* const ob = c->d_pl_out;
  PlResult r{};
  r.n_places = static_cast<uint32_t>(s.n_places), r.n_edges = static_cast<uint32_t>(s.n_edges);
  r.place = reinterpret_cast<int32_t*>(db + D.place);
  r.centre = reinterpret_cast<int32_t*>(ob + L.centre), r.centre_d2 = reinterpret_cast<int32_t*>(ob + L.centre_d2), r.radius = reinterpret_cast<float*>(ob + L.radius);
  r.basis = ob + L.basis, r.site = reinterpret_cast<int32_t*>(ob + L.site), r.n_cells = reinterpret_cast<uint32_t*>(ob + L.n_cells);
  r.sum = reinterpret_cast<long long*>(ob + L.sum), r.degree = reinterpret_cast<uint32_t*>(ob + L.degree), r.component = reinterpret_cast<uint32_t*>(ob + L.component);
  r.edge_a = reinterpret_cast<uint32_t*>(ob + L.edge_a), r.edge_b = reinterpret_cast<uint32_t*>(ob + L.edge_b);
  r.edge_clear = reinterpret_cast<int32_t*>(ob + L.edge_clear), r.edge_contacts = reinterpret_cast<uint32_t*>(ob + L.edge_contacts);
  if (s.n_places > 0) {
    HIP_TRY(hipMemsetAsync(r.degree, 0, 4 * static_cast<size_t>(s.n_places), st));
    hipLaunchKernelGGL(k_pl_finish_cells, dim3(n_wg), dim3(256), 0, st, f, g, r);
    if (s.n_edges > 0) hipLaunchKernelGGL(k_pl_finish_edges, dim3(gridFor(m)), dim3(256), 0, st, g, r);
    HIP_TRY(hipGetLastError());
  } else {
    HIP_TRY(hipMemsetAsync(r.place, 0xff, 4 * n, st));  // (no place is kept: -1 everywhere)
  }
  c->pl_stats = s;
  c->pl.set(origin, dims, n);
  if (stats) *stats = s;
  return KHR_OK;
}

// the buffers every call needs before its first launch, for a box of n cells (`in_bytes` of a host caller's field)
int plReserve(khr_ctx* c, size_t n, size_t in_bytes, const PlDense& D) {
  size_t cub_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<int>(n + 1), c->stream));
  cub_bytes = std::max<size_t>(cub_bytes, 256);
  if (c->d_pl_in.count() < in_bytes || c->d_pl_dense.count() < D.bytes || c->d_pl_cub.count() < cub_bytes || !c->d_pl_ctr || !c->h_pl) {
    HIP_TRY(hipStreamSynchronize(c->stream));  // (whatever still reads the old blocks)
    if (c->d_pl_in.reserve(in_bytes) || c->d_pl_dense.reserve(D.bytes) || c->d_pl_cub.reserve(cub_bytes) || c->d_pl_ctr.reserve(PLC_COUNT) || c->h_pl.reserve(PLC_COUNT))
      return fail(KHR_ENOMEM, "khr_places_graph: work arrays of %zu cells (%zu bytes)", n, in_bytes + D.bytes + cub_bytes);
  }
  return KHR_OK;
}

}  // namespace

int khr_places_graph(khr_ctx* c, const khr_places_request* rq, khr_places_stats* stats) {
  if (stats) *stats = khr_places_stats{};
  if (!c || !rq) return fail(KHR_EINVAL, "khr_places_graph: null argument");
  KHR_TRY(plCheckRequest(c, rq, "khr_places_graph"));
  if (!c->vor.valid) return fail(KHR_ESTATE, "no successful khr_voronoi_field before khr_places_graph");
  // from here on a failure discards the earlier result
  c->pl.valid = false;
  c->pl_stats = khr_places_stats{};
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = c->vor.cells;
  const PlDense D = plDense(n);
  KHR_TRY(plReserve(c, n, 0, D));
  const VorDense V = vorDense(n);
  const uint8_t* const vb = c->d_vor_dense;
  c->pl_from_voronoi = true;
  return plRun(c, rq, c->vor.origin, c->vor.dims, reinterpret_cast<const float*>(vb + V.distance), reinterpret_cast<const int32_t*>(vb + V.d2), vb + V.basis,
               reinterpret_cast<const int32_t*>(vb + V.site), D, stats);
}

int khr_places_graph_from(khr_ctx* c, const khr_places_request* rq, const int32_t* origin, const int32_t* dims, int on_device, const float* distance,
                          const int32_t* d2, const uint8_t* basis, const int32_t* site, khr_places_stats* stats) {
  if (stats) *stats = khr_places_stats{};
  if (!c || !rq || !origin || !dims || !distance || !d2 || !basis || !site) return fail(KHR_EINVAL, "khr_places_graph_from: null argument");
  KHR_TRY(plCheckRequest(c, rq, "khr_places_graph_from"));
  size_t n = 0;
  KHR_TRY(checkBox("khr_places_graph_from", origin, dims, 1, &n));
  // from here on a failure discards the earlier result
  c->pl.valid = false;
  c->pl_stats = khr_places_stats{};
  HIP_TRY(hipSetDevice(c->device));
  const PlDense D = plDense(n);
  c->pl_from_voronoi = false;
  if (on_device) {
    KHR_TRY(plReserve(c, n, 0, D));
    return plRun(c, rq, origin, dims, distance, d2, basis, site, D, stats);
  }
  // a host field: through the page-locked staging into a device copy
  const PlIn I = plIn(n);
  KHR_TRY(plReserve(c, n, I.bytes, D));
  if (c->h_pl_stage.reserve(I.bytes)) return fail(KHR_ENOMEM, "khr_places_graph_from: %zu bytes of page-locked staging", I.bytes);
  const void* const src[4] = {distance, d2, basis, site};
  const size_t bytes[4] = {4 * n, 4 * n, n, 4 * n};
  const size_t at[4] = {I.distance, I.d2, I.basis, I.site};
  KHR_TRY(copyIn(c, c->d_pl_in, c->h_pl_stage, src, bytes, at));
  const uint8_t* const ib = c->d_pl_in;
  return plRun(c, rq, origin, dims, reinterpret_cast<const float*>(ib + I.distance), reinterpret_cast<const int32_t*>(ib + I.d2), ib + I.basis,
               reinterpret_cast<const int32_t*>(ib + I.site), D, stats);
}

int khr_places_graph_box(khr_ctx* c, int32_t* origin, int32_t* dims) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->pl.valid) return fail(KHR_ESTATE, "no successful khr_places_graph before khr_places_graph_box");
  c->pl.boxOut(origin, dims);
  return KHR_OK;
}

int khr_places_graph_into(khr_ctx* c, int on_device, int32_t* place, int32_t* centre, int32_t* centre_d2, float* radius, uint8_t* basis, int32_t* site,
                          uint32_t* n_cells, int64_t* sum, uint32_t* degree, uint32_t* component, uint32_t* edge_a, uint32_t* edge_b,
                          int32_t* edge_clearance_d2, uint32_t* edge_n_contacts) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->pl.valid) return fail(KHR_ESTATE, "no successful khr_places_graph before khr_places_graph_into");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = c->pl.cells, p = static_cast<size_t>(c->pl_stats.n_places), e = static_cast<size_t>(c->pl_stats.n_edges);
  const PlDense D = plDense(n);
  const PlOut L = plOut(p, e);
  const uint8_t* const db = c->d_pl_dense;
  const uint8_t* const ob = c->d_pl_out;
  constexpr int K = 14;
  void* const dst[K] = {place, centre, centre_d2, radius, basis, site, n_cells, sum, degree, component, edge_a, edge_b, edge_clearance_d2, edge_n_contacts};
  const void* const src[K] = {db + D.place, ob + L.centre, ob + L.centre_d2, ob + L.radius, ob + L.basis, ob + L.site, ob + L.n_cells, ob + L.sum, ob + L.degree,
                              ob + L.component, ob + L.edge_a, ob + L.edge_b, ob + L.edge_clear, ob + L.edge_contacts};
  const size_t bytes[K] = {4 * n, 12 * p, 4 * p, 4 * p, p, 12 * p, 4 * p, 24 * p, 4 * p, 4 * p, 4 * e, 4 * e, 4 * e, 4 * e};
  return copyOut(c, c->h_pl_stage, on_device, dst, src, bytes, "khr_places_graph_into");
}

// ---- clearance-bounded travel cost and paths in a box of cells (khr_travel_field / khr_travel_field_from / khr_travel_paths;
// ASSUMPTIONS.md A.22, device side: khr_kernels_travel.h; the layouts of its buffers: tfIn, tfDense and tfStarts of khr_box_host.h)
namespace {

static_assert(kTfRoundsPerWait == KHR_TF_ROUNDS_PER_WAIT && kTfEdge == KHR_TF_TILE_EDGE && kTfUnreached == KHR_TF_UNREACHED, "khr_kernels_travel.h and khronos_amd.h");
constexpr uint32_t kTfMaxGoals = 1u << 20, kTfMaxStarts = 1u << 20;
constexpr uint64_t kTfMaxPathCells = uint64_t(1) << 26;

inline size_t tfTiles(const int32_t dims[3]) {
  size_t t = 1;
  for (int a = 0; a < 3; ++a) t *= static_cast<size_t>((dims[a] + kTfEdge - 1) / kTfEdge);
  return t;
}

// the request checks both calls share (KHR_EINVAL / KHR_ESTATE: nothing is done)
int tfCheckRequest(khr_ctx* c, const khr_travel_request* rq, uint64_t n_goals, const char* who) {
  if (rq->connectivity != 6 && rq->connectivity != 18 && rq->connectivity != 26) return fail(KHR_EINVAL, "%s: connectivity is %d: 6, 18 or 26", who, rq->connectivity);
  if (!(rq->clearance >= 0.f) || !std::isfinite(rq->clearance)) return fail(KHR_EINVAL, "%s: bad clearance %g", who, static_cast<double>(rq->clearance));
  if (n_goals < 1 || n_goals > kTfMaxGoals) return fail(KHR_EINVAL, "%s: %llu goals: 1 .. %u", who, static_cast<unsigned long long>(n_goals), kTfMaxGoals);
  if (c->cfg.world_size > 1) return fail(KHR_ESTATE, "%s needs the whole map: world_size is %d", who, c->cfg.world_size);
  return KHR_OK;
}

// the buffers a call needs before its first launch: a box of n cells in `tiles` tiles, `in_bytes` of a host caller's field and goals
int tfReserve(khr_ctx* c, size_t in_bytes, const TfDense& D) {
  constexpr size_t kMirror = TFC_COUNT + kTfRoundsPerWait + 1;  // the counters, the rounds' words, the paths' total
  if (c->d_tf_in.count() < in_bytes || c->d_tf_dense.count() < D.bytes || !c->d_tf_ctr || !c->h_tf || c->h_tf_stage.count() < in_bytes) {
    HIP_TRY(hipStreamSynchronize(c->stream));  // (whatever still reads the old blocks)
    if (c->d_tf_in.reserve(in_bytes) || c->d_tf_dense.reserve(D.bytes) || c->d_tf_ctr.reserve(TFC_COUNT) || c->h_tf.reserve(kMirror) || c->h_tf_stage.reserve(in_bytes))
      return fail(KHR_ENOMEM, "khr_travel_field: work arrays of %zu bytes", in_bytes + D.bytes);
  }
  return KHR_OK;
}

// the stage itself, on device arrays of the box's cells and of the goals
int tfRun(khr_ctx* c, const khr_travel_request* rq, const int32_t origin[3], const int32_t dims[3], const float* distance, const uint8_t* status,
          const int32_t* goals, uint64_t n_goals, const TfDense& D, khr_travel_stats* stats) {
  hipStream_t st = c->stream;
  const size_t n = static_cast<size_t>(dims[0]) * dims[1] * dims[2], tiles = tfTiles(dims);
  uint8_t* const db = c->d_tf_dense;
  TfField f{};
  f.ox = origin[0], f.oy = origin[1], f.oz = origin[2];
  f.nx = dims[0], f.ny = dims[1], f.nz = dims[2];
  f.ntx = (dims[0] + kTfEdge - 1) / kTfEdge, f.nty = (dims[1] + kTfEdge - 1) / kTfEdge, f.ntz = (dims[2] + kTfEdge - 1) / kTfEdge;
  f.distance = distance, f.status = status;
  f.clearance = rq->clearance, f.allow_unknown = rq->allow_unknown, f.max_cost = rq->max_cost;
  f.goals = goals, f.n_goals = static_cast<uint32_t>(n_goals);
  f.mask = db + D.mask, f.keys = reinterpret_cast<unsigned long long*>(db + D.keys), f.flags = db + D.flags;
  f.go_on = reinterpret_cast<uint32_t*>(db + D.go_on);
  f.ctr = c->d_tf_ctr;
  f.cost = reinterpret_cast<uint32_t*>(db + D.cost), f.goal = reinterpret_cast<int32_t*>(db + D.goal), f.parent = db + D.parent;
  HIP_TRY(hipMemsetAsync(c->d_tf_ctr, 0, sizeof(unsigned long long) * TFC_COUNT, st));
  HIP_TRY(hipMemsetAsync(f.keys, 0xff, 8 * n, st));
  HIP_TRY(hipMemsetAsync(f.flags, 0, 2 * tiles, st));
  hipLaunchKernelGGL(k_tf_seed, dim3(gridFor(std::max<size_t>(n, static_cast<size_t>(n_goals)))), dim3(256), 0, st, f);
  HIP_TRY(hipGetLastError());
  // the rounds: kTfRoundsPerWait launches, then one look at their words.  A shortest path crosses fewer than n tile faces and a
  // round carries every key across one, so n rounds settle any box; more than that is an error, not a longer loop.
  unsigned long long* const h = c->h_tf;
  uint32_t* const h_go = reinterpret_cast<uint32_t*>(h + TFC_COUNT);
  const uint64_t cap = static_cast<uint64_t>(n) + kTfRoundsPerWait;
  khr_travel_stats s{};
  uint64_t queued = 0;
  bool carry = true;
  while (carry) {
    if (queued >= cap) return fail(KHR_EDEVICE, "khr_travel_field: not settled after %llu rounds over %zu cells", static_cast<unsigned long long>(queued), n);
    HIP_TRY(hipMemsetAsync(f.go_on, 0, 4 * kTfRoundsPerWait, st));
    for (uint32_t j = 0; j < kTfRoundsPerWait; ++j) {
      const uint32_t round = static_cast<uint32_t>(queued) + j;
      if (rq->connectivity == 6) tfLaunchRelax<6>(f, static_cast<unsigned>(tiles), round, j, st);
      else if (rq->connectivity == 18) tfLaunchRelax<18>(f, static_cast<unsigned>(tiles), round, j, st);
      else tfLaunchRelax<26>(f, static_cast<unsigned>(tiles), round, j, st);
    }
    HIP_TRY(hipGetLastError());
    queued += kTfRoundsPerWait;
    if (queued == kTfRoundsPerWait) HIP_TRY(hipMemcpyAsync(h, c->d_tf_ctr, sizeof(unsigned long long) * TFC_COUNT, hipMemcpyDeviceToHost, st));
    KHR_TRY(readWords(c, f.go_on, h_go, 4 * kTfRoundsPerWait));
    ++s.n_waits;
    if (queued == kTfRoundsPerWait && h[TFC_GOALS_USED] == 0) carry = false;  // (no usable goal: no tile ran)
    // rounds in which a tile ran: the batch's first if the batch before said so, round j + 1 if round j raised a flag
    if (carry) ++s.n_rounds;
    for (uint32_t j = 0; j + 1 < kTfRoundsPerWait; ++j) s.n_rounds += h_go[j] ? 1 : 0;
    carry = h_go[kTfRoundsPerWait - 1] != 0;
  }
  if (rq->connectivity == 6) tfLaunchFinish<6>(f, n, st);
  else if (rq->connectivity == 18) tfLaunchFinish<18>(f, n, st);
  else tfLaunchFinish<26>(f, n, st);
  HIP_TRY(hipGetLastError());
  KHR_TRY(readWords(c, c->d_tf_ctr, h, sizeof(unsigned long long) * TFC_COUNT));
  s.n_traversable = h[TFC_TRAVERSABLE], s.n_goals_used = h[TFC_GOALS_USED], s.n_reached = h[TFC_REACHED], s.max_cost = h[TFC_MAX_COST];
  if (s.n_traversable > n || s.n_reached > s.n_traversable || s.n_goals_used > n_goals)
    return fail(KHR_EDEVICE, "khr_travel_field: inconsistent counts (%llu reached of %llu traversable of %zu cells)", static_cast<unsigned long long>(s.n_reached),
                static_cast<unsigned long long>(s.n_traversable), n);
  c->tf_stats = s;
  c->tf.set(origin, dims, n);
  if (stats) *stats = s;
  return KHR_OK;
}

}  // namespace

int khr_travel_field(khr_ctx* c, const khr_travel_request* rq, const int32_t* goals, uint64_t n_goals, int goals_on_device, khr_travel_stats* stats) {
  if (stats) *stats = khr_travel_stats{};
  if (!c || !rq || !goals) return fail(KHR_EINVAL, "khr_travel_field: null argument");
  KHR_TRY(tfCheckRequest(c, rq, n_goals, "khr_travel_field"));
  if (!c->vor.valid) return fail(KHR_ESTATE, "no successful khr_voronoi_field before khr_travel_field");
  // from here on a failure discards the earlier result
  c->tf.valid = c->tfp_valid = false;
  c->tf_stats = khr_travel_stats{};
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = c->vor.cells;
  const TfDense D = tfDense(n, tfTiles(c->vor.dims));
  const size_t goal_bytes = 12 * static_cast<size_t>(n_goals);
  KHR_TRY(tfReserve(c, goals_on_device ? 0 : Arena::align(goal_bytes), D));
  if (!goals_on_device) KHR_TRY(copyIn(c, c->d_tf_in, c->h_tf_stage, goals, goal_bytes));
  const VorDense V = vorDense(n);
  const uint8_t* const vb = c->d_vor_dense;
  c->tf_from_voronoi = true;
  return tfRun(c, rq, c->vor.origin, c->vor.dims, reinterpret_cast<const float*>(vb + V.distance), vb + V.status,
               goals_on_device ? goals : reinterpret_cast<const int32_t*>(c->d_tf_in.get()), n_goals, D, stats);
}

int khr_travel_field_from(khr_ctx* c, const khr_travel_request* rq, const int32_t* origin, const int32_t* dims, int on_device, const float* distance,
                          const uint8_t* status, const int32_t* goals, uint64_t n_goals, khr_travel_stats* stats) {
  if (stats) *stats = khr_travel_stats{};
  if (!c || !rq || !origin || !dims || !distance || !status || !goals) return fail(KHR_EINVAL, "khr_travel_field_from: null argument");
  KHR_TRY(tfCheckRequest(c, rq, n_goals, "khr_travel_field_from"));
  size_t n = 0;
  KHR_TRY(checkBox("khr_travel_field_from", origin, dims, 1, &n));
  // from here on a failure discards the earlier result
  c->tf.valid = c->tfp_valid = false;
  c->tf_stats = khr_travel_stats{};
  HIP_TRY(hipSetDevice(c->device));
  const TfDense D = tfDense(n, tfTiles(dims));
  c->tf_from_voronoi = false;
  if (on_device) {
    KHR_TRY(tfReserve(c, 0, D));
    return tfRun(c, rq, origin, dims, distance, status, goals, n_goals, D, stats);
  }
  // a host field and host goals: through the page-locked staging into a device copy
  const TfIn I = tfIn(n, static_cast<size_t>(n_goals));
  KHR_TRY(tfReserve(c, I.bytes, D));
  const void* const src[3] = {distance, status, goals};
  const size_t bytes[3] = {4 * n, n, 12 * static_cast<size_t>(n_goals)};
  const size_t at[3] = {I.distance, I.status, I.goals};
  KHR_TRY(copyIn(c, c->d_tf_in, c->h_tf_stage, src, bytes, at));
  const uint8_t* const ib = c->d_tf_in;
  return tfRun(c, rq, origin, dims, reinterpret_cast<const float*>(ib + I.distance), ib + I.status, reinterpret_cast<const int32_t*>(ib + I.goals), n_goals, D, stats);
}

int khr_travel_field_box(khr_ctx* c, int32_t* origin, int32_t* dims) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->tf.valid) return fail(KHR_ESTATE, "no successful khr_travel_field before khr_travel_field_box");
  c->tf.boxOut(origin, dims);
  return KHR_OK;
}

int khr_travel_field_into(khr_ctx* c, int on_device, uint32_t* cost, int32_t* goal, uint8_t* parent) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->tf.valid) return fail(KHR_ESTATE, "no successful khr_travel_field before khr_travel_field_into");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = c->tf.cells;
  const TfDense D = tfDense(n, tfTiles(c->tf.dims));
  const uint8_t* const db = c->d_tf_dense;
  void* const dst[3] = {cost, goal, parent};
  const void* const src[3] = {db + D.cost, db + D.goal, db + D.parent};
  const size_t bytes[3] = {4 * n, 4 * n, n};
  return copyOut(c, c->h_tf_stage, on_device, dst, src, bytes, "khr_travel_field_into");
}

int khr_travel_paths(khr_ctx* c, uint64_t n_starts, const int32_t* starts, int on_device, uint64_t* n_cells_total) {
  if (n_cells_total) *n_cells_total = 0;
  if (!c || !starts) return fail(KHR_EINVAL, "khr_travel_paths: null argument");
  if (n_starts < 1 || n_starts > kTfMaxStarts) return fail(KHR_EINVAL, "khr_travel_paths: %llu starts: 1 .. %u", static_cast<unsigned long long>(n_starts), kTfMaxStarts);
  if (!c->tf.valid) return fail(KHR_ESTATE, "no successful khr_travel_field before khr_travel_paths");
  // from here on a failure discards the earlier paths (the travel field stays)
  c->tfp_valid = false;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t s = static_cast<size_t>(n_starts);
  const TfStarts L = tfStarts(s);
  size_t cub_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, static_cast<long long*>(nullptr), static_cast<long long*>(nullptr), static_cast<int>(s + 1), st));
  cub_bytes = std::max<size_t>(cub_bytes, 256);
  const size_t stage_bytes = on_device ? 0 : 12 * s;
  if (c->d_tf_path.count() < L.bytes || c->d_tf_cub.count() < cub_bytes || c->h_tf_stage.count() < stage_bytes) {
    HIP_TRY(hipStreamSynchronize(st));  // (whatever still reads the old blocks)
    if (c->d_tf_path.reserve(L.bytes) || c->d_tf_cub.reserve(cub_bytes) || c->h_tf_stage.reserve(stage_bytes))
      return fail(KHR_ENOMEM, "khr_travel_paths: work arrays of %zu starts (%zu bytes)", s, L.bytes + cub_bytes);
  }
  uint8_t* const pb = c->d_tf_path;
  if (on_device) HIP_TRY(hipMemcpyAsync(pb + L.starts, starts, 12 * s, hipMemcpyDeviceToDevice, st));
  else KHR_TRY(copyIn(c, pb + L.starts, c->h_tf_stage, starts, 12 * s));
  const TfDense D = tfDense(c->tf.cells, tfTiles(c->tf.dims));
  const uint8_t* const db = c->d_tf_dense;
  TfPaths p{};
  p.ox = c->tf.origin[0], p.oy = c->tf.origin[1], p.oz = c->tf.origin[2];
  p.nx = c->tf.dims[0], p.ny = c->tf.dims[1], p.nz = c->tf.dims[2];
  p.cost = reinterpret_cast<const uint32_t*>(db + D.cost), p.goal = reinterpret_cast<const int32_t*>(db + D.goal), p.parent = db + D.parent;
  p.starts = reinterpret_cast<const int32_t*>(pb + L.starts), p.n_starts = static_cast<uint32_t>(s);
  p.offsets = reinterpret_cast<long long*>(pb + L.offsets);
  p.path_cost = reinterpret_cast<uint32_t*>(pb + L.path_cost), p.path_goal = reinterpret_cast<int32_t*>(pb + L.path_goal);
  hipLaunchKernelGGL(k_tf_path_count, dim3(gridFor(s + 1)), dim3(256), 0, st, p);
  HIP_TRY(hipGetLastError());
  size_t tb = c->d_tf_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_tf_cub.get(), tb, p.offsets, p.offsets, static_cast<int>(s + 1), st));
  // the one host wait: the total sizes the list
  unsigned long long* const h_total = c->h_tf + TFC_COUNT + kTfRoundsPerWait;
  KHR_TRY(readWords(c, p.offsets + s, h_total, 8));
  const uint64_t total = *h_total;
  if (total > kTfMaxPathCells)
    return fail(KHR_ENOMEM, "khr_travel_paths: the paths hold %llu cells: at most 2^26 in one call", static_cast<unsigned long long>(total));
  if (c->d_tf_cells.reserve(std::max<size_t>(12 * static_cast<size_t>(total), 256)))
    return fail(KHR_ENOMEM, "khr_travel_paths: a list of %llu cells (%zu bytes)", static_cast<unsigned long long>(total), 12 * static_cast<size_t>(total));
  p.cells = reinterpret_cast<int32_t*>(c->d_tf_cells.get()), p.n_cells_total = static_cast<long long>(total);
  if (total > 0) {
    hipLaunchKernelGGL(k_tf_path_emit, dim3(gridFor(s)), dim3(256), 0, st, p);
    HIP_TRY(hipGetLastError());
  }
  c->tfp_starts = s, c->tfp_total = static_cast<size_t>(total);
  c->tfp_valid = true;
  if (n_cells_total) *n_cells_total = total;
  return KHR_OK;
}

int khr_travel_paths_into(khr_ctx* c, int on_device, int64_t* offsets, int32_t* cells, uint32_t* path_cost, int32_t* path_goal) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->tf.valid || !c->tfp_valid) return fail(KHR_ESTATE, "no successful khr_travel_paths before khr_travel_paths_into");
  HIP_TRY(hipSetDevice(c->device));
  const size_t s = c->tfp_starts, total = c->tfp_total;
  const TfStarts L = tfStarts(s);
  const uint8_t* const pb = c->d_tf_path;
  void* const dst[4] = {offsets, cells, path_cost, path_goal};
  const void* const src[4] = {pb + L.offsets, c->d_tf_cells.get(), pb + L.path_cost, pb + L.path_goal};
  const size_t bytes[4] = {8 * (s + 1), 12 * total, 4 * s, 4 * s};
  return copyOut(c, c->h_tf_stage, on_device, dst, src, bytes, "khr_travel_paths_into");
}

// ---- the live map as a registration target (khr_align_linearize / khr_align_frame; ASSUMPTIONS.md A.14, device side:
// khr_kernels_align.h) ---------------------------------------------------------------------------------------------------------
namespace {

struct AlignPlan {
  bool depth_form = false;
  long long n = 0;       // lanes
  size_t src_bytes = 0;  // source bytes, weight bytes (0 without weights)
  size_t w_bytes = 0;
  int ws = 0;
  float min_weight = 0.f, gate = 0.f;
};

// the request's checks (nothing is touched before they pass)
int alignCheck(khr_ctx* c, const khr_align_request* rq, AlignPlan* pl) {
  if (!c || !rq) return fail(KHR_EINVAL, "null argument");
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(rq->world_T_source[i])) return fail(KHR_EINVAL, "world_T_source is not finite");
  if (!(rq->min_weight >= 0.f) || !std::isfinite(rq->min_weight)) return fail(KHR_EINVAL, "bad min_weight %g", static_cast<double>(rq->min_weight));
  if (!(rq->gate >= 0.f) || !std::isfinite(rq->gate)) return fail(KHR_EINVAL, "bad gate %g", static_cast<double>(rq->gate));
  if (!(rq->huber_delta >= 0.f) || !std::isfinite(rq->huber_delta)) return fail(KHR_EINVAL, "bad huber_delta %g", static_cast<double>(rq->huber_delta));
  pl->gate = rq->gate == 0.f ? c->cfg.truncation_distance : rq->gate;
  if (!(pl->gate <= 64.f)) return fail(KHR_EINVAL, "gate %g m: the sums are proven not to wrap up to 64 m", static_cast<double>(pl->gate));
  pl->min_weight = rq->min_weight == 0.f ? c->cfg.mesh_min_weight : rq->min_weight;
  if (rq->points && rq->depth) return fail(KHR_EINVAL, "both a point list and a depth image");
  if (rq->depth) {
    const khr_sensor& sn = rq->sensor;
    if (rq->stride < 1) return fail(KHR_EINVAL, "stride %d", rq->stride);
    if (sn.width <= 0 || sn.height <= 0 || static_cast<int64_t>(sn.width) * sn.height > (int64_t(1) << 30))
      return fail(KHR_EINVAL, "bad image size %d x %d", sn.width, sn.height);
    if (!std::isfinite(sn.fx) || !std::isfinite(sn.fy) || sn.fx == 0.f || sn.fy == 0.f || !std::isfinite(sn.cx) || !std::isfinite(sn.cy))
      return fail(KHR_EINVAL, "bad intrinsics");
    if (!std::isfinite(sn.min_range) || !std::isfinite(sn.max_range) || sn.min_range < 0.f || sn.max_range < sn.min_range)
      return fail(KHR_EINVAL, "bad range limits [%g, %g]", static_cast<double>(sn.min_range), static_cast<double>(sn.max_range));
    pl->depth_form = true;
    // (in 64 bits: width + stride - 1 may pass 2^31)
    const long long st = rq->stride;
    pl->ws = static_cast<int>((sn.width + st - 1) / st);
    pl->n = static_cast<long long>(pl->ws) * ((sn.height + st - 1) / st);
    pl->src_bytes = static_cast<size_t>(sn.width) * sn.height * 4;
    pl->w_bytes = rq->weights ? pl->src_bytes : 0;
  } else {
    if (rq->n < 0) return fail(KHR_EINVAL, "negative point count %lld", static_cast<long long>(rq->n));
    if (rq->n > 0 && !rq->points) return fail(KHR_EINVAL, "neither a point list nor a depth image");
    pl->n = rq->n;
    pl->src_bytes = static_cast<size_t>(rq->n) * 12;
    pl->w_bytes = rq->weights ? static_cast<size_t>(rq->n) * 4 : 0;
  }
  if (pl->n > KHR_ALIGN_MAX_SOURCES) return fail(KHR_EINVAL, "%lld sources, at most %d per call", pl->n, KHR_ALIGN_MAX_SOURCES);
  if (c->cfg.world_size > 1) return fail(KHR_ESTATE, "khr_align_linearize needs the whole map: world_size is %d", c->cfg.world_size);
  return KHR_OK;
}

// the accumulator pair, and for a host source its copy in the device staging (queued on the stream); *d_src / *d_w: what the kernel reads
int alignPrepare(khr_ctx* c, const khr_align_request* rq, const AlignPlan& pl, int on_device, const float** d_src, const float** d_w) {
  HIP_TRY(hipSetDevice(c->device));
  constexpr size_t acc_bytes = sizeof(unsigned long long) * kAlignWords * kAlignAccStride;
  constexpr size_t acc_words = acc_bytes / sizeof(unsigned long long);
  if (!c->d_align_acc && c->d_align_acc.alloc(acc_words)) return fail(KHR_ENOMEM, "align accumulator");
  if (!c->h_align_acc && c->h_align_acc.alloc(acc_words)) return fail(KHR_ENOMEM, "page-locked align accumulator");
  const float* src = pl.depth_form ? rq->depth : rq->points;
  *d_src = src;
  *d_w = rq->weights;
  if (on_device || pl.n == 0) return KHR_OK;
  const size_t w_off = (pl.src_bytes + 255) / 256 * 256, stage_bytes = w_off + (pl.w_bytes + 255) / 256 * 256;
  KHR_TRY(reserveStagePair(c->d_align_stage, c->h_align_stage, stage_bytes, "align"));
  std::memcpy(c->h_align_stage, src, pl.src_bytes);
  HIP_TRY(hipMemcpyAsync(c->d_align_stage, c->h_align_stage, pl.src_bytes, hipMemcpyHostToDevice, c->stream));
  *d_src = reinterpret_cast<const float*>(c->d_align_stage.get());
  if (pl.w_bytes) {
    std::memcpy(c->h_align_stage + w_off, rq->weights, pl.w_bytes);
    HIP_TRY(hipMemcpyAsync(c->d_align_stage + w_off, c->h_align_stage + w_off, pl.w_bytes, hipMemcpyHostToDevice, c->stream));
    *d_w = reinterpret_cast<const float*>(c->d_align_stage + w_off);
  }
  return KHR_OK;
}

// one evaluation at `pose` over a device-resident source: zero, launch, copy back, one wait
int alignEvaluate(khr_ctx* c, const khr_align_request* rq, const AlignPlan& pl, const float* d_src, const float* d_w, const double* pose,
                  uint64_t* words) {
  if (pl.n == 0) {
    std::memset(words, 0, sizeof(uint64_t) * KHR_ALIGN_WORDS);
    return KHR_OK;
  }
  constexpr size_t acc_bytes = sizeof(unsigned long long) * kAlignWords * kAlignAccStride;
  AlignArgs a{};
  a.n = static_cast<uint32_t>(pl.n);
  a.points = pl.depth_form ? nullptr : d_src;
  a.depth = pl.depth_form ? d_src : nullptr;
  a.weights = d_w;
  a.W = static_cast<uint32_t>(pl.depth_form ? rq->sensor.width : 0);
  a.ws = static_cast<uint32_t>(pl.depth_form ? pl.ws : 1);
  a.stride = static_cast<uint32_t>(pl.depth_form ? rq->stride : 1);
  a.fx = rq->sensor.fx;
  a.fy = rq->sensor.fy;
  a.cx = rq->sensor.cx;
  a.cy = rq->sensor.cy;
  a.min_range = rq->sensor.min_range;
  a.max_range = rq->sensor.max_range;
  {
    float R[9], t[3];
    makePose(pose, R, t, a.Rw, a.tw);
  }
  a.min_weight = pl.min_weight;
  a.gate = pl.gate;
  a.huber_delta = rq->huber_delta;
  a.acc = c->d_align_acc;
  HIP_TRY(hipMemsetAsync(c->d_align_acc, 0, acc_bytes, c->stream));
  const dim3 grid(static_cast<unsigned>((pl.n + 255) / 256));  // (at most 4096 workgroups: n <= 2^20)
  const bool depth_form = pl.depth_form;
  int rc = dispatchVps(c, [&](auto vps) {
    if (depth_form)
      hipLaunchKernelGGL((k_align_linearize<decltype(vps)::value, ALIGN_DEPTH>), grid, dim3(256), 0, c->stream, c->m, c->p, a);
    else
      hipLaunchKernelGGL((k_align_linearize<decltype(vps)::value, ALIGN_POINTS>), grid, dim3(256), 0, c->stream, c->m, c->p, a);
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->h_align_acc, c->d_align_acc, acc_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int w = 0; w < KHR_ALIGN_WORDS; ++w) words[w] = c->h_align_acc[static_cast<size_t>(w) * kAlignAccStride];
  return KHR_OK;
}

// L L^T = A for the 6 x 6 symmetric A (upper triangle read), then L y = rhs, L^T x = y; false at a pivot that is not positive
bool alignCholeskySolve(const double (&A)[6][6], const double (&rhs)[6], double (&x)[6]) {
  double L[6][6] = {};
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > 0.0) || !std::isfinite(s)) return false;
    L[j][j] = std::sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double v = A[j][i];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = rhs[i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  return true;
}

// R <- exp(omega^) R, t <- t + v on the row-major 4 x 4 double pose (Rodrigues; the series below 1e-8 rad)
void alignApplyTwist(double* T, const double (&xi)[6]) {
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = std::sqrt(th2);
  double A, B;  // sin(th) / th, (1 - cos(th)) / th^2
  if (th < 1e-8) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
  } else {
    A = std::sin(th) / th;
    B = (1.0 - std::cos(th)) / th2;
  }
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double E[3][3];
  for (int r = 0; r < 3; ++r)
    for (int cc = 0; cc < 3; ++cc) {
      double k2 = 0.0;
      for (int k = 0; k < 3; ++k) k2 += K[r][k] * K[k][cc];
      E[r][cc] = (r == cc ? 1.0 : 0.0) + A * K[r][cc] + B * k2;
    }
  double Rn[3][3];
  for (int r = 0; r < 3; ++r)
    for (int cc = 0; cc < 3; ++cc) {
      double v = 0.0;
      for (int k = 0; k < 3; ++k) v += E[r][k] * T[4 * k + cc];
      Rn[r][cc] = v;
    }
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc) T[4 * r + cc] = Rn[r][cc];
    T[4 * r + 3] += xi[3 + r];
  }
}

}  // namespace

int khr_align_linearize(khr_ctx* c, const khr_align_request* rq, int on_device, uint64_t* words) {
  AlignPlan pl;
  if (!words) return fail(KHR_EINVAL, "null argument");
  int rc = alignCheck(c, rq, &pl);
  if (rc) return rc;
  const float *d_src = nullptr, *d_w = nullptr;
  if ((rc = alignPrepare(c, rq, pl, on_device, &d_src, &d_w))) return rc;
  return alignEvaluate(c, rq, pl, d_src, d_w, rq->world_T_source, words);
}

int khr_align_frame(khr_ctx* c, const khr_align_request* rq, int on_device, const khr_align_options* options, double* world_T_source_out,
                    khr_align_result* result) {
  AlignPlan pl;
  if (!world_T_source_out) return fail(KHR_EINVAL, "null argument");
  int rc = alignCheck(c, rq, &pl);
  if (rc) return rc;
  khr_align_options o{10, 64, 1e-4, 1e-5, 1e-5};
  if (options) o = *options;
  if (!(o.lambda >= 0.0) || !std::isfinite(o.lambda) || !(o.eps_rot >= 0.0) || !(o.eps_trans >= 0.0))
    return fail(KHR_EINVAL, "bad align options (lambda %g, eps_rot %g, eps_trans %g)", o.lambda, o.eps_rot, o.eps_trans);
  if (o.max_iterations <= 0) o.max_iterations = 10;
  if (o.min_inliers < 6) o.min_inliers = 6;
  const float *d_src = nullptr, *d_w = nullptr;
  if ((rc = alignPrepare(c, rq, pl, on_device, &d_src, &d_w))) return rc;  // (a host source is staged once for all iterations)
  khr_align_result res{};
  double T[16];
  std::memcpy(T, rq->world_T_source, sizeof(T));
  const double scale = 1.0 / 16777216.0;
  bool lost = false;
  for (int it = 0; it < o.max_iterations; ++it) {
    uint64_t words[KHR_ALIGN_WORDS];
    if ((rc = alignEvaluate(c, rq, pl, d_src, d_w, T, words))) return rc;
    double H[6][6], b[6];
    int w = 0;
    for (int r = 0; r < 6; ++r)
      for (int cc = r; cc < 6; ++cc, ++w) {
        res.H[w] = static_cast<double>(static_cast<int64_t>(words[w])) * scale;
        H[r][cc] = H[cc][r] = res.H[w];
      }
    for (int r = 0; r < 6; ++r) b[r] = res.b[r] = static_cast<double>(static_cast<int64_t>(words[AW_B + r])) * scale;
    const uint64_t n_in = words[AW_INLIER];
    const double e = static_cast<double>(static_cast<int64_t>(words[AW_E])) * scale;
    const double sum_w = static_cast<double>(words[AW_WEIGHT]) * scale;  // sum of weight * rho over the inliers
    const double rmse = sum_w > 0.0 ? std::sqrt(e / sum_w) : 0.0;
    if (it == 0) {
      res.n_inlier_first = n_in;
      res.rmse_first = rmse;
    }
    res.n_inlier_last = n_in;
    res.rmse_last = rmse;
    if (n_in < static_cast<uint64_t>(o.min_inliers)) {
      lost = true;
      break;
    }
    double A[6][6], rhs[6], xi[6];
    for (int r = 0; r < 6; ++r) {
      for (int cc = 0; cc < 6; ++cc) A[r][cc] = H[r][cc];
      A[r][r] = H[r][r] + o.lambda * H[r][r];
      rhs[r] = -b[r];
    }
    if (!alignCholeskySolve(A, rhs, xi)) {
      lost = true;
      break;
    }
    alignApplyTwist(T, xi);
    res.iterations = it + 1;
    const double nw = std::sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]), nv = std::sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
    if (nw < o.eps_rot && nv < o.eps_trans) {
      res.converged = 1;
      break;
    }
  }
  std::memcpy(world_T_source_out, lost ? rq->world_T_source : T, sizeof(T));
  if (result) *result = res;
  if (lost) return fail(KHR_ENOTFOUND, "alignment lost after %d updates: %llu inliers (at least %d), or a singular system", res.iterations,
                        static_cast<unsigned long long>(res.n_inlier_last), o.min_inliers);
  return KHR_OK;
}

int khr_map_digest(khr_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(KHR_EINVAL, "null argument");
  unsigned long long* acc = c->d_digest;
  HIP_TRY(hipMemsetAsync(acc, 0, sizeof(unsigned long long) * kDigestWords, c->stream));
  hipLaunchKernelGGL(k_map_digest, dim3(2048), dim3(256), 0, c->stream, c->m, c->p, c->last_track_stamp, acc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, acc, sizeof(uint64_t) * kDigestWords, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

// ---- map checkpoints (khr_checkpoint_size / _save / _load / _inspect; device side: khr_kernels_checkpoint.h) -------------------
namespace {
constexpr size_t kCkptStageBytes = 32u << 20;   // one staging area; two of them are the whole device footprint of a checkpoint
constexpr uint32_t kCkptMaxChunkBlocks = 4096;  // (small blocks: bounds the chunk's slot list)
const char* const kCkptSectionNames[KHR_CKPT_SECTIONS] = {"indices", "distance", "weight", "color", "last_observed", "last_occupied",
                                                          "voxel_flags", "sem_label", "block_flags", "likelihoods"};

// bytes of one block in each section (0 = the configuration has no such layer)
struct CkptShape {
  size_t per[KHR_CKPT_SECTIONS];
  size_t per_block;
  CkptShape(int vps, int with_tracking, int with_semantics, int num_labels) {
    const size_t nv = static_cast<size_t>(vps) * vps * vps;
    per[KHR_CKPT_INDICES] = 12;
    per[KHR_CKPT_DISTANCE] = per[KHR_CKPT_WEIGHT] = per[KHR_CKPT_COLOR] = 4 * nv;
    per[KHR_CKPT_LAST_OBSERVED] = per[KHR_CKPT_LAST_OCCUPIED] = with_tracking ? 8 * nv : 0;
    per[KHR_CKPT_VOXEL_FLAGS] = nv;
    per[KHR_CKPT_SEM_LABEL] = with_semantics ? 4 * nv : 0;
    per[KHR_CKPT_BLOCK_FLAGS] = 1;
    per[KHR_CKPT_LIKELIHOODS] = with_semantics ? 4 * nv * static_cast<size_t>(num_labels) : 0;
    per_block = 0;
    for (size_t b : per) per_block += b;
  }
};

// section offsets and total length of a stream of n blocks
void ckptOffsets(const CkptShape& sh, uint64_t n, uint64_t* offset, uint64_t* total) {
  uint64_t at = KHR_CKPT_HEADER_BYTES;
  for (int s = 0; s < KHR_CKPT_SECTIONS; ++s) {
    offset[s] = sh.per[s] ? at : 0;
    at += (sh.per[s] * n + 63) / 64 * 64;
  }
  *total = at;
}

khr_checkpoint_header ckptHeaderFor(const khr_config& cfg, uint64_t n) {
  khr_checkpoint_header h{};
  h.magic = KHR_CKPT_MAGIC;
  h.version = KHR_CKPT_VERSION;
  h.voxel_size = cfg.voxel_size;
  h.voxels_per_side = cfg.voxels_per_side;
  h.truncation_distance = cfg.truncation_distance;
  h.with_semantics = cfg.with_semantics ? 1 : 0;
  h.with_tracking = cfg.with_tracking ? 1 : 0;
  h.num_labels = cfg.with_semantics ? cfg.num_labels : 0;
  h.semantic_mode = cfg.with_semantics ? cfg.semantic_mode : 0;
  h.header_bytes = KHR_CKPT_HEADER_BYTES;
  h.num_blocks = n;
  ckptOffsets(CkptShape(h.voxels_per_side, h.with_tracking, h.with_semantics, h.num_labels), n, h.offset, &h.total_bytes);
  return h;
}

// the regions of a staging area laid out for chunks of `cb` blocks
struct CkptStageLayout {
  size_t off[KHR_CKPT_SECTIONS], bytes;
  CkptStageLayout(const CkptShape& sh, size_t cb) {
    size_t at = 0;
    for (int s = 0; s < KHR_CKPT_SECTIONS; ++s) {
      off[s] = at;
      at += (sh.per[s] * cb + 255) / 256 * 256;
    }
    bytes = at;
  }
};
CkptStage ckptStageViews(const CkptShape& sh, const CkptStageLayout& L, uint8_t* d) {
  auto at = [&](int s) { return sh.per[s] ? d + L.off[s] : nullptr; };
  CkptStage o{};
  o.idx = reinterpret_cast<int32_t*>(at(KHR_CKPT_INDICES));
  o.dist = reinterpret_cast<float*>(at(KHR_CKPT_DISTANCE));
  o.weight = reinterpret_cast<float*>(at(KHR_CKPT_WEIGHT));
  o.color = reinterpret_cast<uint32_t*>(at(KHR_CKPT_COLOR));
  o.lobs = reinterpret_cast<uint64_t*>(at(KHR_CKPT_LAST_OBSERVED));
  o.locc = reinterpret_cast<uint64_t*>(at(KHR_CKPT_LAST_OCCUPIED));
  o.vfl = at(KHR_CKPT_VOXEL_FLAGS);
  o.label = reinterpret_cast<uint32_t*>(at(KHR_CKPT_SEM_LABEL));
  o.bfl = at(KHR_CKPT_BLOCK_FLAGS);
  o.lik = reinterpret_cast<float*>(at(KHR_CKPT_LIKELIHOODS));
  return o;
}

// blocks per chunk: what fits a staging area (at least one: a block larger than the area grows it)
uint32_t ckptChunkBlocks(const CkptShape& sh) {
  const size_t room = kCkptStageBytes - 256 * KHR_CKPT_SECTIONS;
  return static_cast<uint32_t>(std::min<size_t>(kCkptMaxChunkBlocks, std::max<size_t>(1, room / sh.per_block)));
}

int ckptEnsureStage(khr_ctx* c, const CkptShape& sh, uint32_t cb, bool bounce) {
  const size_t need = std::max(kCkptStageBytes, CkptStageLayout(sh, cb).bytes);
  if (c->d_ckpt[0].count() < need || c->d_ckpt[1].count() < need) {  // (both areas, and their mirrors, have one size)
    for (int i = 0; i < 2; ++i) c->d_ckpt[i].reset(), c->h_ckpt[i].reset();
    for (int i = 0; i < 2; ++i)
      if (c->d_ckpt[i].alloc(need)) return fail(KHR_ENOMEM, "checkpoint staging of %zu bytes", need);
  }
  for (int i = 0; i < 2 && bounce; ++i)
    if (!c->h_ckpt[i] && c->h_ckpt[i].alloc(c->d_ckpt[i].count()))
      return fail(KHR_ENOMEM, "page-locked checkpoint staging of %zu bytes", c->d_ckpt[i].count());
  for (int i = 0; i < 2; ++i)
    if (c->d_ckpt_slots[i].reserve(cb)) return fail(KHR_ENOMEM, "checkpoint slot list");
  if (!c->d_ckpt_err && c->d_ckpt_err.alloc(1)) return fail(KHR_ENOMEM, "checkpoint error word");
  for (int i = 0; i < 2; ++i) {
    KHR_TRY(c->ev_ckpt_filled[i].ensure());
    KHR_TRY(c->ev_ckpt_drained[i].ensure());
  }
  if (!c->copy_stream) KHR_TRY(createStream(c, c->copy_stream));
  return KHR_OK;
}

// back to the empty map on the device and in the host mirrors (the failure exit of a load, and its first step)
int ckptClearMap(khr_ctx* c) {
  const size_t n = std::max<size_t>(static_cast<size_t>(c->m.ht_mask) + 1, c->m.capacity);
  hipLaunchKernelGGL(k_reset_map, dim3(gridFor(n)), dim3(256), 0, c->stream, c->m, c->d_wg_stats);
  HIP_TRY(hipGetLastError());
  c->mesh_cur = 0;
  c->mesh_total = 0;
  c->mesh_stale = false;
  c->mesh_made = false;
  c->host_index_valid = false, ++c->map_gen;
  c->explicit_blocks = 0;
  c->box_listed = false;
  c->last_removed = 0;
  c->removed_pending = false;
  c->last_track_stamp = 0;
  return KHR_OK;
}
}  // namespace

int khr_checkpoint_inspect(const void* buffer, uint64_t n_bytes, khr_checkpoint_header* out) {
  if (!buffer || !out) return fail(KHR_EINVAL, "null argument");
  if (n_bytes < KHR_CKPT_HEADER_BYTES)
    return fail(KHR_EINVAL, "checkpoint: truncated buffer (%llu bytes, the header alone has %d)", static_cast<unsigned long long>(n_bytes), KHR_CKPT_HEADER_BYTES);
  khr_checkpoint_header h;
  std::memcpy(&h, buffer, sizeof(h));
  if (h.magic != KHR_CKPT_MAGIC) return fail(KHR_EINVAL, "checkpoint: bad magic 0x%08x (expected 0x%08x)", h.magic, KHR_CKPT_MAGIC);
  if (h.version != KHR_CKPT_VERSION) return fail(KHR_EINVAL, "checkpoint: unknown format version %u (this library reads version %u)", h.version, KHR_CKPT_VERSION);
  if (h.header_bytes != KHR_CKPT_HEADER_BYTES) return fail(KHR_EINVAL, "checkpoint: header_bytes %u, expected %d", h.header_bytes, KHR_CKPT_HEADER_BYTES);
  if (h.voxels_per_side != 8 && h.voxels_per_side != 16) return fail(KHR_EINVAL, "checkpoint: voxels_per_side %d (must be 8 or 16)", h.voxels_per_side);
  if (!(h.voxel_size > 0.f) || !(h.truncation_distance > 0.f)) return fail(KHR_EINVAL, "checkpoint: voxel_size / truncation_distance must be > 0");
  if ((h.with_semantics | 1) != 1 || (h.with_tracking | 1) != 1) return fail(KHR_EINVAL, "checkpoint: with_semantics / with_tracking must be 0 or 1");
  if (h.with_semantics ? (h.num_labels < 1 || h.num_labels > 65536) : (h.num_labels != 0 || h.semantic_mode != 0))
    return fail(KHR_EINVAL, "checkpoint: num_labels %d / semantic_mode %d do not fit with_semantics %d", h.num_labels, h.semantic_mode, h.with_semantics);
  if (h.num_blocks > (1ull << 32)) return fail(KHR_EINVAL, "checkpoint: block count %llu", static_cast<unsigned long long>(h.num_blocks));
  uint64_t off[KHR_CKPT_SECTIONS], total = 0;
  ckptOffsets(CkptShape(h.voxels_per_side, h.with_tracking, h.with_semantics, h.num_labels), h.num_blocks, off, &total);
  for (int s = 0; s < KHR_CKPT_SECTIONS; ++s)
    if (h.offset[s] != off[s])
      return fail(KHR_EINVAL, "checkpoint: section %s at offset %llu, expected %llu", kCkptSectionNames[s], static_cast<unsigned long long>(h.offset[s]),
                  static_cast<unsigned long long>(off[s]));
  if (h.total_bytes != total) return fail(KHR_EINVAL, "checkpoint: total_bytes %llu, expected %llu", static_cast<unsigned long long>(h.total_bytes), static_cast<unsigned long long>(total));
  if (n_bytes < total)
    return fail(KHR_EINVAL, "checkpoint: truncated buffer (%llu bytes, the header claims %llu)", static_cast<unsigned long long>(n_bytes), static_cast<unsigned long long>(total));
  *out = h;
  return KHR_OK;
}

int khr_checkpoint_size(khr_ctx* c, uint64_t* n_bytes, int64_t* n_blocks) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  const int rc = ensureHostIndex(c);
  if (rc) return rc;
  const khr_checkpoint_header h = ckptHeaderFor(c->cfg, c->host_index.size());
  if (n_bytes) *n_bytes = h.total_bytes;
  if (n_blocks) *n_blocks = static_cast<int64_t>(h.num_blocks);
  return KHR_OK;
}

int khr_checkpoint_save(khr_ctx* c, void* buffer, uint64_t cap_bytes, uint64_t* n_bytes) {
  if (!c || (!buffer && cap_bytes)) return fail(KHR_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensureSortKeys(c);
  if (rc) return rc;
  // select -> sort on the device; the count comes back with the one host wait in front of the transfer
  HIP_TRY(hipMemsetAsync(c->d_slice_count, 0, sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(k_ckpt_select, dim3(std::min(gridFor(c->m.capacity), 1024)), dim3(256), 0, c->stream, c->m, c->d_slice_count, c->d_slice_keys);
  HIP_TRY(hipGetLastError());
  if ((rc = sortKeys(c))) return rc;
  uint32_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, c->d_slice_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const khr_checkpoint_header h = ckptHeaderFor(c->cfg, n);
  if (n_bytes) *n_bytes = h.total_bytes;
  if (h.total_bytes > cap_bytes)
    return fail(KHR_ENOMEM, "checkpoint: the stream of %u blocks has %llu bytes, the buffer %llu", n, static_cast<unsigned long long>(h.total_bytes),
                static_cast<unsigned long long>(cap_bytes));
  const CkptShape sh(h.voxels_per_side, h.with_tracking, h.with_semantics, h.num_labels);
  const uint32_t cb = ckptChunkBlocks(sh);
  const bool bounce = !pointerIs(buffer, 0);
  if ((rc = ckptEnsureStage(c, sh, cb, bounce))) return rc;
  const CkptStageLayout L(sh, cb);
  uint8_t* const dst = static_cast<uint8_t*>(buffer);
  // header, and zeros in the alignment gaps behind the sections (the stream is a function of the map alone)
  std::memset(dst, 0, KHR_CKPT_HEADER_BYTES);
  std::memcpy(dst, &h, sizeof(h));
  for (int s = 0; s < KHR_CKPT_SECTIONS; ++s)
    if (sh.per[s]) {
      const uint64_t end = h.offset[s] + sh.per[s] * n, pad = (64 - end % 64) % 64;
      std::memset(dst + end, 0, pad);
    }
  const uint32_t n_chunks = (n + cb - 1) / cb;
  auto drain = [&](uint32_t chunk) {  // (pageable buffers) the chunk's sections out of the page-locked mirror
    const uint32_t b0 = chunk * cb, nb = std::min(cb, n - b0);
    for (int s = 0; s < KHR_CKPT_SECTIONS; ++s)
      if (sh.per[s]) std::memcpy(dst + h.offset[s] + sh.per[s] * b0, c->h_ckpt[chunk & 1] + L.off[s], sh.per[s] * nb);
  };
  for (uint32_t i = 0; i < n_chunks; ++i) {
    const int buf = i & 1;
    const uint32_t b0 = i * cb, nb = std::min(cb, n - b0);
    if (i >= 2) {  // the staging area is free once the copy of chunk i - 2 has left it
      if (bounce) {
        HIP_TRY(hipEventSynchronize(c->ev_ckpt_drained[buf]));
        drain(i - 2);
      }
      HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_ckpt_drained[buf], 0));
    }
    rc = dispatchVps(c, [&](auto vps) {
      hipLaunchKernelGGL((k_ckpt_pack<decltype(vps)::value>), dim3(nb), dim3(256), 0, c->stream, c->m, c->p, c->d_slice_keys, c->d_slice_count, b0,
                         nb, ckptStageViews(sh, L, c->d_ckpt[buf]), c->last_track_stamp);
      HIP_TRY(hipGetLastError());
      return KHR_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev_ckpt_filled[buf], c->stream));
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->ev_ckpt_filled[buf], 0));
    for (int s = 0; s < KHR_CKPT_SECTIONS; ++s)
      if (sh.per[s]) {
        uint8_t* const to = bounce ? c->h_ckpt[buf] + L.off[s] : dst + h.offset[s] + sh.per[s] * b0;
        HIP_TRY(hipMemcpyAsync(to, c->d_ckpt[buf] + L.off[s], sh.per[s] * nb, hipMemcpyDeviceToHost, c->copy_stream));
      }
    HIP_TRY(hipEventRecord(c->ev_ckpt_drained[buf], c->copy_stream));
  }
  HIP_TRY(hipStreamSynchronize(c->copy_stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (bounce)
    for (uint32_t i = n_chunks >= 2 ? n_chunks - 2 : 0; i < n_chunks; ++i) drain(i);
  return KHR_OK;
}

int khr_checkpoint_load(khr_ctx* c, const void* buffer, uint64_t n_bytes, int64_t* n_kept) {
  if (!c || !buffer) return fail(KHR_EINVAL, "null argument");
  if (n_kept) *n_kept = 0;
  c->weld_valid = false;  // (khr_weld_mesh: the welded mesh belongs to the map before the load)
  c->diff_valid = false;  // (khr_diff_map: so does the diff)
  c->seg_valid = false;   // (khr_segment_map: and the segmentation)
  c->vor.valid = false;   // (khr_voronoi_field: and the Voronoi field)
  c->pl.valid = false;    // (khr_places_graph: and the places graph)
  c->tf.valid = c->tfp_valid = false;  // (khr_travel_field: and the travel field with its paths)
  khr_checkpoint_header h;
  int rc = khr_checkpoint_inspect(buffer, n_bytes, &h);
  if (rc) return rc;
  const khr_checkpoint_header mine = ckptHeaderFor(c->cfg, 0);
#define KHR_CKPT_FIELD(name, fmt, cast)                                                                                        \
  if (h.name != mine.name)                                                                                                     \
    return fail(KHR_EINVAL, "checkpoint: " #name " is " fmt " in the stream and " fmt " in this context", static_cast<cast>(h.name), \
                static_cast<cast>(mine.name));
  KHR_CKPT_FIELD(voxel_size, "%.9g", double)
  KHR_CKPT_FIELD(voxels_per_side, "%d", int)
  KHR_CKPT_FIELD(truncation_distance, "%.9g", double)
  KHR_CKPT_FIELD(with_semantics, "%d", int)
  KHR_CKPT_FIELD(with_tracking, "%d", int)
  KHR_CKPT_FIELD(num_labels, "%d", int)
  KHR_CKPT_FIELD(semantic_mode, "%d", int)
#undef KHR_CKPT_FIELD
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ensureHostIndex(c))) return rc;
  if (!c->host_index.empty()) return fail(KHR_ESTATE, "checkpoint: the map holds %zu blocks; a load needs an empty map (khr_reset_map)", c->host_index.size());
  const uint8_t* const src = static_cast<const uint8_t*>(buffer);
  const uint32_t n = static_cast<uint32_t>(h.num_blocks);
  // blocks this rank keeps, counted on the host: a stream that cannot fit is refused before the map is touched
  uint64_t kept = 0;
  {
    const int32_t* idx = reinterpret_cast<const int32_t*>(src + h.offset[KHR_CKPT_INDICES]);
    for (uint32_t b = 0; b < n; ++b) {
      int32_t v[3];
      std::memcpy(v, idx + 3 * static_cast<size_t>(b), sizeof(v));
      for (int a = 0; a < 3; ++a)
        if (v[a] < -(1 << 20) || v[a] >= (1 << 20)) return fail(KHR_EINVAL, "checkpoint: block %u has index (%d, %d, %d), out of range", b, v[0], v[1], v[2]);
      kept += ownerOf(v[0], v[1], v[2], c->p.world) == c->p.rank ? 1 : 0;
    }
  }
  if (kept > c->m.capacity)
    return fail(KHR_ENOMEM, "checkpoint: %llu blocks to keep, max_blocks is %u", static_cast<unsigned long long>(kept), c->m.capacity);
  const CkptShape sh(h.voxels_per_side, h.with_tracking, h.with_semantics, h.num_labels);
  const uint32_t cb = ckptChunkBlocks(sh);
  const bool bounce = !pointerIs(buffer, 0);
  if ((rc = ckptEnsureStage(c, sh, cb, bounce))) return rc;
  const CkptStageLayout L(sh, cb);
  // canonical empty state first (an emptied map may have any free list), then chunk by chunk: copy, insert, scatter
  if ((rc = ckptClearMap(c))) return rc;
  HIP_TRY(hipMemsetAsync(c->d_ckpt_err, 0, sizeof(uint32_t), c->stream));
  const uint32_t n_chunks = (n + cb - 1) / cb;
  for (uint32_t i = 0; i < n_chunks; ++i) {
    const int buf = i & 1;
    const uint32_t b0 = i * cb, nb = std::min(cb, n - b0);
    if (i >= 2) {
      if (bounce) HIP_TRY(hipEventSynchronize(c->ev_ckpt_filled[buf]));               // the mirror's chunk i - 2 has been copied
      HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->ev_ckpt_drained[buf], 0));        // the kernels of chunk i - 2 have read the staging
    }
    for (int s = 0; s < KHR_CKPT_SECTIONS; ++s)
      if (sh.per[s]) {
        const uint8_t* from = src + h.offset[s] + sh.per[s] * b0;
        if (bounce) {
          std::memcpy(c->h_ckpt[buf] + L.off[s], from, sh.per[s] * nb);
          from = c->h_ckpt[buf] + L.off[s];
        }
        HIP_TRY(hipMemcpyAsync(c->d_ckpt[buf] + L.off[s], from, sh.per[s] * nb, hipMemcpyHostToDevice, c->copy_stream));
      }
    HIP_TRY(hipEventRecord(c->ev_ckpt_filled[buf], c->copy_stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_ckpt_filled[buf], 0));
    const CkptStage in = ckptStageViews(sh, L, c->d_ckpt[buf]);
    hipLaunchKernelGGL(k_ckpt_insert, dim3(gridFor(nb)), dim3(256), 0, c->stream, c->m, c->p, in.idx, in.bfl, nb, c->d_ckpt_slots[buf], c->d_ckpt_err);
    HIP_TRY(hipGetLastError());
    rc = dispatchVps(c, [&](auto vps) {
      hipLaunchKernelGGL((k_ckpt_unpack<decltype(vps)::value>), dim3(nb), dim3(256), 0, c->stream, c->m, c->p, c->d_ckpt_slots[buf], nb, in);
      HIP_TRY(hipGetLastError());
      return KHR_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev_ckpt_drained[buf], c->stream));
  }
  rc = dispatchVps(c, [&](auto vps) {
    hipLaunchKernelGGL((k_ckpt_rebuild<decltype(vps)::value>), dim3(std::max(1u, std::min(c->m.capacity, 4096u))), dim3(256), 0, c->stream, c->m, c->p, c->wpb);
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
  if (rc) return rc;
  uint32_t err = 0, live = 0;
  HIP_TRY(hipMemcpyAsync(&err, c->d_ckpt_err, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&live, &c->m.counters[C_N_LIVE], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->copy_stream));
  if (err || live != kept) {
    if ((rc = ckptClearMap(c))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (err & kCkptErrDuplicate) return fail(KHR_EINVAL, "checkpoint: duplicate block index in the stream (met its twin at the hash insert)");
    if (err & kCkptErrIndex) return fail(KHR_EINVAL, "checkpoint: block index out of range");
    if (err & kCkptErrPool) return fail(KHR_ENOMEM, "checkpoint: the block pool (max_blocks %u) ran out during the load", c->m.capacity);
    return fail(KHR_EDEVICE, "checkpoint: %u blocks restored, %llu expected", live, static_cast<unsigned long long>(kept));
  }
  c->host_index_valid = false, ++c->map_gen;
  c->stats = khr_stats{};
  if (n_kept) *n_kept = static_cast<int64_t>(kept);
  return KHR_OK;
}

static int refreshMeshTotals(khr_ctx* c) {
  if (!c->mesh_stale) return KHR_OK;
  // one round trip through a pinned block of its own: mesh total, work count and the counter block (C_MESH_OVERFLOW,
  // C_MAX_SLOT).  NOT the mesh staging block: a gather queued by khr_fetch_mesh_launch may be writing there, and its ticket
  // is header word 15 -- exactly where counter 13 of this copy used to land ("mesh gather was never published" whenever
  // statistics were read between the launch and the fetch: bench.py --output-copy host beyond ~30 steps)
  if (!c->h_totals && c->h_totals.alloc(C_COUNT + 2)) return fail(KHR_ENOMEM, "pinned block for the mesh totals");
  uint32_t* hs = c->h_totals;
  HIP_TRY(hipMemcpyAsync(hs, c->d_mesh_offset + c->m.capacity, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hs + 1, c->d_mesh_nwork + c->mesh_nwork_last, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hs + 2, c->m.counters, sizeof(uint32_t) * C_COUNT, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const uint32_t total = hs[0], nwork = hs[1];
  c->h_counters.assign(hs + 2, hs + 2 + C_COUNT);
  c->counters_gen = c->map_gen;
  const uint32_t ovf = c->h_counters[C_MESH_OVERFLOW];
  if (ovf) return fail(KHR_ENOMEM, "mesh needs %u vertices, max_mesh_vertices=%llu", total,
                       static_cast<unsigned long long>(c->cfg.max_mesh_vertices));
  c->mesh_total = total;
  c->stats.n_mesh_blocks = nwork;
  c->stats.n_mesh_vertices = total;
  c->mesh_stale = false;
  return KHR_OK;
}

int64_t khr_download_updated(khr_ctx* c, int32_t* indices, float* distance, float* weight, uint8_t* color_rgba,
                             uint64_t* last_observed, uint8_t* voxel_flags, uint32_t* sem_label, int64_t cap_blocks) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  int rc = ensureHostIndex(c);
  if (rc) return rc;
  // updated blocks in sorted index order (std::map iteration)
  std::vector<uint32_t> slots;
  std::vector<int32_t> idx;
  for (auto& kv : c->host_index)
    if (c->host_flags[kv.second] & BLK_UPDATED) {
      slots.push_back(kv.second);
      idx.insert(idx.end(), kv.first.begin(), kv.first.end());
    }
  const int64_t n = static_cast<int64_t>(slots.size());
  if (n > cap_blocks) return fail(KHR_EINVAL, "%lld updated blocks, cap %lld", static_cast<long long>(n), static_cast<long long>(cap_blocks));
  if (n == 0) return 0;
  if (indices) std::memcpy(indices, idx.data(), sizeof(int32_t) * idx.size());
  const size_t nv = c->p.nvox, tot = static_cast<size_t>(n) * nv;
  const bool trk = c->cfg.with_tracking, sem = c->cfg.with_semantics;
  // staging: one allocation, carved per field
  const size_t bytes = tot * ((distance ? 4 : 0) + (weight ? 4 : 0) + (color_rgba ? 4 : 0) + ((last_observed && trk) ? 8 : 0) +
                              (voxel_flags ? 1 : 0) + ((sem_label && sem) ? 4 : 0)) + sizeof(uint32_t) * n + 256;
  DevTemp stage;  // (freed on every way out of this call)
  KHR_TRY(stage.alloc(bytes));
  uint8_t* cur = stage;
  auto carve = [&](size_t b) { uint8_t* p = cur; cur += (b + 15) / 16 * 16; return p; };
  PackOut o{};
  if (last_observed && trk) o.last_obs = reinterpret_cast<uint64_t*>(carve(tot * 8));
  if (distance) o.dist = reinterpret_cast<float*>(carve(tot * 4));
  if (weight) o.weight = reinterpret_cast<float*>(carve(tot * 4));
  if (color_rgba) o.color = reinterpret_cast<uint32_t*>(carve(tot * 4));
  if (sem_label && sem) o.sem_label = reinterpret_cast<uint32_t*>(carve(tot * 4));
  if (voxel_flags) o.vflags = carve(tot);
  uint32_t* d_slots = reinterpret_cast<uint32_t*>(carve(sizeof(uint32_t) * n));
  hipError_t e = hipMemcpyAsync(d_slots, slots.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rc = dispatchVps(c, [&](auto vps) {
      hipLaunchKernelGGL((k_pack_blocks<decltype(vps)::value>), dim3(static_cast<unsigned>(std::min<int64_t>(n, 4096))), dim3(256), 0,
                         c->stream, c->m, d_slots, static_cast<int>(n), o);
      return KHR_OK;
    });
    auto D = [&](void* dst, const void* src, size_t b) { if (e == hipSuccess && dst && src) e = hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, c->stream); };
    D(distance, o.dist, tot * 4);
    D(weight, o.weight, tot * 4);
    D(color_rgba, o.color, tot * 4);
    D(last_observed, o.last_obs, tot * 8);
    D(voxel_flags, o.vflags, tot);
    D(sem_label, o.sem_label, tot * 4);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e != hipSuccess) return fail(KHR_EDEVICE, "download_updated failed: %s", hipGetErrorString(e));
  if (rc) return rc;
  if (last_observed && !trk) std::memset(last_observed, 0, tot * 8);
  if (sem_label && !sem) std::memset(sem_label, 0, tot * 4);
  return n;
}

// ---- snapshot of the updated blocks (VolumetricMap::cloneUpdated, active_window.cpp:229) --------------------------------
struct khr_snapshot {
  khr_ctx* ctx = nullptr;  // valid while !pool->dead
  std::shared_ptr<khr_ctx::SnapPool> pool;
  int device = 0;
  khr_ctx::SnapArena arena;
  uint32_t fields = 0, cap = 0, nvox = 0, ticket = 0;
  // carved from the arena
  uint32_t* d_count = nullptr;
  uint32_t* d_slots = nullptr;
  int4* d_index = nullptr;
  PackOut o{};
  int64_t n = -1;        // blocks copied (known after the first wait)
  int64_t total = -1;    // updated blocks found (> cap: overflow)
  Event ev_packed;  // recorded on the context's stream behind the pack kernel
  Event ev_copied;  // khr_snapshot_download_begin: the last device -> host copy on the copy stream
  bool copying = false;
  int32_t* d_index3 = nullptr;  // carved from the arena: the block indices as (x, y, z) triples (khr_snapshot_download_begin)
};

static size_t snapBytes(uint32_t fields, size_t cap, size_t nvox, bool trk, bool sem, size_t K) {
  auto al = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t b = 256 + al(cap * 4) + al(cap * 16) + al(cap * 12);
  if (fields & KHR_SNAP_DISTANCE) b += al(cap * nvox * 4);
  if (fields & KHR_SNAP_WEIGHT) b += al(cap * nvox * 4);
  if (fields & KHR_SNAP_COLOR) b += al(cap * nvox * 4);
  if ((fields & KHR_SNAP_LAST_OBSERVED) && trk) b += al(cap * nvox * 8);
  if (fields & KHR_SNAP_FLAGS) b += al(cap * nvox);
  if ((fields & KHR_SNAP_LABEL) && sem) b += al(cap * nvox * 4);
  if ((fields & KHR_SNAP_LAST_OCCUPIED) && trk) b += al(cap * nvox * 8);
  if ((fields & KHR_SNAP_LIKELIHOODS) && sem) b += al(cap * nvox * 4 * K);
  return b;
}

// Arenas are allocated when a snapshot finds none free -- a hipMalloc of up to a gigabyte, i.e. tens of milliseconds in which the
// device does nothing else.  A consumer that knows how many outputs it keeps in flight allocates them up front.
int khr_reserve_snapshots(khr_ctx* c, uint32_t fields, int64_t cap_blocks, int n_arenas) {
  if (!c || !(fields & KHR_SNAP_EVERYTHING) || n_arenas < 0 || n_arenas > 16) return fail(KHR_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  const size_t cap = cap_blocks > 0 ? static_cast<size_t>(std::min<int64_t>(cap_blocks, c->m.capacity)) : c->m.capacity;
  const size_t need = snapBytes(fields, cap, c->p.nvox, c->cfg.with_tracking, c->cfg.with_semantics, static_cast<size_t>(c->p.K));
  size_t have = 0;
  {
    std::lock_guard<std::mutex> lock(c->snap_pool->mu);
    for (const auto& a : c->snap_pool->free) have += a.buf.count() >= need ? 1 : 0;
  }
  for (size_t i = have; i < static_cast<size_t>(n_arenas); ++i) {
    khr_ctx::SnapArena a;
    KHR_TRY(a.alloc(need));
    std::lock_guard<std::mutex> lock(c->snap_pool->mu);
    c->snap_pool->free.push_back(std::move(a));
  }
  return KHR_OK;
}

// the snapshot's kernels on stream `st`: the context's (khr_snapshot_updated), or khr_process_frame's snapshot stream
static int snapshotUpdated(khr_ctx* c, hipStream_t st, uint32_t fields, int64_t cap_blocks, khr_snapshot** out) {
  if (!out || !(fields & KHR_SNAP_EVERYTHING)) return fail(KHR_EINVAL, "bad argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(c->device));
  const bool trk = c->cfg.with_tracking, sem = c->cfg.with_semantics;
  const size_t cap = cap_blocks > 0 ? static_cast<size_t>(std::min<int64_t>(cap_blocks, c->m.capacity)) : c->m.capacity;
  const size_t nvox = c->p.nvox;
  const size_t need = snapBytes(fields, cap, nvox, trk, sem, static_cast<size_t>(c->p.K));
  auto snap = std::make_unique<khr_snapshot>();
  {
    auto& fr = c->snap_pool->free;
    std::lock_guard<std::mutex> lock(c->snap_pool->mu);
    size_t best = fr.size();
    for (size_t i = 0; i < fr.size(); ++i)
      if (fr[i].buf.count() >= need && (best == fr.size() || fr[i].buf.count() < fr[best].buf.count())) best = i;
    if (best < fr.size()) {
      snap->arena = std::move(fr[best]);
      fr.erase(fr.begin() + static_cast<long>(best));
    }
  }
  // first snapshots of a run: a device allocation (stalls the device once per arena; released arenas are reused)
  if (!snap->arena.buf) KHR_TRY(snap->arena.alloc(need));
  snap->ctx = c;
  snap->pool = c->snap_pool;
  snap->device = c->device;
  snap->fields = fields;
  snap->cap = static_cast<uint32_t>(cap);
  snap->nvox = static_cast<uint32_t>(nvox);
  snap->ticket = ++c->snap_ticket;
  if (snap->ticket == 0) snap->ticket = ++c->snap_ticket;
  uint8_t* cur = snap->arena.buf;
  auto carve = [&](size_t b) { uint8_t* p = cur; cur += (b + 255) / 256 * 256; return p; };
  snap->d_count = reinterpret_cast<uint32_t*>(carve(256));
  snap->d_slots = reinterpret_cast<uint32_t*>(carve(cap * 4));
  snap->d_index = reinterpret_cast<int4*>(carve(cap * 16));
  snap->d_index3 = reinterpret_cast<int32_t*>(carve(cap * 12));
  if (fields & KHR_SNAP_DISTANCE) snap->o.dist = reinterpret_cast<float*>(carve(cap * nvox * 4));
  if (fields & KHR_SNAP_WEIGHT) snap->o.weight = reinterpret_cast<float*>(carve(cap * nvox * 4));
  if (fields & KHR_SNAP_COLOR) snap->o.color = reinterpret_cast<uint32_t*>(carve(cap * nvox * 4));
  if ((fields & KHR_SNAP_LAST_OBSERVED) && trk) snap->o.last_obs = reinterpret_cast<uint64_t*>(carve(cap * nvox * 8));
  if (fields & KHR_SNAP_FLAGS) snap->o.vflags = carve(cap * nvox);
  if ((fields & KHR_SNAP_LABEL) && sem) snap->o.sem_label = reinterpret_cast<uint32_t*>(carve(cap * nvox * 4));
  if ((fields & KHR_SNAP_LAST_OCCUPIED) && trk) snap->o.last_occ = reinterpret_cast<uint64_t*>(carve(cap * nvox * 8));
  if ((fields & KHR_SNAP_LIKELIHOODS) && sem) snap->o.lik = reinterpret_cast<float*>(carve(cap * nvox * 4 * static_cast<size_t>(c->p.K)));
  snap->o.K = c->p.K;
  snap->o.KS = c->p.KS;
  snap->o.track_stamp = c->last_track_stamp;
  hipError_t e = hipMemsetAsync(snap->d_count, 0, 4, st);
  int rc_ev = KHR_OK;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_snapshot_select, dim3(gridFor(c->m.capacity)), dim3(256), 0, st, c->m, snap->d_count, snap->d_slots,
                       snap->d_index, snap->cap);
    dispatchVps(c, [&](auto vps) {
      KHR_LAUNCH_TIMED_ON(12, st, (k_snapshot_pack<decltype(vps)::value>), dim3(2048), dim3(256), c->m, snap->d_count, snap->d_slots,
                          snap->cap, snap->o, snap->arena.count.dev(), snap->ticket);
      return KHR_OK;
    });
    e = hipGetLastError();
    // consumers on other streams (khr_snapshot_download_begin's copy stream) order themselves behind the pack kernel with this
    if (e == hipSuccess) rc_ev = snap->ev_packed.ensure();
    if (e == hipSuccess && rc_ev == KHR_OK) e = hipEventRecord(snap->ev_packed, st);
  }
  if (e != hipSuccess || rc_ev != KHR_OK) {
    std::lock_guard<std::mutex> lock(c->snap_pool->mu);
    c->snap_pool->free.push_back(std::move(snap->arena));
    return rc_ev != KHR_OK ? rc_ev : fail(KHR_EDEVICE, "snapshot launch failed: %s", hipGetErrorString(e));
  }
  *out = snap.release();
  return KHR_OK;
}

int khr_snapshot_updated(khr_ctx* c, uint32_t fields, int64_t cap_blocks, khr_snapshot** out) {
  if (!c) return fail(KHR_EINVAL, "bad argument");
  return snapshotUpdated(c, c->stream, fields, cap_blocks, out);
}

int khr_take_snapshot(khr_ctx* c, khr_snapshot** out) {
  if (!c || !out) return fail(KHR_EINVAL, "null argument");
  *out = c->pending_snapshot;
  c->pending_snapshot = nullptr;
  return *out ? KHR_OK : KHR_ENOTFOUND;
}

static int snapshotWait(khr_snapshot* s) {
  if (s->n >= 0) return KHR_OK;
  // the pack kernel's first thread publishes {count, ticket}; the host spins on the ticket (a blocking stream wait costs
  // hundreds of us of wake-up latency; the kernel is at most one output stage away)
  const auto t0 = std::chrono::steady_clock::now();
  while (s->arena.h_count()[1] != s->ticket) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) return fail(KHR_EDEVICE, "snapshot was never produced (stream stuck?)");
    std::this_thread::yield();
  }
  s->total = s->arena.h_count()[0];
  s->n = std::min<int64_t>(s->total, s->cap);
  return KHR_OK;
}

// non-blocking: 1 once the snapshot's block count is known (its pack kernel has started), 0 before
int khr_snapshot_poll(khr_snapshot* s) {
  if (!s) return fail(KHR_EINVAL, "null snapshot");
  return (s->n >= 0 || s->arena.h_count()[1] == s->ticket) ? 1 : 0;
}

int64_t khr_snapshot_num_blocks(khr_snapshot* s) {
  if (!s) return fail(KHR_EINVAL, "null snapshot");
  const int rc = snapshotWait(s);
  return rc ? rc : s->total;
}

static int64_t snapshotDownload(khr_snapshot* s, int32_t* indices, float* distance, float* weight, uint8_t* color_rgba,
                                uint64_t* last_observed, uint8_t* voxel_flags, uint32_t* sem_label, uint64_t* last_occupied,
                                float* likelihoods, int64_t cap_blocks) {
  if (!s) return fail(KHR_EINVAL, "null snapshot");
  int rc = snapshotWait(s);
  if (rc) return rc;
  if (s->total > s->cap) return fail(KHR_ENOMEM, "%lld updated blocks, snapshot capacity %u", static_cast<long long>(s->total), s->cap);
  const int64_t n = s->n;
  if (n > cap_blocks) return fail(KHR_EINVAL, "%lld blocks in the snapshot, cap %lld", static_cast<long long>(n), static_cast<long long>(cap_blocks));
  if (n == 0) return 0;
  {
    std::lock_guard<std::mutex> lock(s->pool->mu);
    if (s->pool->dead) return fail(KHR_ESTATE, "the snapshot's context has been destroyed");
  }
  khr_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  // the copy kernel itself must have finished, not only published its count (the event sits right behind it: later frames
  // queued on the stream are not waited for)
  if (s->copying) return fail(KHR_ESTATE, "an asynchronous download of this snapshot is in flight (khr_snapshot_download_end first)");
  HIP_TRY(hipEventSynchronize(s->ev_packed));
  const size_t nv = s->nvox;
  // blocks come in the snapshot's own order (the order the device found them in); `indices` says which is which.  Each
  // field is ONE device -> host copy straight into the caller's array (pinned caller memory gets the full link rate).
  if (indices) {
    std::vector<int4> idx(static_cast<size_t>(n));
    HIP_TRY(hipMemcpy(idx.data(), s->d_index, sizeof(int4) * n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
      indices[3 * i] = idx[i].x;
      indices[3 * i + 1] = idx[i].y;
      indices[3 * i + 2] = idx[i].z;
    }
  }
  hipError_t e = hipSuccess;
  auto field = [&](void* dst, const void* src, size_t elem) {
    if (e == hipSuccess && dst && src) e = hipMemcpyAsync(dst, src, static_cast<size_t>(n) * nv * elem, hipMemcpyDeviceToHost, c->stream);
  };
  field(distance, s->o.dist, 4);
  field(weight, s->o.weight, 4);
  field(color_rgba, s->o.color, 4);
  field(last_observed, s->o.last_obs, 8);
  field(voxel_flags, s->o.vflags, 1);
  field(sem_label, s->o.sem_label, 4);
  field(last_occupied, s->o.last_occ, 8);
  field(likelihoods, s->o.lik, 4 * static_cast<size_t>(s->o.K));
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(KHR_EDEVICE, "snapshot download failed: %s", hipGetErrorString(e));
  return n;
}

int64_t khr_snapshot_download(khr_snapshot* s, int32_t* indices, float* distance, float* weight, uint8_t* color_rgba,
                              uint64_t* last_observed, uint8_t* voxel_flags, uint32_t* sem_label, int64_t cap_blocks) {
  return snapshotDownload(s, indices, distance, weight, color_rgba, last_observed, voxel_flags, sem_label, nullptr, nullptr, cap_blocks);
}

int64_t khr_snapshot_download_extra(khr_snapshot* s, int32_t* indices, uint64_t* last_occupied, float* likelihoods, int64_t cap_blocks) {
  return snapshotDownload(s, indices, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, last_occupied, likelihoods, cap_blocks);
}

// Asynchronous form of khr_snapshot_download for a consumer that overlaps the transfer with the next frames: the copies go to a
// copy stream of the context, ordered behind the snapshot's pack kernel by an event -- the context's own stream is neither
// waited for nor delayed.  Non-NULL pointers select the fields (the consumer's field mask); pinned destinations get the
// full link rate.  _end waits for the copies and returns the block count.
int khr_snapshot_download_begin(khr_snapshot* s, int32_t* indices, float* distance, float* weight, uint8_t* color_rgba,
                                uint64_t* last_observed, uint8_t* voxel_flags, uint32_t* sem_label, int64_t cap_blocks) {
  if (!s) return fail(KHR_EINVAL, "null snapshot");
  if (s->copying) return fail(KHR_ESTATE, "a download of this snapshot is already in flight");
  HT("dl_begin_enter");
  int rc = snapshotWait(s);  // (the count: published by the pack kernel's first thread)
  if (rc) return rc;
  if (s->total > s->cap) return fail(KHR_ENOMEM, "%lld updated blocks, snapshot capacity %u", static_cast<long long>(s->total), s->cap);
  const int64_t n = s->n;
  if (n > cap_blocks) return fail(KHR_EINVAL, "%lld blocks in the snapshot, cap %lld", static_cast<long long>(n), static_cast<long long>(cap_blocks));
  {
    std::lock_guard<std::mutex> lock(s->pool->mu);
    if (s->pool->dead) return fail(KHR_ESTATE, "the snapshot's context has been destroyed");
  }
  khr_ctx* c = s->ctx;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->copy_stream) KHR_TRY(createStream(c, c->copy_stream));
  KHR_TRY(s->ev_copied.ensure());
  HIP_TRY(hipStreamWaitEvent(c->copy_stream, s->ev_packed, 0));
  const size_t nv = s->nvox;
  if (n > 0) {
    if (indices) {  // (x, y, z) triples made on the device, then one copy straight into the caller's (pinned) array
      hipLaunchKernelGGL(k_snapshot_index3, dim3(gridFor(static_cast<size_t>(n))), dim3(256), 0, c->copy_stream, s->d_index, s->d_index3,
                         static_cast<uint32_t>(n));
      HIP_TRY(hipMemcpyAsync(indices, s->d_index3, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost, c->copy_stream));
    }
    hipError_t e = hipSuccess;
    auto field = [&](void* dst, const void* src, size_t elem) {
      if (e == hipSuccess && dst && src) e = hipMemcpyAsync(dst, src, static_cast<size_t>(n) * nv * elem, hipMemcpyDeviceToHost, c->copy_stream);
    };
    field(distance, s->o.dist, 4);
    field(weight, s->o.weight, 4);
    field(color_rgba, s->o.color, 4);
    field(last_observed, s->o.last_obs, 8);
    field(voxel_flags, s->o.vflags, 1);
    field(sem_label, s->o.sem_label, 4);
    if (e != hipSuccess) return fail(KHR_EDEVICE, "snapshot download failed: %s", hipGetErrorString(e));
  }
  HIP_TRY(hipEventRecord(s->ev_copied, c->copy_stream));
  s->copying = true;
  HT("dl_begin_exit");
  return KHR_OK;
}

int64_t khr_snapshot_download_end(khr_snapshot* s) {
  if (!s) return fail(KHR_EINVAL, "null snapshot");
  if (!s->copying) return fail(KHR_ESTATE, "no download in flight (khr_snapshot_download_begin first)");
  HT("dl_end_enter");
  HIP_TRY(hipEventSynchronize(s->ev_copied));
  HT("dl_end_exit");
  s->copying = false;
  return s->n;
}

void khr_snapshot_release(khr_snapshot* s) {
  if (!s) return;
  if (s->copying) (void)hipEventSynchronize(s->ev_copied);  // (the arena must not be recycled under a copy in flight)
  // the arena may be handed to the next snapshot right away: that one's kernels are queued behind this one's on the same
  // stream.  After khr_destroy (the consumer kept an output longer than the window lived) the arena is simply freed.
  {
    std::lock_guard<std::mutex> lock(s->pool->mu);
    if (s->pool->dead) hipSetDevice(s->device);  // (delete frees the arena)
    else s->pool->free.push_back(std::move(s->arena));
  }
  delete s;
}

int64_t khr_mesh_num_vertices(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  int rc = refreshMeshTotals(c);
  if (rc) return rc;
  return static_cast<int64_t>(c->mesh_total);
}

int64_t khr_download_mesh(khr_ctx* c, float* points, uint8_t* colors_rgba, uint32_t* labels, uint64_t* first_seen,
                          uint64_t* stamps, int64_t cap) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (c->fetch_pending) {  // a gather queued by khr_fetch_mesh_launch writes the staging block this call is about to fill
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->fetch_pending = false;  // (a later khr_fetch_mesh starts over)
  }
  // Two host round trips in all: (1) totals + counters (skipped when they are current), (2) block index, flags, mesh
  // descriptors and the vertex arrays as one batch of asynchronous copies into the pinned staging buffer.
  int rc = c->mesh_stale ? refreshMeshTotals(c) : (c->counters_gen == c->map_gen ? KHR_OK : readCounters(c));
  if (rc) return rc;
  const uint32_t nslots = c->h_counters[C_MAX_SLOT];
  // (`all` = the whole vertex buffer, blocks archived since the last meshing included: it sizes the staging buffer only;
  // the caller's capacity is compared with the LIVE blocks' total below)
  const size_t all = c->mesh_total;
  const MeshBuffers& mb = c->mesh[c->mesh_cur];
  auto al = [](size_t b) { return (b + 63) & ~static_cast<size_t>(63); };
  const size_t o_idx = 0, o_flag = o_idx + al(sizeof(int4) * nslots), o_desc = o_flag + al(sizeof(uint32_t) * nslots);
  const size_t o_p = o_desc + al(sizeof(MeshDesc) * nslots), o_c = o_p + al(points ? all * 12 : 0);
  const size_t o_l = o_c + al(colors_rgba ? all * 4 : 0), o_s = o_l + al(labels ? all * 4 : 0);
  const size_t bytes = o_s + al((first_seen || stamps) ? all * 8 : 0);
  if ((rc = ensureStage(c, bytes))) return rc;
  char* st = static_cast<char*>(c->h_stage.get());
  if (nslots) {
    HIP_TRY(hipMemcpyAsync(st + o_idx, c->m.blk_index, sizeof(int4) * nslots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(st + o_flag, c->m.blk_flags, sizeof(uint32_t) * nslots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(st + o_desc, c->m.mesh_desc, sizeof(MeshDesc) * nslots, hipMemcpyDeviceToHost, c->stream));
  }
  if (all) {
    if (points) HIP_TRY(hipMemcpyAsync(st + o_p, mb.points, all * 12, hipMemcpyDeviceToHost, c->stream));
    if (colors_rgba) HIP_TRY(hipMemcpyAsync(st + o_c, mb.colors, all * 4, hipMemcpyDeviceToHost, c->stream));
    if (labels) HIP_TRY(hipMemcpyAsync(st + o_l, mb.labels, all * 4, hipMemcpyDeviceToHost, c->stream));
    if (first_seen || stamps) HIP_TRY(hipMemcpyAsync(st + o_s, mb.stamps, all * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int4* idx = reinterpret_cast<const int4*>(st + o_idx);
  const uint32_t* flg = reinterpret_cast<const uint32_t*>(st + o_flag);
  const MeshDesc* desc = reinterpret_cast<const MeshDesc*>(st + o_desc);
  c->host_flags.assign(flg, flg + nslots);
  c->host_index.clear();
  for (uint32_t sl = 0; sl < nslots; ++sl)
    if (flg[sl] & BLK_LIVE) c->host_index[{idx[sl].x, idx[sl].y, idx[sl].z}] = sl;
  c->host_index_valid = true;
  int64_t total = 0;
  for (auto& kv : c->host_index) total += desc[kv.second].count;
  if (total > cap) return fail(KHR_EINVAL, "mesh has %lld vertices, cap %lld", static_cast<long long>(total), static_cast<long long>(cap));
  if (total == 0) return 0;
  const float* hp = reinterpret_cast<const float*>(st + o_p);
  const uint32_t* hc = reinterpret_cast<const uint32_t*>(st + o_c);
  const uint32_t* hl = reinterpret_cast<const uint32_t*>(st + o_l);
  const uint64_t* hs = reinterpret_cast<const uint64_t*>(st + o_s);
  int64_t n = 0;
  for (auto& kv : c->host_index) {  // sorted block order (combineMeshLayer iterates the mesh layer)
    const MeshDesc d = desc[kv.second];
    if (!d.count) continue;
    if (points) std::memcpy(points + 3 * n, hp + 3 * static_cast<size_t>(d.offset), 12ull * d.count);
    if (colors_rgba) std::memcpy(colors_rgba + 4 * n, hc + d.offset, 4ull * d.count);
    if (labels) std::memcpy(labels + n, hl + d.offset, 4ull * d.count);
    if (first_seen) std::memcpy(first_seen + n, hs + d.offset, 8ull * d.count);
    if (stamps) std::memcpy(stamps + n, hs + d.offset, 8ull * d.count);
    n += d.count;
  }
  return n;
}

// one launch + one host wait: the device gathers index / flags / descriptors / vertex arrays into the pinned staging
// buffer (k_mesh_gather), the host orders the blocks and hands out views of arrays it owns
// first half of khr_fetch_mesh for a pipelined consumer: the gather of the CURRENT mesh into the pinned staging block is queued
// behind the stream's work and nothing is awaited; the next khr_fetch_mesh only collects it.  Collect before the next
// khr_generate_mesh (the vertex buffers flip there) and before any other call that uses the staging block.
static int fetchMeshLaunch(khr_ctx* c) {
  const MeshBuffers& mb = c->mesh[c->mesh_cur];
  ++c->fetch_ticket;
  if (c->fetch_ticket == 0) ++c->fetch_ticket;
  static_cast<volatile uint32_t*>(c->h_stage.get())[15] = 0u;
  hipLaunchKernelGGL(k_mesh_gather, dim3(256), dim3(256), 0, c->stream, c->m, mb, c->d_mesh_offset + c->m.capacity,
                     static_cast<uint32_t*>(c->h_stage.dev()), static_cast<uint64_t>(c->h_stage.count() / 4), c->d_fetch_done, c->fetch_ticket);
  HIP_TRY(hipGetLastError());
  HT("fetch_launched");
  return KHR_OK;
}

// The pinned staging block of the mesh fetches grows on demand (x 1.5): a growth is a hipHostFree + hipHostMalloc of tens of
// megabytes -- tens of MILLISECONDS -- and a repeated gather.  A consumer that takes a mesh per output reserves once instead.
int khr_reserve_mesh_staging(khr_ctx* c, uint64_t n_vertices) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  const size_t cap = c->m.capacity;
  const size_t bytes = 4096 + (sizeof(int4) + sizeof(uint32_t) + sizeof(MeshDesc) + 64) * cap + 40 * static_cast<size_t>(n_vertices);
  // (exactly this many bytes, not x 1.5: the caller named its bound)
  if (bytes <= c->h_stage.count()) return KHR_OK;  // (nothing is replaced: a gather queued by khr_fetch_mesh_launch stays valid)
  HIP_TRY(hipStreamSynchronize(c->stream));  // (a gather in flight writes the block that is about to be replaced)
  c->fetch_pending = false;                  // ... and what it gathered goes with the block: the next khr_fetch_mesh starts over
  return c->h_stage.reserve(bytes);
}

int khr_fetch_mesh_launch(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  // (sized from the previous fetch: a mesh that has outgrown the block is fetched again, synchronously, by khr_fetch_mesh)
  int rc = ensureStage(c, 1u << 20);
  if (rc) return rc;
  if ((rc = fetchMeshLaunch(c))) return rc;
  c->fetch_pending = true;
  return KHR_OK;
}

int64_t khr_fetch_mesh(khr_ctx* c, khr_mesh_view* out) {
  if (!c || !out) return fail(KHR_EINVAL, "null argument");
  *out = khr_mesh_view{};
  c->fm_order.clear();
  c->fm_total = 0;
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensureStage(c, 1u << 20);
  if (rc) return rc;
  const uint32_t* h = static_cast<const uint32_t*>(c->h_stage.get());
  for (int attempt = 0; attempt < 2; ++attempt) {
    const bool launched_before = attempt == 0 && c->fetch_pending;
    c->fetch_pending = false;
    if (!launched_before && (rc = fetchMeshLaunch(c))) return rc;
    if ((rc = waitWord(c, static_cast<volatile uint32_t*>(c->h_stage.get()) + 15, c->fetch_ticket, "mesh gather"))) return rc;
    HT("fetch_arrived");
    if (h[2]) return fail(KHR_ENOMEM, "mesh needs %u vertices, max_mesh_vertices=%llu", h[0], static_cast<unsigned long long>(c->cfg.max_mesh_vertices));
    if (h[3]) break;
    if (attempt == 1) return fail(KHR_ENOMEM, "mesh staging of %u words", h[4]);
    const size_t need = static_cast<size_t>(h[4]) * 4;
    if ((rc = ensureStage(c, need))) return rc;
    h = static_cast<const uint32_t*>(c->h_stage.get());
  }
  const uint32_t total_dev = h[0], nslots = h[1];
  c->mesh_total = total_dev;
  c->stats.n_mesh_vertices = total_dev;
  c->mesh_stale = false;
  const int4* idx = reinterpret_cast<const int4*>(h + h[8]);
  const uint32_t* flg = h + h[9];
  const MeshDesc* desc = reinterpret_cast<const MeshDesc*>(h + h[10]);
  const float* hp = reinterpret_cast<const float*>(h + h[11]);
  const uint32_t* hc = h + h[12];
  const uint32_t* hl = h + h[13];
  const uint64_t* hs = reinterpret_cast<const uint64_t*>(h + h[14]);
  // only the blocks that carry vertices matter, in sorted block order (combineMeshLayer iterates the mesh layer):
  // a sort of those few, not a map of every live block
  std::vector<uint32_t> order;
  size_t total = 0;
  for (uint32_t sl = 0; sl < nslots; ++sl)
    if ((flg[sl] & BLK_LIVE) && desc[sl].count) {
      order.push_back(sl);
      total += desc[sl].count;
    }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return idx[a].x != idx[b].x ? idx[a].x < idx[b].x : (idx[a].y != idx[b].y ? idx[a].y < idx[b].y : idx[a].z < idx[b].z);
  });
  HT("fetch_sorted");
  c->fm_order.swap(order);
  c->fm_total = total;
  out->num_vertices = static_cast<int64_t>(total);
  return static_cast<int64_t>(total);
}

// second half of khr_fetch_mesh: the staged vertex arrays, block by block in sorted block order, into the caller's arrays
// (any pointer may be NULL).  No device access.
int khr_fetch_mesh_into(khr_ctx* c, float* points, uint8_t* colors_rgba, uint32_t* labels, uint64_t* first_seen, uint64_t* stamps) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->h_stage || c->fetch_ticket == 0) return fail(KHR_ESTATE, "no khr_fetch_mesh before khr_fetch_mesh_into");
  const uint32_t* h = static_cast<const uint32_t*>(c->h_stage.get());
  const MeshDesc* desc = reinterpret_cast<const MeshDesc*>(h + h[10]);
  const float* hp = reinterpret_cast<const float*>(h + h[11]);
  const uint32_t* hc = h + h[12];
  const uint32_t* hl = h + h[13];
  const uint64_t* hs = reinterpret_cast<const uint64_t*>(h + h[14]);
  // block by block in sorted order; a large mesh (the window's: ~0.6 M vertices, 22 MB) is split over a few threads -- one
  // thread copies out of the pinned block at ~12 GB/s, and a host consumer that takes a mesh per output is bound by exactly this
  const size_t nb = c->fm_order.size();
  std::vector<size_t> first(nb + 1, 0);
  for (size_t i = 0; i < nb; ++i) first[i + 1] = first[i] + desc[c->fm_order[i]].count;
  auto copy_range = [&](size_t b0, size_t b1) {
    for (size_t i = b0; i < b1; ++i) {
      const MeshDesc d = desc[c->fm_order[i]];
      const size_t n = first[i];
      if (points) std::memcpy(points + 3 * n, hp + 3 * static_cast<size_t>(d.offset), 12ull * d.count);
      if (colors_rgba) std::memcpy(colors_rgba + 4 * n, hc + d.offset, 4ull * d.count);
      if (labels) std::memcpy(labels + n, hl + d.offset, 4ull * d.count);
      if (first_seen) std::memcpy(first_seen + n, hs + d.offset, 8ull * d.count);
      if (stamps) std::memcpy(stamps + n, hs + d.offset, 8ull * d.count);
    }
  };
  const size_t total = first[nb];
  const int n_thr = total >= (1u << 16) ? 4 : 1;  // (>= 64 k vertices: ~2.4 MB)
  if (n_thr == 1) {
    copy_range(0, nb);
  } else {
    std::vector<std::thread> pool;
    size_t b0 = 0;
    for (int t = 0; t < n_thr; ++t) {
      // block range whose vertices end at the t-th share of the total
      const size_t want = total * static_cast<size_t>(t + 1) / n_thr;
      size_t b1 = static_cast<size_t>(std::lower_bound(first.begin(), first.end(), want) - first.begin());
      b1 = t + 1 == n_thr ? nb : std::min(nb, std::max(b0, b1));
      if (t + 1 < n_thr) pool.emplace_back(copy_range, b0, b1);
      else copy_range(b0, b1);
      b0 = b1;
    }
    for (std::thread& th : pool) th.join();
  }
  HT("fetch_copied");
  return KHR_OK;
}

// ---- welded mesh (khr_kernels_weld.h, ASSUMPTIONS.md A.16) ----------------------------------------------------------------
int khr_weld_mesh(khr_ctx* c, float resolution, khr_weld_stats* stats) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (stats) *stats = khr_weld_stats{};
  c->weld_valid = false;  // (a failed weld discards the earlier result)
  c->weld_stats = khr_weld_stats{};
  if (!std::isfinite(resolution) || !(resolution > 0.f)) return fail(KHR_EINVAL, "khr_weld_mesh: resolution must be finite and > 0");
  if (c->cfg.world_size > 1)
    return fail(KHR_ESTATE, "khr_weld_mesh needs the whole mesh: world_size is %d (indices are rank-local; weld after the gather)", c->cfg.world_size);
  HIP_TRY(hipSetDevice(c->device));
  int rc = refreshMeshTotals(c);  // (host wait 1, only when the total is not current; KHR_ENOMEM in the overflow state)
  if (rc) return rc;
  // the extent of the vertex buffer: vertices of blocks archived since the meshing included, so an upper bound of the soup
  const uint64_t n_cap64 = c->mesh_total;
  if (n_cap64 == 0) {
    c->weld_valid = true;
    return KHR_OK;
  }
  if (n_cap64 > (1ull << 30)) return fail(KHR_ENOMEM, "khr_weld_mesh: %llu vertices, at most 2^30", static_cast<unsigned long long>(n_cap64));
  const uint32_t n_cap = static_cast<uint32_t>(n_cap64), cap = c->m.capacity, nf_cap = n_cap / 3u;
  if ((rc = ensureSortKeys(c))) return rc;
  uint32_t tsize = 4;
  while (tsize < 2u * n_cap) tsize <<= 1;
  // the three areas; a growth waits for whatever still reads the old block (a device-to-device copy of the last result)
  Arena wa, oa;
  const size_t w_cnt = wa.take(4ull * (cap + 1)), w_base = wa.take(4ull * (cap + 1)), w_off = wa.take(4ull * cap), w_src = wa.take(4ull * n_cap),
               w_hs = wa.take(4ull * n_cap), w_rep = wa.take(4ull * (n_cap + 1)), w_widx = wa.take(4ull * (n_cap + 1)), w_keep = wa.take(4ull * (nf_cap + 1)),
               w_fidx = wa.take(4ull * (nf_cap + 1)), w_keys = wa.take(8ull * tsize), w_vals = wa.take(4ull * tsize), w_head = wa.take(4ull * kWeldHeadWords);
  const size_t work_bytes = wa.bytes();
  const size_t o_p = oa.take(12ull * n_cap), o_c = oa.take(4ull * n_cap), o_l = oa.take(4ull * n_cap), o_s = oa.take(8ull * n_cap),
               o_f = oa.take(12ull * (nf_cap + 1)), o_v = oa.take(4ull * n_cap);
  const size_t out_bytes = oa.bytes();
  const int scan_len = static_cast<int>(std::max(n_cap, cap) + 1u);
  size_t cub_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), scan_len, c->stream));
  cub_bytes = std::max<size_t>(cub_bytes, 256);
  if (work_bytes > c->d_weld_work.count() || out_bytes > c->d_weld_out.count() || cub_bytes > c->d_weld_cub.count()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_weld_work.reserve(work_bytes) || c->d_weld_out.reserve(out_bytes) || c->d_weld_cub.reserve(cub_bytes))
      return fail(KHR_ENOMEM, "khr_weld_mesh: buffers for %u vertices (%zu bytes)", n_cap, work_bytes + out_bytes + cub_bytes);
  }
  if (!c->h_weld && c->h_weld.alloc(kWeldHeadWords)) return fail(KHR_ENOMEM, "khr_weld_mesh: page-locked counts");
  uint8_t* const wb = c->d_weld_work;
  WeldWork w{};
  w.blk_count = reinterpret_cast<uint32_t*>(wb + w_cnt), w.blk_base = reinterpret_cast<uint32_t*>(wb + w_base);
  w.blk_off = reinterpret_cast<uint32_t*>(wb + w_off), w.src = reinterpret_cast<uint32_t*>(wb + w_src);
  w.hslot = reinterpret_cast<uint32_t*>(wb + w_hs), w.is_rep = reinterpret_cast<uint32_t*>(wb + w_rep);
  w.widx = reinterpret_cast<uint32_t*>(wb + w_widx), w.keep = reinterpret_cast<uint32_t*>(wb + w_keep);
  w.fidx = reinterpret_cast<uint32_t*>(wb + w_fidx), w.keys = reinterpret_cast<uint64_t*>(wb + w_keys);
  w.vals = reinterpret_cast<uint32_t*>(wb + w_vals), w.head = reinterpret_cast<uint32_t*>(wb + w_head);
  w.mask = tsize - 1u, w.n_cap = n_cap;
  w.max_vertices = static_cast<uint32_t>(std::min<uint64_t>(c->cfg.max_mesh_vertices, 0xfffffff0ull));
  uint8_t* const ob = c->d_weld_out;
  WeldOut& out = c->weld_out;
  out.points = reinterpret_cast<float*>(ob + o_p), out.colors = reinterpret_cast<uint32_t*>(ob + o_c);
  out.labels = reinterpret_cast<uint32_t*>(ob + o_l), out.stamps = reinterpret_cast<uint64_t*>(ob + o_s);
  out.faces = reinterpret_cast<uint32_t*>(ob + o_f), out.soup_to_vertex = reinterpret_cast<uint32_t*>(ob + o_v);
  const MeshBuffers mb = c->mesh[c->mesh_cur];
  hipStream_t st = c->stream;
  // KHR_WELD_MERGE=0: every lane inserts for itself (A/B switch of the wave-level key merge, results identical)
  const char* const env = std::getenv("KHR_WELD_MERGE");
  const bool merge = !(env && env[0] == '0');
  hipLaunchKernelGGL(k_weld_clear, dim3(std::min(gridFor(tsize / 2), 2048)), dim3(256), 0, st, w);
  // the live blocks in sorted (x, y, z) order, as the checkpoint stream orders them
  HIP_TRY(hipMemsetAsync(c->d_slice_count, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_ckpt_select, dim3(std::min(gridFor(cap), 1024)), dim3(256), 0, st, c->m, c->d_slice_count, c->d_slice_keys);
  HIP_TRY(hipGetLastError());
  if ((rc = sortKeys(c))) return rc;
  hipLaunchKernelGGL(k_weld_block_counts, dim3(gridFor(static_cast<size_t>(cap) + 1)), dim3(256), 0, st, c->m, c->d_slice_keys, c->d_slice_count, w);
  size_t tb = c->d_weld_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_weld_cub.get(), tb, w.blk_count, w.blk_base, static_cast<int>(cap + 1u), st));
  if (merge) hipLaunchKernelGGL((k_weld_insert<true>), dim3(gridFor(n_cap)), dim3(256), 0, st, c->m, mb, resolution, w);
  else hipLaunchKernelGGL((k_weld_insert<false>), dim3(gridFor(n_cap)), dim3(256), 0, st, c->m, mb, resolution, w);
  hipLaunchKernelGGL(k_weld_resolve, dim3(gridFor(static_cast<size_t>(n_cap) + 1)), dim3(256), 0, st, cap, w);
  tb = c->d_weld_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_weld_cub.get(), tb, w.is_rep, w.widx, static_cast<int>(n_cap + 1u), st));
  hipLaunchKernelGGL(k_weld_vertices, dim3(gridFor(n_cap)), dim3(256), 0, st, cap, mb, w, out);
  hipLaunchKernelGGL(k_weld_face_flags, dim3(gridFor(static_cast<size_t>(nf_cap) + 1)), dim3(256), 0, st, cap, w, out);
  tb = c->d_weld_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_weld_cub.get(), tb, w.keep, w.fidx, static_cast<int>(nf_cap + 1u), st));
  hipLaunchKernelGGL(k_weld_faces, dim3(gridFor(static_cast<size_t>(nf_cap) + 1)), dim3(256), 0, st, cap, w, out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(c->h_weld.get(), w.head, sizeof(uint32_t) * kWeldHeadWords, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // (host wait 2: the counts)
  const uint32_t* h = c->h_weld;
  if (h[0] & kWeldErrBounds) return fail(KHR_ESTATE, "khr_weld_mesh: the mesh descriptors do not match the vertex buffer (%u vertices)", n_cap);
  if (h[0] & kWeldErrRange)
    return fail(KHR_EINVAL, "khr_weld_mesh: a vertex lies outside the cell range [-2^20, 2^20) at resolution %g: too fine for the extent of the map",
                static_cast<double>(resolution));
  khr_weld_stats s{};
  s.n_soup_vertices = h[1], s.n_vertices = h[2], s.n_faces = h[3];
  s.n_degenerate_faces = s.n_soup_vertices / 3 - s.n_faces;
  c->weld_stats = s;
  c->weld_valid = true;
  if (stats) *stats = s;
  return KHR_OK;
}

int khr_weld_mesh_into(khr_ctx* c, int on_device, float* points, uint8_t* colors_rgba, uint32_t* labels, uint64_t* first_seen, uint64_t* stamps,
                       uint32_t* faces, uint32_t* soup_to_vertex) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->weld_valid) return fail(KHR_ESTATE, "no successful khr_weld_mesh before khr_weld_mesh_into");
  const khr_weld_stats& s = c->weld_stats;
  if (s.n_soup_vertices == 0) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const WeldOut& o = c->weld_out;
  const size_t nv = s.n_vertices, nf = s.n_faces, ns = s.n_soup_vertices;
  hipError_t e = hipSuccess;
  auto field = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, kind, c->stream);
  };
  field(points, o.points, 12 * nv);
  field(colors_rgba, o.colors, 4 * nv);
  field(labels, o.labels, 4 * nv);
  field(first_seen, o.stamps, 8 * nv);
  field(stamps, o.stamps, 8 * nv);
  field(faces, o.faces, 12 * nf);
  field(soup_to_vertex, o.soup_to_vertex, 4 * ns);
  if (e != hipSuccess) return fail(KHR_EDEVICE, "khr_weld_mesh_into: copy failed: %s", hipGetErrorString(e));
  if (!on_device) HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

// ---- another map fused into the live map (khr_merge_map; ASSUMPTIONS.md A.17, device side: khr_kernels_merge.h) ----------------
// What khr_merge_map and khr_diff_map ask of their pair of contexts and of the sampling part of their request (`call` names the
// caller in the texts); fills X's mode, min_weight, offset or transforms, row stride and stamps.
static int mergeCheckPair(const char* call, khr_ctx* c, khr_ctx* src, const void* rq, int mode, const int32_t* voxel_offset, const double* T,
                          float min_weight, MergeArgs* Xo) {
  if (!c || !src || !rq) return fail(KHR_EINVAL, "%s: null argument", call);
  if (src == c) return fail(KHR_EINVAL, "%s: src and dst are the same context", call);
  if (c->device != src->device) return fail(KHR_EINVAL, "%s: the contexts live on different devices (%d and %d)", call, src->device, c->device);
  {
    const khr_checkpoint_header hs = ckptHeaderFor(src->cfg, 0), hd = ckptHeaderFor(c->cfg, 0);
#define KHR_MERGE_FIELD(name, fmt, cast)                                                                                          \
  if (hs.name != hd.name)                                                                                                         \
    return fail(KHR_EINVAL, "%s: " #name " is " fmt " in the source and " fmt " in the destination", call, static_cast<cast>(hs.name), \
                static_cast<cast>(hd.name));
    KHR_MERGE_FIELD(voxel_size, "%.9g", double)
    KHR_MERGE_FIELD(voxels_per_side, "%d", int)
    KHR_MERGE_FIELD(truncation_distance, "%.9g", double)
    KHR_MERGE_FIELD(with_semantics, "%d", int)
    KHR_MERGE_FIELD(with_tracking, "%d", int)
    KHR_MERGE_FIELD(num_labels, "%d", int)
    KHR_MERGE_FIELD(semantic_mode, "%d", int)
#undef KHR_MERGE_FIELD
  }
  if (mode != KHR_MERGE_ALIGNED && mode != KHR_MERGE_RESAMPLE) return fail(KHR_EINVAL, "%s: unknown mode %d", call, mode);
  if (!std::isfinite(min_weight) || min_weight < 0.f) return fail(KHR_EINVAL, "%s: min_weight must be finite and >= 0", call);
  if (c->cfg.world_size > 1 || src->cfg.world_size > 1)
    return fail(KHR_ESTATE, "%s needs whole maps: world_size is %d in the source and %d in the destination", call, src->cfg.world_size,
                c->cfg.world_size);
  MergeArgs& X = *Xo;
  X = MergeArgs{};
  X.mode = mode;
  X.min_weight = min_weight > 0.f ? min_weight : c->p.mesh_min_weight;
  X.ks_src = src->p.KS;
  X.src_stamp = src->last_track_stamp;
  X.dst_stamp = c->last_track_stamp;
  if (mode == KHR_MERGE_ALIGNED) {
    for (int a = 0; a < 3; ++a) {
      const int64_t o = voxel_offset[a];
      if (o <= -(1ll << 30) || o >= (1ll << 30)) return fail(KHR_EINVAL, "%s: voxel_offset[%d] = %lld, |offset| must be below 2^30", call, a, static_cast<long long>(o));
      X.off[a] = voxel_offset[a];
    }
  } else {
    for (int i = 0; i < 16; ++i)
      if (!std::isfinite(T[i])) return fail(KHR_EINVAL, "%s: dst_T_src is not finite", call);
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return fail(KHR_EINVAL, "%s: the last row of dst_T_src is not 0 0 0 1", call);
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += T[4 * k + i] * T[4 * k + j];
        worst = std::max(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
      }
    if (worst > 1e-5) return fail(KHR_EINVAL, "%s: dst_T_src is not rigid: max |R^T R - I| = %.3g", call, worst);
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) + T[2] * (T[4] * T[9] - T[5] * T[8]);
    if (det < 0.0) return fail(KHR_EINVAL, "%s: dst_T_src is a reflection (det R = %.3g)", call, det);
    for (int a = 0; a < 3; ++a) {  // src_T_dst = [R^T | -R^T t] in double, cast once
      double t = 0.0;
      for (int k = 0; k < 3; ++k) {
        X.M[4 * a + k] = static_cast<float>(T[4 * k + a]);
        t += T[4 * k + a] * T[4 * k + 3];
        X.F[4 * a + k] = static_cast<float>(T[4 * a + k]);
      }
      X.M[4 * a + 3] = static_cast<float>(-t);
      X.F[4 * a + 3] = static_cast<float>(T[4 * a + 3]);
    }
  }
  return KHR_OK;
}

constexpr size_t kMergeCounterWords = 32;  // the counter block of a merge (12 words) or a diff (kDiffCounterWords)
static_assert(kDiffCounterWords <= static_cast<int>(kMergeCounterWords), "the counters of a diff fit the block");

// The scratch of a merge or a diff in context c (calls on one context are serialised: they share it), sized by what the pool of
// `src` can reach (its block count is not known without a wait) with `words` 32-bit words per candidate behind the list; queues
// the clears of the counters and the candidate set on c's stream, behind everything queued on src's stream.
static int mergeBeginScratch(const char* call, khr_ctx* c, khr_ctx* src, int mode, size_t words, MergeScratch* So) {
  const size_t reach = mode == KHR_MERGE_ALIGNED ? kMergeReachAligned : kMergeReachResample;
  const size_t cap = reach * static_cast<size_t>(src->m.capacity);
  if (cap > (1ull << 30)) return fail(KHR_ENOMEM, "%s: %zu candidate blocks, at most 2^30", call, cap);
  size_t set_n = 64;
  while (set_n < 2 * cap) set_n <<= 1;
  if (set_n > c->d_merge_set.count() || cap > c->d_merge_cand.count() || words * cap > c->d_merge_words.count() ||
      kMergeCounterWords > c->d_merge_ctr.count() || !c->h_merge) {
    HIP_TRY(hipStreamSynchronize(c->stream));  // (whatever still uses the old blocks)
    int rc = KHR_OK;
    KHR_CHAIN(c->d_merge_set.reserve(set_n));
    KHR_CHAIN(c->d_merge_cand.reserve(cap));
    KHR_CHAIN(c->d_merge_words.reserve(words * cap));
    KHR_CHAIN(c->d_merge_ctr.reserve(kMergeCounterWords));
    KHR_CHAIN(c->h_merge.reserve(kMergeCounterWords));
    if (rc) return fail(KHR_ENOMEM, "%s: scratch for %zu candidate blocks", call, cap);
  }
  KHR_TRY(c->ev_merge.ensure());
  MergeScratch& S = *So;
  S = MergeScratch{};
  S.set_keys = c->d_merge_set;
  S.set_mask = static_cast<uint32_t>(set_n - 1);
  S.cand = c->d_merge_cand;
  S.cap = static_cast<uint32_t>(cap);
  S.cand_slot = c->d_merge_words;
  S.cand_hit = c->d_merge_words + cap;
  S.touched = c->d_merge_words + 2 * cap;
  S.ctr = c->d_merge_ctr;
  S.ctr64 = reinterpret_cast<unsigned long long*>(c->d_merge_ctr + MC_COUNT);
  // behind everything queued on the source's stream
  if (c->stream != src->stream) {
    HIP_TRY(hipEventRecord(c->ev_merge, src->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_merge, 0));
  }
  HIP_TRY(hipMemsetAsync(S.ctr, 0, kMergeCounterWords * sizeof(uint32_t), c->stream));
  HIP_TRY(hipMemsetAsync(S.set_keys, 0xff, set_n * sizeof(uint64_t), c->stream));
  return KHR_OK;
}

int khr_merge_map(khr_ctx* c, khr_ctx* src, const khr_merge_request* rq, khr_merge_stats* stats) {
  if (stats) *stats = khr_merge_stats{};
  MergeArgs X{};
  KHR_TRY(mergeCheckPair("khr_merge_map", c, src, rq, rq ? rq->mode : 0, rq ? rq->voxel_offset : nullptr, rq ? rq->dst_T_src : nullptr,
                         rq ? rq->min_weight : 0.f, &X));
  HIP_TRY(hipSetDevice(c->device));
  MergeScratch S{};
  KHR_TRY(mergeBeginScratch("khr_merge_map", c, src, rq->mode, 3, &S));
  const size_t cap = S.cap;
  int rc = dispatchVps(c, [&](auto vps) {
    constexpr int V = decltype(vps)::value;
    hipLaunchKernelGGL((k_merge_candidates<V>), dim3(std::max(1, std::min(gridFor(src->m.capacity), 1024))), dim3(256), 0, c->stream, src->m, c->p, X, S);
    HIP_TRY(hipGetLastError());
    const dim3 grid(static_cast<uint32_t>(std::min<size_t>(cap, 8192)));
    if (X.mode == kMergeAligned) hipLaunchKernelGGL((k_merge_probe<V, kMergeAligned>), grid, dim3(256), 0, c->stream, c->m, src->m, c->p, X, S);
    else hipLaunchKernelGGL((k_merge_probe<V, kMergeResample>), grid, dim3(256), 0, c->stream, c->m, src->m, c->p, X, S);
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
  if (rc) return rc;
  // the one host wait: the counts
  uint32_t* const h = c->h_merge;
  HIP_TRY(hipMemcpyAsync(h, S.ctr, 12 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h + 12, &c->m.counters[C_FREE_HEAD], 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  static_assert(C_FREE_HEAD == 0 && C_N_FREE == 1, "the two free-list words are adjacent");
  uint64_t v64[2];
  std::memcpy(v64, h + MC_COUNT, sizeof(v64));
  const uint32_t n_list = std::min<uint32_t>(h[MC_LIST], S.cap), n_touched = h[MC_TOUCHED], n_new = h[MC_NEW];
  if (h[MC_ERR] & kMergeErrOverflow) return fail(KHR_EDEVICE, "khr_merge_map: the candidate list overflowed (%u entries, room for %u)", h[MC_LIST], S.cap);
  if (h[MC_ERR] & kMergeErrRange)
    return fail(KHR_EINVAL, "khr_merge_map: a destination block with a valid sample lies outside the block index range [-2^20, 2^20)");
  const uint32_t n_free = h[13] - std::min(h[12], h[13]);
  if (n_new > n_free) return fail(KHR_ENOMEM, "khr_merge_map: the merge needs %u new blocks, the pool (max_blocks %u) has %u free", n_new, c->m.capacity, n_free);
  khr_merge_stats st{};
  st.n_src_blocks = h[MC_SRC];
  st.n_candidate_blocks = h[MC_CAND];
  st.n_touched_blocks = n_touched;
  st.n_new_blocks = n_new;
  st.n_added_voxels = v64[0];
  st.n_merged_voxels = v64[1];
  if (n_touched > 0) {
    hipLaunchKernelGGL(k_merge_insert, dim3(gridFor(n_list)), dim3(256), 0, c->stream, c->m, S);
    HIP_TRY(hipGetLastError());
    rc = dispatchVps(c, [&](auto vps) {
      constexpr int V = decltype(vps)::value;
      const auto write = [&](auto mode) {  // semantics first: it reads the voxel flags the attributes kernel rewrites
        constexpr int M = decltype(mode)::value;
        if (c->p.with_semantics) hipLaunchKernelGGL((k_merge_rows<V, M>), dim3(n_list), dim3(256), 0, c->stream, c->m, src->m, c->p, X, S);
        hipLaunchKernelGGL((k_merge_attributes<V, M>), dim3(n_list), dim3(256), 0, c->stream, c->m, src->m, c->p, X, S);
        hipLaunchKernelGGL((k_merge_apply<V, M>), dim3(n_list), dim3(256), 0, c->stream, c->m, src->m, c->p, X, S);
      };
      if (X.mode == kMergeAligned) write(std::integral_constant<int, kMergeAligned>());
      else write(std::integral_constant<int, kMergeResample>());
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL((k_ckpt_rebuild<V>), dim3(n_touched), dim3(256), 0, c->stream, c->m, c->p, c->wpb, static_cast<const uint32_t*>(S.touched),
                         static_cast<const uint32_t*>(S.ctr + MC_NLIST));
      HIP_TRY(hipGetLastError());
      return KHR_OK;
    });
    if (rc) return rc;
    // ... and the source's later work (a frame, a reset, its destruction) behind the kernels that still read it
    if (c->stream != src->stream) {
      HIP_TRY(hipEventRecord(c->ev_merge, c->stream));
      HIP_TRY(hipStreamWaitEvent(src->stream, c->ev_merge, 0));
    }
    c->host_index_valid = false, ++c->map_gen;
    if (c->explicit_blocks > 0) c->explicit_blocks += n_new;
  }
  if (stats) *stats = st;
  return KHR_OK;
}

// ---- the live map compared with another map (khr_diff_map; ASSUMPTIONS.md A.18, device side: khr_kernels_diff.h) ----------------
int khr_diff_map(khr_ctx* c, khr_ctx* ref, const khr_diff_request* rq, khr_diff_stats* stats) {
  if (stats) *stats = khr_diff_stats{};
  if (c) {  // (a failed diff discards the earlier result)
    c->diff_valid = false;
    c->diff_stats = khr_diff_stats{};
  }
  MergeArgs X{};
  KHR_TRY(mergeCheckPair("khr_diff_map", c, ref, rq, rq ? rq->mode : 0, rq ? rq->voxel_offset : nullptr, rq ? rq->ctx_T_ref : nullptr,
                         rq ? rq->min_weight : 0.f, &X));
  if (!std::isfinite(rq->occupied_distance) || !std::isfinite(rq->free_distance))
    return fail(KHR_EINVAL, "khr_diff_map: occupied_distance and free_distance must be finite");
  if (!(rq->occupied_distance < rq->free_distance))
    return fail(KHR_EINVAL, "khr_diff_map: occupied_distance (%.9g) must be below free_distance (%.9g)", static_cast<double>(rq->occupied_distance),
                static_cast<double>(rq->free_distance));
  const DiffArgs D{rq->occupied_distance, rq->free_distance};
  HIP_TRY(hipSetDevice(c->device));
  // per candidate: its slot in `now`, its two counts; the changed list: a candidate and a 64-bit key
  MergeScratch S{};
  KHR_TRY(mergeBeginScratch("khr_diff_map", c, ref, rq->mode, kDiffWordsPerCandidate, &S));
  const size_t cap = S.cap;
  DiffWork W{};
  W.words = c->d_merge_words;
  W.cap = S.cap;
  hipStream_t st = c->stream;
  int rc = dispatchVps(c, [&](auto vps) {
    constexpr int V = decltype(vps)::value;
    hipLaunchKernelGGL((k_merge_candidates<V>), dim3(std::max(1, std::min(gridFor(ref->m.capacity), 1024))), dim3(256), 0, st, ref->m, c->p, X, S);
    HIP_TRY(hipGetLastError());
    const dim3 grid(static_cast<uint32_t>(std::min<size_t>(cap, 8192)));
    if (X.mode == kMergeAligned) hipLaunchKernelGGL((k_diff_count<V, kMergeAligned>), grid, dim3(256), 0, st, c->m, ref->m, c->p, X, D, S, W);
    else hipLaunchKernelGGL((k_diff_count<V, kMergeResample>), grid, dim3(256), 0, st, c->m, ref->m, c->p, X, D, S, W);
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
  if (rc) return rc;
  // the one host wait: the counts
  uint32_t* const h = c->h_merge;
  HIP_TRY(hipMemcpyAsync(h, S.ctr, kDiffCounterWords * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h[MC_ERR] & kMergeErrOverflow) return fail(KHR_EDEVICE, "khr_diff_map: the candidate list overflowed (%u entries, room for %u)", h[MC_LIST], S.cap);
  uint64_t v64[DV_COUNT];
  std::memcpy(v64, h + DC_COUNT, sizeof(v64));
  khr_diff_stats s{};
  s.n_ref_blocks = h[MC_SRC];
  s.n_candidate_blocks = h[MC_CAND];
  s.n_present_blocks = h[DC_PRESENT];
  s.n_compared_voxels = v64[DV_COMPARED];
  s.n_appeared = v64[DV_APPEARED];
  s.n_disappeared = v64[DV_DISAPPEARED];
  s.n_only_now = v64[DV_ONLY_NOW];
  s.n_only_then = v64[DV_ONLY_THEN];
  s.n_changed_blocks = h[DC_CHANGED];
  const uint64_t n64 = s.n_appeared + s.n_disappeared;
  if (n64 > (1ull << 30)) return fail(KHR_ENOMEM, "khr_diff_map: %llu changed voxels, at most 2^30", static_cast<unsigned long long>(n64));
  if (h[DC_CHANGED] > S.cap || (h[DC_CHANGED] == 0) != (n64 == 0))
    return fail(KHR_EDEVICE, "khr_diff_map: inconsistent counts (%u changed blocks, %llu changed voxels)", h[DC_CHANGED], static_cast<unsigned long long>(n64));
  const uint32_t m = h[DC_CHANGED], n = static_cast<uint32_t>(n64);
  if (m > 0) {
    // the work area and the result; nothing is queued on the stream here (the wait above), so a growth frees nothing in use
    Arena wa;
    const size_t w_key = wa.take(8ull * m), w_cand = wa.take(4ull * m), w_cnt = wa.take(4ull * (m + 1ull)), w_first = wa.take(4ull * (m + 1ull));
    const size_t work_bytes = wa.bytes(), out_bytes = diffLayout(n, m).bytes;
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                               static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<int>(m), 0, 63, st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<int>(m + 1u), st));
    const size_t cub_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 256);
    if (c->d_diff_work.reserve(work_bytes) || c->d_diff_out.reserve(out_bytes) || c->d_diff_cub.reserve(cub_bytes))
      return fail(KHR_ENOMEM, "khr_diff_map: buffers for %u changed voxels in %u blocks (%zu bytes)", n, m, work_bytes + out_bytes + cub_bytes);
    uint8_t* const wb = c->d_diff_work;
    W.sorted_key = reinterpret_cast<uint64_t*>(wb + w_key), W.sorted_cand = reinterpret_cast<uint32_t*>(wb + w_cand);
    W.blk_count = reinterpret_cast<uint32_t*>(wb + w_cnt), W.blk_first = reinterpret_cast<uint32_t*>(wb + w_first);
    W.n_blocks = m, W.n_voxels = n;
    uint8_t* const out = c->d_diff_out;
    // (x, y, z) order: the keys are unique, the result does not depend on the order the workgroups arrived in
    size_t tb = c->d_diff_cub.count();
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(c->d_diff_cub.get(), tb, static_cast<const uint64_t*>(diffChangedKey(W)), W.sorted_key,
                                               static_cast<const uint32_t*>(diffChangedCand(W)), W.sorted_cand, static_cast<int>(m), 0, 63, st));
    hipLaunchKernelGGL(k_diff_block_counts, dim3(gridFor(static_cast<size_t>(m) + 1)), dim3(256), 0, st, W);
    HIP_TRY(hipGetLastError());
    tb = c->d_diff_cub.count();
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_diff_cub.get(), tb, W.blk_count, W.blk_first, static_cast<int>(m + 1u), st));
    rc = dispatchVps(c, [&](auto vps) {
      constexpr int V = decltype(vps)::value;
      if (X.mode == kMergeAligned) hipLaunchKernelGGL((k_diff_emit<V, kMergeAligned>), dim3(m), dim3(256), 0, st, c->m, ref->m, c->p, X, D, static_cast<const int4*>(S.cand), W, out);
      else hipLaunchKernelGGL((k_diff_emit<V, kMergeResample>), dim3(m), dim3(256), 0, st, c->m, ref->m, c->p, X, D, static_cast<const int4*>(S.cand), W, out);
      HIP_TRY(hipGetLastError());
      return KHR_OK;
    });
    if (rc) return rc;
    // ... and ref's later work (a frame, a reset, its destruction) behind the kernel that still reads it
    if (st != ref->stream) {
      HIP_TRY(hipEventRecord(c->ev_merge, st));
      HIP_TRY(hipStreamWaitEvent(ref->stream, c->ev_merge, 0));
    }
  }
  c->diff_stats = s;
  c->diff_valid = true;
  if (stats) *stats = s;
  return KHR_OK;
}

int khr_diff_map_into(khr_ctx* c, int on_device, int32_t* voxels, uint8_t* kind, float* d_now, float* d_then, uint32_t* label, uint64_t* stamp_now,
                      uint64_t* stamp_then, int32_t* blocks, uint32_t* block_appeared, uint32_t* block_disappeared, uint32_t* block_first) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->diff_valid) return fail(KHR_ESTATE, "no successful khr_diff_map before khr_diff_map_into");
  const khr_diff_stats& s = c->diff_stats;
  if (s.n_changed_blocks == 0) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  const hipMemcpyKind dir = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t n = s.n_appeared + s.n_disappeared, m = s.n_changed_blocks;
  const DiffLayout L = diffLayout(n, m);
  const uint8_t* const ob = c->d_diff_out;
  hipError_t e = hipSuccess;
  auto field = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, dir, c->stream);
  };
  field(voxels, ob + L.voxels, 12 * n);
  field(kind, ob + L.kind, n);
  field(d_now, ob + L.d_now, 4 * n);
  field(d_then, ob + L.d_then, 4 * n);
  field(label, ob + L.label, 4 * n);
  field(stamp_now, ob + L.stamp_now, 8 * n);
  field(stamp_then, ob + L.stamp_then, 8 * n);
  field(blocks, ob + L.blocks, 12 * m);
  field(block_appeared, ob + L.block_appeared, 4 * m);
  field(block_disappeared, ob + L.block_disappeared, 4 * m);
  field(block_first, ob + L.block_first, 4 * m);
  if (e != hipSuccess) return fail(KHR_EDEVICE, "khr_diff_map_into: copy failed: %s", hipGetErrorString(e));
  if (!on_device) HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

// ---- connected components of the live map's occupied voxels (khr_segment_map; ASSUMPTIONS.md A.19, device side:
// khr_kernels_segment.h) ----------------------------------------------------------------------------------------------------------
int khr_segment_map(khr_ctx* c, const khr_segment_request* rq, khr_segment_stats* stats) {
  if (stats) *stats = khr_segment_stats{};
  if (c) {  // (a failed call discards the earlier result)
    c->seg_valid = false;
    c->seg_stats = khr_segment_stats{};
  }
  if (!c || !rq) return fail(KHR_EINVAL, "khr_segment_map: null argument");
  if (rq->connectivity != 6 && rq->connectivity != 18 && rq->connectivity != 26)
    return fail(KHR_EINVAL, "khr_segment_map: connectivity is %d, must be 6, 18 or 26", rq->connectivity);
  if (!std::isfinite(rq->min_weight) || rq->min_weight < 0.f) return fail(KHR_EINVAL, "khr_segment_map: min_weight must be finite and >= 0");
  if (!std::isfinite(rq->surface_distance)) return fail(KHR_EINVAL, "khr_segment_map: surface_distance is not finite");
  if (rq->n_labels < 0 || rq->n_labels > 64) return fail(KHR_EINVAL, "khr_segment_map: n_labels is %d, must be 0 .. 64", rq->n_labels);
  if (rq->n_labels > 0 && !rq->labels) return fail(KHR_EINVAL, "khr_segment_map: n_labels is %d and labels is null", rq->n_labels);
  const int64_t min_voxels = std::max<int64_t>(rq->min_voxels, 1);
  if (rq->max_voxels > 0 && rq->max_voxels < min_voxels)
    return fail(KHR_EINVAL, "khr_segment_map: max_voxels (%lld) is below min_voxels (%lld)", static_cast<long long>(rq->max_voxels),
                static_cast<long long>(min_voxels));
  if (c->cfg.world_size > 1)
    return fail(KHR_ESTATE, "khr_segment_map needs the whole map: world_size is %d (a shard cannot see across faces it does not own)", c->cfg.world_size);
  SegMember M{};
  M.min_weight = rq->min_weight > 0.f ? rq->min_weight : c->p.mesh_min_weight;
  M.surface_distance = rq->surface_distance;
  M.flags_require = rq->flags_require, M.flags_exclude = rq->flags_exclude;
  M.n_labels = rq->n_labels;
  for (int i = 0; i < rq->n_labels; ++i) M.labels[i] = static_cast<uint32_t>(rq->labels[i]);
  SegRule R{};
  R.n_dirs = rq->connectivity == 6 ? 3 : (rq->connectivity == 18 ? 9 : 13);
  R.by_label = rq->by_label != 0;
  R.min_voxels = static_cast<unsigned long long>(min_voxels);
  R.max_voxels = rq->max_voxels > 0 ? static_cast<unsigned long long>(rq->max_voxels) : ~0ull;
  HIP_TRY(hipSetDevice(c->device));
  KHR_TRY(ensureSortKeys(c));
  hipStream_t st = c->stream;
  // The scratch holds `bound` blocks: the live blocks where the host index is current (their number is then known without a
  // wait), else the pool's capacity.  Node ids are 32 bits.
  const size_t nv = static_cast<size_t>(c->p.nvox), cap = c->m.capacity;
  const size_t bound = std::max<size_t>(1, c->host_index_valid ? std::min(cap, c->host_index.size()) : cap);
  const size_t nodes = bound * nv;
  Arena wa;
  const size_t w_ctr = wa.take(8 * SC_COUNT), w_ros = wa.take(4 * cap), w_sor = wa.take(4 * bound), w_par = wa.take(4 * nodes), w_cnt = wa.take(4 * nodes),
               w_num = wa.take(4 * (nodes + 1));
  const size_t work_bytes = wa.bytes();
  if (nodes + 1 > static_cast<size_t>(INT32_MAX))  // (the scan counts in int; node ids then fit 32 bits with room for kSegNone)
    return fail(KHR_ENOMEM, "khr_segment_map: %zu blocks of %zu voxels to number, at most 2^31 - 2 voxels (%zu bytes of scratch)", bound, nv, work_bytes);
  size_t cub_bytes = 0;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<int>(nodes + 1), st));
  cub_bytes = std::max<size_t>(cub_bytes, 256);
  if (work_bytes > c->d_seg_work.count() || cub_bytes > c->d_seg_cub.count() || !c->h_seg) {
    HIP_TRY(hipStreamSynchronize(st));  // (whatever still uses the old blocks)
    if (c->d_seg_work.reserve(work_bytes) || c->d_seg_cub.reserve(cub_bytes) || c->h_seg.reserve(SC_COUNT + 1))
      return fail(KHR_ENOMEM, "khr_segment_map: scratch for %zu blocks (%zu bytes)", bound, work_bytes + cub_bytes);
  }
  uint8_t* const wb = c->d_seg_work;
  unsigned long long* const ctr = reinterpret_cast<unsigned long long*>(wb + w_ctr);
  uint32_t* const parent = reinterpret_cast<uint32_t*>(wb + w_par);
  uint32_t* const cnt = reinterpret_cast<uint32_t*>(wb + w_cnt);
  uint32_t* const number = reinterpret_cast<uint32_t*>(wb + w_num);
  SegBlocks B{};
  B.keys = c->d_slice_keys, B.count = c->d_slice_count, B.bound = static_cast<uint32_t>(bound);
  B.rank_of_slot = reinterpret_cast<uint32_t*>(wb + w_ros), B.slot_of_rank = reinterpret_cast<uint32_t*>(wb + w_sor);
  // the live blocks in sorted (x, y, z) order, as the checkpoint stream orders them
  HIP_TRY(hipMemsetAsync(c->d_slice_count, 0, sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(ctr, 0, 8 * SC_COUNT, st));
  hipLaunchKernelGGL(k_ckpt_select, dim3(std::min(gridFor(cap), 1024)), dim3(256), 0, st, c->m, c->d_slice_count, c->d_slice_keys);
  HIP_TRY(hipGetLastError());
  KHR_TRY(sortKeys(c));
  const dim3 block_grid(static_cast<uint32_t>(std::min<size_t>(bound, 8192))), node_grid(static_cast<uint32_t>(std::min<size_t>(gridFor(nodes + 1), 8192)));
  int rc = dispatchVps(c, [&](auto vps) {
    constexpr int V = decltype(vps)::value;
    hipLaunchKernelGGL((k_seg_local<V>), block_grid, dim3(256), 0, st, c->m, c->p, M, R, B, parent, cnt, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_seg_seams<V>), block_grid, dim3(256), 0, st, c->m, c->p, R, B, parent);
    HIP_TRY(hipGetLastError());
    return KHR_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_seg_count, node_grid, dim3(256), 0, st, B, static_cast<uint32_t>(nv), parent, cnt);
  hipLaunchKernelGGL(k_seg_flag, node_grid, dim3(256), 0, st, B, static_cast<uint32_t>(nv), R, static_cast<const uint32_t*>(parent),
                     static_cast<const uint32_t*>(cnt), number, ctr);
  HIP_TRY(hipGetLastError());
  size_t tb = c->d_seg_cub.count();
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_seg_cub.get(), tb, number, number, static_cast<int>(nodes + 1), st));
  // the one host wait: the counts
  unsigned long long* const h = c->h_seg;
  HIP_TRY(hipMemcpyAsync(h, ctr, 8 * SC_COUNT, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h + SC_COUNT, c->d_slice_count, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint32_t n_blocks = 0;
  std::memcpy(&n_blocks, h + SC_COUNT, sizeof(n_blocks));
  if ((h[SC_ERR] & kSegErrBound) || n_blocks > bound)
    return fail(KHR_EDEVICE, "khr_segment_map: %u live blocks, the scratch was sized for %zu", n_blocks, bound);
  khr_segment_stats s{};
  s.n_blocks = n_blocks;
  s.n_member_voxels = h[SC_MEMBERS];
  s.n_components_all = h[SC_ALL], s.n_too_small = h[SC_SMALL], s.n_too_large = h[SC_LARGE], s.n_components = h[SC_KEPT];
  s.n_voxels = h[SC_VOXELS];
  if (s.n_components_all != s.n_too_small + s.n_too_large + s.n_components || s.n_voxels > s.n_member_voxels || s.n_components > s.n_voxels)
    return fail(KHR_EDEVICE, "khr_segment_map: inconsistent counts (%llu components, %llu kept, %llu voxels)",
                static_cast<unsigned long long>(s.n_components_all), static_cast<unsigned long long>(s.n_components), static_cast<unsigned long long>(s.n_voxels));
  const bool list = rq->want_voxels != 0;
  if (s.n_components > 0) {
    const uint32_t m = static_cast<uint32_t>(s.n_components);  // (below 2^32: a component has a node id of its own)
    const uint64_t n = list ? s.n_voxels : 0;
    if (n > (1ull << 30)) return fail(KHR_ENOMEM, "khr_segment_map: a voxel list of %llu entries, at most 2^30 (%llu bytes)", static_cast<unsigned long long>(n),
                                       static_cast<unsigned long long>(48 * n));
    // the result and the sort's work area; nothing is queued on the stream here (the wait above), so a growth frees nothing in use
    const size_t out_bytes = segLayout(m, n).bytes, sort_bytes = 2 * Arena::align(8 * n);
    size_t scan64_bytes = 0, radix_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan64_bytes, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), static_cast<int>(m), st));
    if (n) HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, radix_bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), static_cast<int>(n), 0, 64, st));
    const size_t cub2_bytes = std::max(std::max(scan64_bytes, radix_bytes), cub_bytes);
    if (c->d_seg_out.reserve(out_bytes) || c->d_seg_sort.reserve(sort_bytes) || c->d_seg_cub.reserve(cub2_bytes))
      return fail(KHR_ENOMEM, "khr_segment_map: buffers for %u components and %llu listed voxels (%zu bytes)", m, static_cast<unsigned long long>(n),
                  out_bytes + sort_bytes + cub2_bytes);
    uint8_t* const out = c->d_seg_out;
    const SegLayout L = segLayout(m, n);
    uint64_t* const keys_in = n ? reinterpret_cast<uint64_t*>(c->d_seg_sort.get()) : nullptr;
    uint64_t* const keys_out = n ? reinterpret_cast<uint64_t*>(c->d_seg_sort.get() + Arena::align(8 * n)) : nullptr;
    const dim3 live_grid(static_cast<uint32_t>(std::min<size_t>(std::max<size_t>(1, gridFor(static_cast<size_t>(n_blocks) * nv)), 8192)));
    rc = dispatchVps(c, [&](auto vps) {
      constexpr int V = decltype(vps)::value;
      hipLaunchKernelGGL((k_seg_heads<V>), live_grid, dim3(256), 0, st, c->m, c->p, R, B, static_cast<const uint32_t*>(parent), static_cast<const uint32_t*>(cnt),
                         static_cast<const uint32_t*>(number), m, n, out);
      HIP_TRY(hipGetLastError());
      if (n) hipLaunchKernelGGL((k_seg_reduce<V, true>), live_grid, dim3(256), 0, st, c->m, c->p, R, B, static_cast<const uint32_t*>(parent),
                                static_cast<const uint32_t*>(cnt), static_cast<const uint32_t*>(number), m, n, out, keys_in, ctr);
      else hipLaunchKernelGGL((k_seg_reduce<V, false>), live_grid, dim3(256), 0, st, c->m, c->p, R, B, static_cast<const uint32_t*>(parent),
                              static_cast<const uint32_t*>(cnt), static_cast<const uint32_t*>(number), m, n, out, keys_in, ctr);
      HIP_TRY(hipGetLastError());
      return KHR_OK;
    });
    if (rc) return rc;
    tb = c->d_seg_cub.count();
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(c->d_seg_cub.get(), tb, reinterpret_cast<uint64_t*>(out + L.n_voxels), reinterpret_cast<uint64_t*>(out + L.first),
                                             static_cast<int>(m), st));
    if (n) {
      tb = c->d_seg_cub.count();
      HIP_TRY(hipcub::DeviceRadixSort::SortKeys(c->d_seg_cub.get(), tb, static_cast<const uint64_t*>(keys_in), keys_out, static_cast<int>(n), 0, 64, st));
      rc = dispatchVps(c, [&](auto vps) {
        hipLaunchKernelGGL((k_seg_emit<decltype(vps)::value>), dim3(static_cast<uint32_t>(std::min<size_t>(gridFor(n), 8192))), dim3(256), 0, st,
                           static_cast<const uint64_t*>(c->d_slice_keys), static_cast<const uint64_t*>(keys_out), m, n, n_blocks, out);
        HIP_TRY(hipGetLastError());
        return KHR_OK;
      });
      if (rc) return rc;
    }
  }
  c->seg_stats = s;
  c->seg_valid = true;
  c->seg_listed = list;
  if (stats) *stats = s;
  return KHR_OK;
}

int khr_segment_map_into(khr_ctx* c, int on_device, int32_t* comp_label, uint64_t* comp_n_voxels, int32_t* comp_bbox_min, int32_t* comp_bbox_max,
                         int64_t* comp_sum, int32_t* comp_representative, uint64_t* comp_last_observed, uint64_t* comp_first, int32_t* voxels,
                         uint32_t* voxel_component) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (!c->seg_valid) return fail(KHR_ESTATE, "no successful khr_segment_map before khr_segment_map_into");
  if ((voxels || voxel_component) && !c->seg_listed)
    return fail(KHR_ESTATE, "khr_segment_map_into: the last khr_segment_map ran with want_voxels = 0 and holds no voxel list");
  const khr_segment_stats& s = c->seg_stats;
  if (s.n_components == 0) return KHR_OK;
  HIP_TRY(hipSetDevice(c->device));
  const hipMemcpyKind dir = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t m = s.n_components, n = c->seg_listed ? s.n_voxels : 0;
  const SegLayout L = segLayout(m, n);
  const uint8_t* const ob = c->d_seg_out;
  hipError_t e = hipSuccess;
  auto field = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && dst && bytes) e = hipMemcpyAsync(dst, src, bytes, dir, c->stream);
  };
  field(comp_label, ob + L.label, 4 * m);
  field(comp_n_voxels, ob + L.n_voxels, 8 * m);
  field(comp_bbox_min, ob + L.bbox_min, 12 * m);
  field(comp_bbox_max, ob + L.bbox_max, 12 * m);
  field(comp_sum, ob + L.sum, 24 * m);
  field(comp_representative, ob + L.representative, 12 * m);
  field(comp_last_observed, ob + L.last_observed, 8 * m);
  field(comp_first, ob + L.first, 8 * m);
  field(voxels, ob + L.voxels, 12 * n);
  field(voxel_component, ob + L.voxel_component, 4 * n);
  if (e != hipSuccess) return fail(KHR_EDEVICE, "khr_segment_map_into: copy failed: %s", hipGetErrorString(e));
  if (!on_device) HIP_TRY(hipStreamSynchronize(c->stream));
  return KHR_OK;
}

int khr_debug_read(khr_ctx* c, unsigned long long* out, int64_t n) {
  if (!c || !out) return fail(KHR_EINVAL, "null argument");
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(out, c->d_dbg, sizeof(unsigned long long) * std::min<int64_t>(n, 4096 * 4 * 12), hipMemcpyDeviceToHost));
  return KHR_OK;
}

int khr_debug_live_resources(int64_t out[4]) {
  if (!out) return fail(KHR_EINVAL, "null argument");
  for (int k = 0; k < 4; ++k) out[k] = g_live[k].load(std::memory_order_relaxed);
  return KHR_OK;
}

int khr_timing_enable(khr_ctx* c, int enable) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  if (enable && !c->timing) {
    // what the first timed launches would otherwise do inside the caller's measurement: create their events (a signal each) and switch
    // the stream's hardware queue to time-stamped dispatches -- the first hipExtLaunchKernelGGL with events on a queue can stall it
    // for milliseconds (round 6: one run of the driver's command in twenty had a 2.7 ms wait for the seed count in its second step)
    HIP_TRY(hipSetDevice(c->device));
    while (c->event_pool.size() < 256) {
      Event e;
      KHR_TRY(e.ensure(hipEventDefault));
      c->event_pool.push_back(std::move(e));
    }
    Event a = takeEvent(c), b = takeEvent(c);
    hipExtLaunchKernelGGL(k_copy_words, dim3(1), dim3(64), 0, c->stream, a, b, 0, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventSynchronize(b));
    c->event_pool.push_back(std::move(a));
    c->event_pool.push_back(std::move(b));
  }
  c->timing = static_cast<uint32_t>(enable);
  return KHR_OK;
}
int khr_timing_reset(khr_ctx* c) {
  if (!c) return fail(KHR_EINVAL, "null ctx");
  resolveTimers(c);
  for (int i = 0; i < kNumTimers; ++i) { c->t_ms[i] = 0; c->t_n[i] = 0; }
  return KHR_OK;
}
int khr_timing_get(khr_ctx* c, int which, double* total_ms, uint64_t* launches) {
  if (!c || which < 0 || which >= kNumTimers) return fail(KHR_EINVAL, "bad timer");
  resolveTimers(c);
  if (total_ms) *total_ms = c->t_ms[which];
  if (launches) *launches = c->t_n[which];
  return KHR_OK;
}

}  // extern "C"
