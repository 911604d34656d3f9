"""Every HIP resource of a context, snapshot, frame copy or ray verificator has an owner (khronos_amd/csrc/khr_owned.h), and the
owners count what they hold (khr_debug_live_resources: device buffers, page-locked blocks, events, streams, process-wide).  Each
case reads the four counts, does its work, destroys what it made and finds the counts where they were -- compared with its OWN
starting counts, since fixtures of other tests may be alive -- and, so that a count that never moves cannot pass, sees them higher
while its objects lived.

What the counts can and cannot see: they move only where an owner allocates or releases.  A block that an owner allocated and
nobody releases (an owner that is never destroyed, a pool that is never emptied) leaves a count above its start and fails these
cases; a raw hipHostMalloc kept in a raw member passes them unseen.  tests/test_cpu_owned.py closes that side by reading: outside
khr_owned.h no code of csrc/ calls the runtime's allocate / create / free / destroy functions."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import DeviceArray, PinnedArray, compact_mesh_halo_exchange, record_mesh_halo_exchange
from khronos_amd import FusionContext, RayVerificator, default_config
from khronos_amd.capi import live_resources
from khronos_amd.synth import SyntheticStream

pytestmark = pytest.mark.gpu

W, H = 64, 48
NAMES = ("device buffers", "page-locked blocks", "events", "streams")


def make_cfg(vps=16, **kw):
    base = dict(voxel_size=0.1, truncation_distance=0.3, voxels_per_side=vps, with_semantics=1, with_tracking=1, num_labels=4, max_blocks=512,
                max_frame_pixels=W * H, num_frame_slots=4, temporal_window=0.35, md_min_cluster_size=5, md_min_separation_distance=2.0,
                md_max_range=5.0)
    base.update(kw)
    return default_config(**base)


def stream():
    return SyntheticStream(W, H)


def render(s, i):
    fr = s.render(i)
    fr["label"] = np.ascontiguousarray(fr["label"] % 4)  # (the maps here hold 4 labels)
    return fr


def sensor(ctx, s):
    return ctx.make_sensor(W, H, s.fx, s.fy, s.cx, s.cy)


def begin():
    """the counts a case starts from (contexts that earlier tests dropped without closing are collected first, not in the middle)"""
    gc.collect()
    return live_resources()


def assert_back(start, what):
    now = live_resources()
    assert now == start, "%s: live %s went from %s to %s" % (what, NAMES, start, now)


def assert_above(start, what, kinds=(0, 1, 2, 3)):
    now = live_resources()
    assert all(now[k] > start[k] for k in kinds) and all(a >= b for a, b in zip(now, start)), "%s: %s -> %s" % (what, start, now)


@pytest.mark.parametrize("vps", [16, 8])
def test_create_destroy_cycles_leave_nothing(vps):
    start = begin()
    for i in range(20):
        ctx = FusionContext(make_cfg(vps))
        if i == 0:
            assert_above(start, "a bare context")
            one = live_resources()
        else:
            assert live_resources() == one, "context %d holds something the first did not" % i
        ctx.close()
        assert_back(start, "create / destroy cycle %d at %d^3" % (i, vps))


def _pinned_frame(ctx, fr, held):
    arrs = [PinnedArray(np.ascontiguousarray(fr[k])) for k in ("depth", "rgb", "label")]
    held.append(arrs)
    f = ctx.make_frame(fr["stamp"], fr["pose"], 0)
    f.depth, f.color, f.label = (a.data_ptr() for a in arrs)
    return f


def _frame_copy(ctx, slot):
    fc = C.c_void_p()
    ctx._chk(ctx.lib.khr_frame_copy_create(ctx.h, int(slot), C.byref(fc)))
    return fc


def _frame_copy_depth(ctx, fc):
    depth = np.zeros((H, W), np.float32)
    ctx.lib.khr_frame_copy_download.argtypes = [C.c_void_p] * 6
    ctx._chk(ctx.lib.khr_frame_copy_download(fc, depth.ctypes.data, None, None, None, None))
    return depth


def _frame_copy_release(ctx, fc):
    ctx.lib.khr_frame_copy_release.argtypes = [C.c_void_p]
    ctx.lib.khr_frame_copy_release.restype = None
    ctx.lib.khr_frame_copy_release(fc)


def test_window_context_first_use_and_growth_sites(monkeypatch):
    start = begin()
    s = stream()
    held = []
    ctx = FusionContext(make_cfg())
    sen = sensor(ctx, s)
    bare = live_resources()
    ctx.timing_enable(True)  # (the pool of timing events)
    assert live_resources()[2] > bare[2]
    # three frames through khr_process_frame: output + snapshot, page-locked input, the next frame handed over ahead
    ctx.configure_object_detector([1, 2, 3], use_3d=True, grid_size=0.1, max_range=5.0, min_cluster_size=5)
    base = ctx.PF_MOTION | ctx.PF_TRACKING | ctx.PF_INPUT_READY | ctx.PF_INPUT_PINNED | ctx.PF_OBJECTS
    frames = [render(s, i) for i in range(3)]
    f0 = _pinned_frame(ctx, frames[0], held)
    slot0, _ = ctx.process_frame(sen, f0, on_device=False, flags=base)
    f1 = _pinned_frame(ctx, frames[1], held)
    assert ctx.ingest_ahead_host(sen, f1) is not None
    slot1, _ = ctx.process_frame(sen, f1, on_device=False, flags=base | ctx.PF_INGESTED)
    f2 = _pinned_frame(ctx, frames[2], held)
    slot2, _ = ctx.process_frame(sen, f2, on_device=False, flags=base | ctx.PF_OUTPUT | ctx.PF_SNAPSHOT)
    snap = ctx.take_snapshot()
    assert snap is not None and snap.num_blocks() > 0
    ctx.last_removed()
    # the object detector, both voxel-set requests, khr_pixel_iou and khr_forward_instances
    n_obj = ctx.detect_objects(slot2)
    ctx.cluster_voxels(slot2, 0, 0.2)
    ctx.cluster_voxels(slot2, 1, 0.2)
    ctx.pixel_iou(slot2, [(slot1, 1, 1)], max(n_obj, 1))
    ctx.forward_instances(slot2, max_range=5.0, background_ids=(0,), max_id=3)
    # asynchronous snapshot download (the copy stream), then the snapshot goes back to the pool
    n = snap.num_blocks()
    dist = np.zeros((n, ctx.nvox), np.float32)
    idx = np.zeros((n, 3), np.int32)
    snap.download_begin([idx.ctypes.data, dist.ctypes.data, 0, 0, 0, 0, 0], n)
    assert snap.download_end() == n
    snap.release()
    # mesh staging, a mesh fetch, a frame copy
    ctx.reserve_mesh_staging(200000)
    mesh = ctx.fetch_mesh()
    assert len(mesh["points"]) > 0
    fc = _frame_copy(ctx, slot2)
    assert (_frame_copy_depth(ctx, fc) > 0).any()
    _frame_copy_release(ctx, fc)
    # a tick ingest
    fr3 = render(s, 3)
    dev = [DeviceArray(fr3[k]) for k in ("depth", "rgb", "label")]
    tick_slots, _ = ctx.tick_ingest(sen, [ctx.make_frame(fr3["stamp"], fr3["pose"], *(d.data_ptr() for d in dev))], count_seeds=True)
    ctx.tick_integrate(tick_slots, phases=3)
    ctx.update_tracking(fr3["stamp"])
    ctx.sync()
    # a slice; the host forms of the three map readers, twice each, the second time larger so that their staging grows
    ctx.map_slice(int(ctx.block_indices()[0][2]) * 16 + 8)
    small = ctx.make_sensor(W // 2, H // 2, s.fx / 2, s.fy / 2, s.cx / 2, s.cy / 2)
    pts = np.random.default_rng(0).uniform(-2, 2, (4000, 3)).astype(np.float32)
    after = []
    for sn, k in ((small, 100), (sen, 4000)):
        ctx.render_view(sn, frames[2]["pose"])
        ctx.query_points(pts[:k])
        ctx.align_linearize(np.eye(4), points=pts[:k])
        after.append(live_resources())
    assert after[1] == after[0], "a staging pair that grows frees what it replaces"
    # a checkpoint through pageable memory, out and back in
    blob = ctx.save_map()
    other = FusionContext(make_cfg())
    assert other.load_map(blob) == ctx.num_blocks()
    other.close()
    # a remote halo and both mesh-halo forms need a second rank: two shards of the same frames
    shards = [FusionContext(make_cfg(rank=r, world_size=2)) for r in range(2)]
    for fr in frames:
        for c in shards:
            c.integrate(c.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"]))
            c.update_tracking_phase(fr["stamp"], 1)
        recs = np.concatenate([c.export_halo(512) for c in shards])
        for c in shards:
            c.import_halo(recs)
            c.update_tracking_phase(fr["stamp"], 2)
    record_mesh_halo_exchange(shards, only_mesh_updated=False)
    for c in shards:
        c.generate_mesh(False, False)
    _, bufs = compact_mesh_halo_exchange(shards, only_mesh_updated=False)
    for c in shards:
        c.generate_mesh(False, False)
        c.close()
    for d in [bufs[0]] + bufs[1] + bufs[2]:
        d.free()
    # a block list of more than 64 KB (the page-locked upload block grows; the pool of 512 blocks takes what fits)
    bl = np.array([[x, y, z] for x in range(40, 60) for y in range(20) for z in range(15)], np.int32)
    assert bl.nbytes > (1 << 16)
    ctx.allocate_blocks(bl)
    ctx.sync()
    assert_above(start, "the window context at work")
    assert all(a >= b for a, b in zip(live_resources(), bare))
    ctx.close()
    for d in dev:
        d.free()
    for arrs in held:
        for a in arrs:
            a.free()
    assert_back(start, "the window context")
    # a seed frame whose clusters are walked on the host (KHR_MD_HOST_WALK is read when the context is created)
    monkeypatch.setenv("KHR_MD_HOST_WALK", "1")
    ctx = FusionContext(make_cfg())
    walks = 0
    for i in range(24):
        fr = render(s, i)
        f = ctx.make_frame(fr["stamp"], fr["pose"], fr["depth"].ctypes.data, fr["rgb"].ctypes.data, fr["label"].ctypes.data)
        ctx.process_frame(sen, f, on_device=False, flags=ctx.PF_MOTION | ctx.PF_TRACKING)
        walks = ctx.stats()["n_md_host_walks"]
        if walks:
            break
    assert walks > 0, "no frame of the stream had motion seeds"
    ctx.close()
    assert_back(start, "the host-walk context")


def test_object_mini_map():
    start = begin()
    s = stream()
    win = FusionContext(make_cfg())
    sen = sensor(win, s)
    mini = FusionContext(make_cfg(8, with_tracking=0))
    assert_above(start, "window + mini-map")
    slots = []
    for i in range(3):
        fr = render(s, i)
        slot = win.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        win._chk(win.lib.khr_retain_slot(win.h, slot))
        win.integrate(slot)
        slots.append(slot)
    win.sync()
    mini._chk(mini.lib.khr_depend_on(mini.h, win.h))
    # the mini-map's blocks (0.8 m) where the window has surface: the eight children of its first 40 blocks (1.6 m)
    kids = np.array([[2 * b[0] + i, 2 * b[1] + j, 2 * b[2] + k] for b in win.block_indices()[:40].tolist()
                     for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.int32)
    mini.allocate_blocks(kids)
    mini.integrate_shared_batch(win, slots)
    mini.object_prune(0.5, 2.0)
    mini.sync()
    assert mini.stats()["cum_updated_voxels"] > 0
    mini.close()
    win.close()
    assert_back(start, "window + mini-map")


def test_snapshot_and_frame_copy_outlive_their_context():
    start = begin()
    s = stream()
    ctx = FusionContext(make_cfg())
    sen = sensor(ctx, s)
    fr = render(s, 0)
    slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
    ctx.integrate(slot)
    ctx.update_tracking(fr["stamp"])
    snap = ctx.snapshot_updated()
    assert snap.num_blocks() > 0
    fc = _frame_copy(ctx, slot)
    ctx.sync()
    lib = ctx.lib
    ctx.close()
    held = live_resources()
    # the snapshot's arena (a device block, its page-locked count word, its event) and the copy's block and event are still there
    assert held[0] >= start[0] + 2 and held[1] >= start[1] + 1 and held[2] >= start[2] + 2 and held[3] == start[3], (start, held)
    assert (_frame_copy_depth(ctx, fc) > 0).any()
    _frame_copy_release(ctx, fc)
    mid = live_resources()
    assert mid[0] == held[0] - 1 and mid[2] == held[2] - 1 and mid[0] > start[0] and mid[1] > start[1], (held, mid)
    lib.khr_snapshot_release(snap.h)
    snap.h = None
    assert_back(start, "snapshot and frame copy released after khr_destroy")


def test_ray_verificator():
    start = begin()
    rv = RayVerificator(block_size=1.0)
    assert_above(start, "khr_rv_create", kinds=(3,))
    rng = np.random.default_rng(1)
    n = 300
    src = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    tgt = (src + rng.uniform(-4, 4, (n, 3))).astype(np.float32)
    rv.add_rays(np.arange(n, dtype=np.uint64) + 1, src, tgt)
    assert rv.num_rays() == n and rv.num_pairs() > n
    rv.check(tgt[:100], np.zeros(100, np.uint64), np.full(100, 10 ** 6, np.uint64))
    assert_above(start, "a ray verificator with an index", kinds=(0, 3))
    rv.close()
    assert_back(start, "khr_rv_create / khr_rv_destroy")
