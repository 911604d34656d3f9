"""-m gpu: the cases of tests/update_cases.py on the device, through every update path that accepts their configuration.  Every run
is compared with a fresh OracleMap through common.compare_maps and common.assert_digests_equal: exact arithmetic, every layer bit for
bit.  The generic case runs once more in relaxed arithmetic under compare_maps' TOL and borderline bound.
tests/test_cpu_update_cases.py shows on the CPU that every case is what it claims to be.

  path     entry points                                          kernel
  slot     upload_frame, integrate(allocate_blocks=False)        k_fuse<16 | 8, .., DEFCFG or not, ..> on explicitly allocated blocks
  tick     tick_ingest, tick_integrate (2 - 3 cameras a tick)    k_fuse2<16, ..> / k_fuse2<8, ..>; k_fuse per camera for non-default switches
  batch    integrate_shared_batch from a window context, 8^3     k_fuse_obj (binary object layer, no tracking), k_fuse2<8, 4, ..> (labels);
                                                                 k_fuse per frame for non-default switches
The tick and the batch must also equal the same frames sent one by one (integrate / integrate_shared): bit for bit.  A switch that
k_fuse2 and k_fuse_obj hard-code and that the host's guards (multiApplies, tickUnion) let through would show as a mismatch with the
oracle here: tests/test_cpu_update_cases.py shows that every switch setting changes the map.

The band phase of a label case, by label count K (khr_device.h: likStride; khr_kernels_fuse.h: fuseBandRowsOk, fuseBandRowLanesOk,
fuseBandRows; khronos_amd.hip: fillFuseMap):
  K              floats per row KS   band form with max_frame_pixels > 640 x 480          lanes per record   passes per 64 records
  1, 2, 3, 4     K                   records (fuseBandRecord; scalar loop for K & 3 != 0)  --                 --
  5 .. 32        32                  rows                                                  8                  8  (one round of kRowPasses)
  33 .. 64       64                  rows                                                  16                 16 (two rounds)
  65 .. 96       96                  records: 24 lanes do not divide a wave                --                 --
  97 .. 128      128                 rows                                                  32                 32 (four rounds)
  129 .. 224     160, 192, 224       records                                               --                 --
  225 .. 256     256                 rows                                                  64                 64 (eight rounds)
  257 ..         288 ..              records (rows longer than a wave)                     --                 --
Up to 640 x 480 pixels of frame capacity, and with packed_likelihood_rows (KS = K), every K takes the record form.  Each label case
runs in all three settings; the three maps must be equal.

(Why rows of 96, 160, 192 and 224 floats take the record form: DESIGN.md, section 3.)"""
import pytest

import common
import update_cases as uc
from common import DeviceArray
from khronos_amd import FusionContext, default_config

pytestmark = pytest.mark.gpu
BIG_FRAMES = 640 * 480 + 1      # frame capacity above which fillFuseMap chooses the row form of the band phase
_CONTEXTS = {}


def context(kw, tag=""):
    """one context per configuration, emptied (khr_reset_map) before every use; the oldest are closed when there are many"""
    key = (tag,) + tuple(sorted(kw.items()))
    ctx = _CONTEXTS.pop(key, None)
    if ctx is None:
        ctx = FusionContext(default_config(**kw))
        while len(_CONTEXTS) >= 24:
            _CONTEXTS.pop(next(iter(_CONTEXTS))).close()
    else:
        ctx.reset_map(uc.VS, uc.TRUNC)
    _CONTEXTS[key] = ctx
    return ctx


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    while _CONTEXTS:
        _CONTEXTS.popitem()[1].close()


def sensor(ctx, case):
    return ctx.make_sensor(*case["size"], *case["intr"], *case["ranges"])


def binary(kw):
    return kw.get("semantic_mode", 0) == 1


def paint(ctx, slot, case, f, kw):
    if case["use_mask"] and f["dyn"] is not None:
        ctx.set_frame_image(slot, 0, f["dyn"])
    if binary(kw):
        ctx.set_frame_image(slot, 1, uc.object_image(f))


def check(ctx, case, kw, exact=True, stats=None, **oracle_kw):
    """the context against a fresh oracle run of the case; returns the context's digest"""
    ora, ostats, _ = uc.run_oracle(case, kw, **oracle_kw)
    try:
        common.compare_maps(ctx, ora, exact=exact, max_blocks=48)
        if stats:
            s = ctx.stats()
            assert s["pool_exhausted"] == 0
            for k in ("updated_voxels", "band_voxels"):
                assert s["cum_" + k] == sum(st["n_" + k] for st in ostats), (case["name"], k)
            assert s["cum_updated_voxels"] > 0
    finally:
        ora.close()
    return [int(x) for x in ctx.map_digest()]


def run_slot(case, vps, exact=1, **extra):
    kw = uc.config(case, vps, exact_arithmetic=exact, **extra)
    ctx = context(kw)
    ctx.allocate_blocks(uc.blocks(case, vps))
    sen = sensor(ctx, case)
    for f in case["frames"]:
        slot = ctx.upload_frame(sen, f["stamp"], f["pose"], f["depth"], f["rgb"], f["label"])
        paint(ctx, slot, case, f, kw)
        ctx.integrate(slot, allocate_blocks=False, use_mask=case["use_mask"], object_id=uc.OBJECT_ID if binary(kw) else -1)
        if case["track"]:
            ctx.update_tracking(f["stamp"])
    return check(ctx, case, kw, exact=bool(exact), stats=True)


def run_tick(case, vps, exact=1, **extra):
    """the frames as cameras of ticks of two or three (tick_chunks), one stamp a tick; and the same frames one by one through the
    allocating integrate"""
    kw = uc.config(case, vps, exact_arithmetic=exact, max_blocks=256 if vps == 8 else 64, **extra)   # (the tick allocates the frustum: 188 / 49 blocks at most)
    frames = case["frames"]
    oid = uc.OBJECT_ID if binary(kw) else -1
    stamps = uc.tick_stamps(case)
    ctx, twin = context(kw), context(kw, "twin")
    sen = sensor(ctx, case)
    for k0, k1 in uc.tick_chunks(case):
        chunk = frames[k0:k1]
        assert len(chunk) >= 2, "every tick is a rig: two or three cameras share the union launch"
        dev = [(DeviceArray(f["depth"]), DeviceArray(f["rgb"]), DeviceArray(f["label"])) for f in chunk]
        try:
            slots, _ = ctx.tick_ingest(sen, [ctx.make_frame(stamps[k0], f["pose"], d.data_ptr(), c.data_ptr(), l.data_ptr()) for f, (d, c, l) in zip(chunk, dev)],
                                       count_seeds=False)
            for slot, f in zip(slots, chunk):
                paint(ctx, slot, case, f, kw)
            ctx.tick_integrate(slots, use_mask=case["use_mask"], object_id=oid)
            ctx.sync()
        finally:
            for t3 in dev:
                for t in t3:
                    t.free()
    for k, f in enumerate(frames):
        slot = twin.upload_frame(sen, stamps[k], f["pose"], f["depth"], f["rgb"], f["label"])
        paint(twin, slot, case, f, kw)
        twin.integrate(slot, allocate_blocks=True, use_mask=case["use_mask"], object_id=oid)
    dg = check(ctx, case, kw, exact=bool(exact), allocate=True, stamps=stamps, track=False)
    assert ctx.stats()["pool_exhausted"] == 0
    if exact:
        common.assert_digests_equal(dg, twin.map_digest(), what=(case["name"], "tick against frame by frame"))
    return dg


def run_batch(case, layout=None, exact=1, **extra):
    """8^3 maps: the frames from a window context in one khr_integrate_shared_batch, and one by one through khr_integrate_shared"""
    kw = uc.config(case, 8, layout, exact_arithmetic=exact, **extra)
    W, H = case["size"]
    if uc.default_switches(kw):     # meant for k_fuse2 / k_fuse_obj: multiApplies must not decline the batch for its length
        assert uc.MIN_MULTI_FRAMES <= len(case["frames"]) <= uc.MAX_MULTI_FRAMES, case["name"]
    # (the window converts depth to range at the ingest: it shares the mini-map's range mode, as the extractor's window does)
    win = context(dict(voxel_size=uc.VS, truncation_distance=uc.TRUNC, with_semantics=1, max_blocks=8, max_frame_pixels=W * H, num_frame_slots=10,
                       max_mesh_vertices=1 << 16, range_mode=kw.get("range_mode", 0)), "window")
    sen = sensor(win, case)
    slots = []
    for f in case["frames"]:
        slot = win.upload_frame(sen, f["stamp"], f["pose"], f["depth"], f["rgb"], f["label"])
        win._chk(win.lib.khr_retain_slot(win.h, slot))
        paint(win, slot, case, f, kw)
        slots.append(slot)
    assert len(set(slots)) == len(slots)
    win.sync()
    ids = [uc.OBJECT_ID] * len(slots) if binary(kw) else None
    ctx, twin = context(kw), context(kw, "twin")
    for c in (ctx, twin):
        c.allocate_blocks(uc.blocks(case, 8))
    ctx.integrate_shared_batch(win, slots, ids, use_mask=case["use_mask"])
    for slot in slots:
        twin.integrate_shared(win, slot, use_mask=case["use_mask"], object_id=uc.OBJECT_ID if binary(kw) else -1)
    dg = check(ctx, case, kw, exact=bool(exact), stats=True, track=False)
    common.assert_digests_equal(dg, twin.map_digest(), what=(case["name"], "batch against frame by frame"))   # (both arithmetic modes)
    return dg


def run_all_paths(case, exact=1):
    for vps in uc.vps_of(case):
        run_slot(case, vps, exact)
        run_tick(case, vps, exact)
    run_batch(case, None, exact)
    if not case["cfg"].get("semantic_mode"):
        run_batch(case, uc.OBJECT_LAYOUT, exact)


@pytest.mark.parametrize("name", sorted(uc.EDGE_CASES))
def test_edge_cases(name):
    run_all_paths(uc.EDGE_CASES[name])


@pytest.mark.parametrize("name", sorted(uc.SWITCH_CASES))
def test_switch_cases_and_fallbacks(name):
    """every switch setting through k_fuse (slot), and through the tick and the batch, which must fall back to k_fuse for the settings
    k_fuse2 and k_fuse_obj hard-code; the slot digests differ from the default run's exactly in the stated layers"""
    case = uc.SWITCH_CASES[name]
    run_all_paths(case)
    if name != "default":
        base, dg = run_slot(uc.SWITCH_CASES["default"], 16), run_slot(case, 16)
        assert {n for n, a, b in zip(common.DIGEST_LAYERS, base, dg) if a != b} == case["differs"], name


@pytest.mark.parametrize("exact", [1, 0])
def test_generic_case(exact):
    run_all_paths(uc.GENERIC, exact)


@pytest.mark.parametrize("name", sorted(uc.LABEL_CASES, key=lambda n: (uc.LABEL_CASES[n]["K"], n)))
def test_label_counts_in_the_three_band_forms(name):
    """records (frame capacity of the image), rows where fuseBandRowsOk holds (capacity above 640 x 480), packed rows: each equals the
    oracle, on k_fuse (slot) and on the multi-frame kernel (batch), and the three maps are equal; records and rows on the tick as well"""
    case = uc.LABEL_CASES[name]
    forms = (dict(), dict(max_frame_pixels=BIG_FRAMES), dict(packed_likelihood_rows=1))
    for vps in uc.vps_of(case):
        dg = [run_slot(case, vps, **f) for f in forms]
        assert dg[0] == dg[1] == dg[2], (name, vps)
    dg = [run_batch(case, **f) for f in forms]
    assert dg[0] == dg[1] == dg[2], name
    for vps in uc.vps_of(case):
        assert run_tick(case, vps) == run_tick(case, vps, max_frame_pixels=BIG_FRAMES), (name, vps, "tick")
