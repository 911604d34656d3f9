"""The object detector's per-frame device chain with the tracker's voxel sets collected by the id-remap pass
(khr_configure_object_voxel_sets): every case against the
oracle (ora.detect_objects / ora.cluster_voxels) AND against a second context that never configures the voxel sets, which
takes the stand-alone k_obj_remap_tab + k_cluster_voxels path.  Integer results bit-exact, centroids to 1e-4.

Frames are 80 x 48 pixels (2.5 x 1.5 paint tiles of 32 x 32: partial tiles in both directions), plus 320 x 240 frames of the
synthetic stream."""
import numpy as np
import pytest

from common import DeviceArray, make_pair

pytestmark = pytest.mark.gpu

W, H = 80, 48
OBJS = [2, 3, 4, 6] + list(range(7, 20))
DET = dict(use_3d=True, grid_size=0.1, max_range=0.0, min_cluster_size=0)


def _pair(width=W, height=H, **kw):
    """(context with the voxel sets configured later by the test, plain context, oracle, stream, sensors)"""
    cfg, ctx, ora, s, sen, osen = make_pair(width, height, seed=77, **kw)
    _, ref, ora2, _, _, _ = make_pair(width, height, seed=77, **kw)
    ora2.close()
    return ctx, ref, ora, s, sen, osen


def _hand_frame(s, i=0):
    """four object rectangles at their own depths in front of a non-object wall; they straddle the tile borders at 32 / 64"""
    fr = dict(s.render(i))
    depth = np.full((H, W), 3.0, np.float32)
    label = np.ones((H, W), np.int32)
    for r0, r1, c0, c1, lab, d in ((4, 20, 4, 30, 2, 1.0), (10, 40, 36, 70, 3, 1.5), (30, 46, 8, 28, 4, 2.0), (2, 8, 50, 78, 6, 2.5)):
        label[r0:r1, c0:c1] = lab
        depth[r0:r1, c0:c1] = d
    fr["depth"], fr["label"] = depth, label
    fr["rgb"] = np.ascontiguousarray(fr["rgb"])
    return fr


def _same_clusters(cl_g, cl_o):
    assert len(cl_g) == len(cl_o)
    for g, o in zip(cl_g, cl_o):
        assert g["id"] == o["id"] and g["semantic_id"] == o["semantic_id"] and g["num_pixels"] == o["num_pixels"]
        assert (g["bbox_min"] == o["bbox_min"]).all() and (g["bbox_max"] == o["bbox_max"]).all()
        assert np.allclose(g["centroid"], o["centroid"], rtol=1e-4, atol=1e-4)


def _detect(ctxs, ora, sen, osen, fr, det, label=True):
    """detection on every context and on the oracle; returns the slots, the cluster count and the oracle's object image"""
    lab = fr["label"] if label else None
    if label:
        no, img_o, cl_o = ora.detect_objects(osen, fr["stamp"], fr["pose"], fr["depth"], fr["label"], OBJS, **det)
    else:
        no, img_o, cl_o = 0, np.zeros(fr["depth"].shape, np.int32), []
    slots = []
    for c in ctxs:
        slot = c.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], lab)
        c.configure_object_detector(OBJS, **det)
        assert c.detect_objects(slot) == no
        assert np.array_equal(c.download_frame(slot, fr["depth"].shape, range_image=False, object_image=True)[3], img_o)
        _same_clusters(c.semantic_clusters(slot), cl_o)
        slots.append(slot)
    return slots, no, img_o


def _voxels_two_halves(c, slot, vs):
    c.cluster_voxels_launch(slot, 1, vs)
    return c.cluster_voxels_fetch(1)


def _check_sets(got, want):
    assert len(got[0]) == len(want[0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("vs", [0.2, 0.05])
def test_prequeued_voxel_sets(vs):
    ctx, ref, ora, s, sen, osen = _pair()
    ctx.configure_object_voxel_sets(vs)
    fr = _hand_frame(s)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, DET)
    assert n >= 3
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, vs)
    assert len(want[0]) > n
    _check_sets(_voxels_two_halves(ctx, slot, vs), want)
    _check_sets(_voxels_two_halves(ref, rslot, vs), want)
    # the same request again (nothing is queued ahead any more): the stand-alone pass on the configured context
    _check_sets(_voxels_two_halves(ctx, slot, vs), want)
    _check_sets(ctx.cluster_voxels(slot, 1, vs), want)
    # the object image still holds the final ids
    assert np.array_equal(ctx.download_frame(slot, (H, W), range_image=False, object_image=True)[3], img_o)
    # the size filter drops clusters AFTER the provisional ids were painted: ids remapped to 0 carry no voxels
    det = dict(DET, min_cluster_size=200)
    (slot, rslot), n2, img_o = _detect((ctx, ref), ora, sen, osen, fr, det)
    assert 1 <= n2 < n
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, vs)
    _check_sets(_voxels_two_halves(ctx, slot, vs), want)
    _check_sets(_voxels_two_halves(ref, rslot, vs), want)
    for c in (ctx, ref):
        c.close()


def test_size_mismatch_runs_the_stand_alone_pass():
    ctx, ref, ora, s, sen, osen = _pair()
    ctx.configure_object_voxel_sets(0.2)
    fr = _hand_frame(s)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, DET)
    assert n >= 3
    for vs in (0.05, 0.2, 0.1):  # another size; then the configured one, still queued ahead; then another one again
        want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, vs)
        assert len(want[0]) > n
        _check_sets(_voxels_two_halves(ctx, slot, vs), want)
        _check_sets(_voxels_two_halves(ref, rslot, vs), want)
    # another slot than the one the detector ran on last
    fr2 = _hand_frame(s, 1)
    fr2["depth"] = fr2["depth"] + np.float32(0.25)
    (slot2, _), n2, img_o2 = _detect((ctx, ref), ora, sen, osen, fr2, DET)
    assert slot2 != slot and n2 >= 3
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2))
    _check_sets(_voxels_two_halves(ctx, slot2, 0.2), ora.cluster_voxels(osen, fr2["stamp"], fr2["pose"], fr2["depth"], img_o2, 0.2))
    # switched off again: as if never configured
    ctx.configure_object_voxel_sets(0.0)
    (slot3, _), n3, img_o3 = _detect((ctx, ref), ora, sen, osen, fr, DET)
    _check_sets(_voxels_two_halves(ctx, slot3, 0.2), ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o3, 0.2))
    with pytest.raises(Exception):
        ctx.configure_object_voxel_sets(-1.0)
    for c in (ctx, ref):
        c.close()


def test_dynamic_image_request_in_between():
    """a which = 0 request between the detection and the which = 1 fetch uses the same (group, voxel) table"""
    ctx, ref, ora, s, sen, osen = _pair()
    ctx.configure_object_voxel_sets(0.2)
    fr = _hand_frame(s)
    dyn = np.zeros((H, W), np.int32)
    dyn[5:25, 20:60] = 1
    dyn[28:44, 40:79] = 2
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, DET)
    assert n >= 3
    want0 = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], dyn, 0.2)
    want1 = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2)
    assert len(want0[0]) > 2 and len(want1[0]) > n
    for c, sl in ((ctx, slot), (ref, rslot)):
        c.set_frame_image(sl, 0, dyn)
        _check_sets(c.cluster_voxels(sl, 0, 0.2), want0)
        c.cluster_voxels_launch(sl, 1, 0.2)
        c.cluster_voxels_launch(sl, 0, 0.2)
        _check_sets(c.cluster_voxels_fetch(1), want1)
        _check_sets(c.cluster_voxels_fetch(0), want0)
    for c in (ctx, ref):
        c.close()


def test_more_components_than_the_remap_table():
    """a fine checkerboard of two object labels on a 3 cm grid: every pixel is its own component (neighbouring pixels are 5 cm
    apart at 3 m), more than 256 of them reach the host and the ids are remapped from the table in device memory"""
    ctx, ref, ora, s, sen, osen = _pair()
    ctx.configure_object_voxel_sets(0.2)
    fr = _hand_frame(s)
    depth = np.full((H, W), 3.0, np.float32)
    label = np.ones((H, W), np.int32)
    rr, cc = np.mgrid[0:H, 0:W]
    board = (rr >= 8) & (rr < 40) & (cc >= 20) & (cc < 60)
    label[board] = np.where((rr + cc) % 2 == 0, 2, 3)[board]
    fr["depth"], fr["label"] = depth, label
    det = dict(DET, grid_size=0.03)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, det)
    assert n > 256
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2)
    assert len(want[0]) >= n
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    _check_sets(_voxels_two_halves(ref, rslot, 0.2), want)
    # and a frame with few components right behind it on the same contexts
    fr2 = _hand_frame(s)
    (slot, rslot), n2, img_o = _detect((ctx, ref), ora, sen, osen, fr2, DET)
    assert 3 <= n2 <= 256
    want = ora.cluster_voxels(osen, fr2["stamp"], fr2["pose"], fr2["depth"], img_o, 0.2)
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    _check_sets(_voxels_two_halves(ref, rslot, 0.2), want)
    for c in (ctx, ref):
        c.close()


def test_zero_clusters_and_no_label_image():
    ctx, ref, ora, s, sen, osen = _pair()
    ctx.configure_object_voxel_sets(0.2)
    fr = _hand_frame(s)
    fr0 = dict(fr)
    fr0["label"] = np.ones((H, W), np.int32)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr0, DET)
    assert n == 0 and not img_o.any()
    for c, sl in ((ctx, slot), (ref, rslot)):
        ids, vox = _voxels_two_halves(c, sl, 0.2)
        assert len(ids) == 0
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, DET, label=False)
    assert n == 0
    for c, sl in ((ctx, slot), (ref, rslot)):
        ids, vox = _voxels_two_halves(c, sl, 0.2)
        assert len(ids) == 0
    # every component filtered out: the remap pass runs and writes zeros, no voxel is collected
    det = dict(DET, min_cluster_size=100000)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, det)
    assert n == 0 and not img_o.any()
    for c, sl in ((ctx, slot), (ref, rslot)):
        assert len(_voxels_two_halves(c, sl, 0.2)[0]) == 0
    # a frame with clusters afterwards: the table and the counters were left clean
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, DET)
    assert n >= 3
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2)
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    _check_sets(_voxels_two_halves(ref, rslot, 0.2), want)
    for c in (ctx, ref):
        c.close()


def test_origin_voxel_and_far_pose():
    ctx, ref, ora, s, sen, osen = _pair()
    ctx.configure_object_voxel_sets(0.2)
    # object pixels with depth 0 and NaN: vertex (0, 0, 0), one voxel at the world origin per cluster
    fr = _hand_frame(s)
    d = fr["depth"].copy()
    d[6:12, 6:26] = 0.0
    d[14:20, 40:66] = np.nan
    fr["depth"] = d
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, DET)
    assert n >= 3
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2)
    assert (want[1] == 0).all(axis=1).any()
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    _check_sets(_voxels_two_halves(ref, rslot, 0.2), want)
    # far from the world origin: the window follows the sensor, the origin voxel lies outside it
    fr2 = dict(fr)
    T = fr["pose"].copy()
    T[:3, 3] += np.array([5000.0, -7000.0, 300.0])
    fr2["pose"] = T
    d = _hand_frame(s)["depth"]
    d[6:12, 6:26] = 0.0
    fr2["depth"] = d
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr2, DET)
    assert n >= 3
    want = ora.cluster_voxels(osen, fr2["stamp"], fr2["pose"], fr2["depth"], img_o, 0.2)
    assert len(want[0]) > n
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    _check_sets(_voxels_two_halves(ref, rslot, 0.2), want)
    for c in (ctx, ref):
        c.close()


def test_2d_mode_and_stream_frame():
    """2D mode (no (group, voxel) table in the detector, k_publish at its end); and one 320 x 240 frame of the stream"""
    ctx, ref, ora, s, sen, osen = _pair()
    ctx.configure_object_voxel_sets(0.2)
    fr = _hand_frame(s)
    det = dict(use_3d=False, min_cluster_size=0)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, det)
    assert n >= 3
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2)
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    _check_sets(_voxels_two_halves(ref, rslot, 0.2), want)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, DET)  # 3D right behind it
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2)
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    for c in (ctx, ref):
        c.close()
    ctx, ref, ora, s, sen, osen = _pair(320, 240)
    ctx.configure_object_voxel_sets(0.2)
    fr = s.render(40)
    det = dict(use_3d=True, grid_size=0.1, max_range=4.5, min_cluster_size=20)
    (slot, rslot), n, img_o = _detect((ctx, ref), ora, sen, osen, fr, det)
    assert n >= 3
    want = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, 0.2)
    assert len(want[0]) > n
    _check_sets(_voxels_two_halves(ctx, slot, 0.2), want)
    _check_sets(_voxels_two_halves(ref, rslot, 0.2), want)
    for c in (ctx, ref):
        c.close()


@pytest.mark.parametrize("ahead", [False, True])
def test_table_reuse_over_consecutive_frames(ahead):
    """five frames through khr_process_frame(OBJECTS | MOTION | TRACKING): the (group, voxel) table goes from the detector to
    the voxel sets and back every frame; with khr_ingest_ahead the NEXT frame's detector kernels are queued before this frame's
    voxel sets are asked for.  The tracker's order of calls: the fetch of a frame comes after the next frame's khr_process_frame."""
    ctx, ref, ora, s, sen, osen = _pair(320, 240, temporal_window=0.75, num_frame_slots=5)
    det = dict(use_3d=True, grid_size=0.1, max_range=4.5, min_cluster_size=20)
    for c in (ctx, ref):
        c.configure_object_detector(OBJS, **det)
    ctx.configure_object_voxel_sets(0.2)
    held = []
    N = 5
    frames = [s.render(20 + i) for i in range(N)]

    def device_frame(c, fr):
        f = c.make_frame(fr["stamp"], fr["pose"], 0)
        dev = [DeviceArray(np.ascontiguousarray(fr[k])) for k in ("depth", "rgb", "label")]
        held.append(dev)
        f.depth, f.color, f.label = (d.data_ptr() for d in dev)
        return f

    total = 0
    for c in (ctx, ref):
        base = c.PF_INPUT_READY | c.PF_MOTION | c.PF_OBJECTS | c.PF_TRACKING
        handed = {}
        pending = None  # (frame index, oracle image): voxel sets launched, fetch outstanding
        for i, fr in enumerate(frames):
            flags = base
            if i in handed:
                f = handed.pop(i)
                flags |= c.PF_INGESTED
            else:
                f = device_frame(c, fr)
            slot, _ = c.process_frame(sen, f, on_device=True, flags=flags)
            if ahead and i + 1 < N:
                nf = device_frame(c, frames[i + 1])
                assert c.ingest_ahead(sen, nf) is not None
                handed[i + 1] = nf
            no, img_o, cl_o = ora.detect_objects(osen, fr["stamp"], fr["pose"], fr["depth"], fr["label"], OBJS, **det)
            assert no >= 3
            total += no
            if pending is not None:  # the previous frame's sets, behind this frame's detection (the tracker's software pipeline)
                j, img_j = pending
                pj = frames[j]
                _check_sets(c.cluster_voxels_fetch(1), ora.cluster_voxels(osen, pj["stamp"], pj["pose"], pj["depth"], img_j, 0.2))
            assert np.array_equal(c.download_frame(slot, fr["depth"].shape, range_image=False, object_image=True)[3], img_o)
            _same_clusters(c.semantic_clusters(slot), cl_o)
            c.cluster_voxels_launch(slot, 1, 0.2)
            pending = (i, img_o)
        j, img_j = pending
        pj = frames[j]
        _check_sets(c.cluster_voxels_fetch(1), ora.cluster_voxels(osen, pj["stamp"], pj["pose"], pj["depth"], img_j, 0.2))
        c.sync()
    assert total >= 30
    for c in (ctx, ref):
        c.close()
    for dev in held:
        for d in dev:
            d.free()
