"""GPU parity for the object mini-map's multi-frame update (k_fuse_obj: the whole voxel state -- distance, weight, colour, the two
likelihoods, flag byte, label -- stays in registers across the frames of a launch, chunks of kMultiChunk = 7 frames per launch).
Two 8^3 object contexts over the same allocated box: one takes khr_integrate_shared_batch, the other one khr_integrate_shared call
per frame (the single-frame kernel, which test_gpu_parity holds to the oracle).  Everything is compared bit for bit: map digests,
voxel layers, prune counts, mesh arrays, update counters.  A second map configuration (LABEL_MAP: tracking stamps, four labels read
from the label image) is not the extractor's: its batch takes k_fuse2<8, 4, ..> with LDS records and fuseBandRecord.

The box is the part of the scene's back wall (label 3 at pixel (160, 120) of frame 0: the plane y = 3 m) the first frames look at,
324 blocks of 32 cm; the objects in front of it give the object image its misses, the turning camera new voxels in every frame."""
import numpy as np
import pytest

from khronos_amd import FusionContext, default_config
from khronos_amd.synth import SyntheticStream

pytestmark = pytest.mark.gpu

W, H = 320, 240
N_MAX = 15
VOX_SEM_VALID = 8
BOX = np.array([[x, y, z] for x in range(-2, 10) for y in range(8, 11) for z in range(0, 9)], np.int32)


@pytest.fixture(scope="module")
def window():
    """the window context with N_MAX retained frames; object image = 3 where the frame's label is the wall's"""
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, with_semantics=1, with_tracking=1, max_blocks=1024,
                         max_frame_pixels=W * H, num_frame_slots=N_MAX + 2, exact_arithmetic=1)
    win = FusionContext(cfg)
    s = SyntheticStream(W, H)
    sen = win.make_sensor(W, H, s.fx, s.fy, s.cx, s.cy)
    target = int(s.render(0)["label"][120, 160])
    slots = []
    for i in range(N_MAX):
        fr = s.render(i)
        slot = win.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        win._chk(win.lib.khr_retain_slot(win.h, slot))
        win.set_frame_image(slot, 1, (fr["label"] == target).astype(np.int32) * 3)
        slots.append(slot)
    assert len(set(slots)) == N_MAX
    win.sync()
    yield win, slots
    win.close()


OBJECT_MAP = dict(with_tracking=0, semantic_mode=1, num_labels=2)  # the extractor's configuration: the batch takes k_fuse_obj
LABEL_MAP = dict(with_tracking=1, semantic_mode=0, num_labels=4)   # any other 8^3 map: the batch takes k_fuse2<8, 4, ..>


def _mini(exact, blend, layout):
    c = FusionContext(default_config(voxels_per_side=8, voxel_size=0.04, truncation_distance=0.08, with_semantics=1,
                                     max_blocks=512, max_frame_pixels=W * H, exact_arithmetic=exact, color_blend_weight=blend, **layout))
    c.allocate_blocks(BOX)
    return c


LAYERS = ("distance", "weight", "color", "flags", "sem_label", "likelihoods", "last_observed")


def _layers(ctx):
    order = ctx.block_indices()
    order = order[np.lexsort(order.T)]
    bl = [ctx.download_block(idx) for idx in order]
    return {k: np.stack([b[k] for b in bl]) for k in LAYERS}


def _run(win, slots, ids, exact=1, blend=0, use_mask=False, layout=OBJECT_MAP):
    """the batch context against the frame-by-frame one; returns the batch context's digest"""
    a, b = _mini(exact, blend, layout), _mini(exact, blend, layout)
    try:
        a.integrate_shared_batch(win, slots, ids, use_mask=use_mask)
        sem_frames = [i for i in range(len(slots)) if ids is not None and ids[i] >= 0]
        keeps_object = ids is not None and sum(1 for i in ids if i == 3) >= 2  # (3: the id the object image carries)
        valid_first = None
        for i, sl in enumerate(slots):
            b.integrate_shared(win, sl, use_mask=use_mask, object_id=-1 if ids is None else ids[i])
            if sem_frames and i == sem_frames[0]:
                valid_first = (_layers(b)["flags"] & VOX_SEM_VALID) != 0
        da, db = [int(x) for x in a.map_digest()], [int(x) for x in b.map_digest()]
        assert da == db
        la = _layers(a)
        valid = (la["flags"] & VOX_SEM_VALID) != 0
        assert (la["weight"] > 0).any() and (la["color"][..., :3] != 0).any()
        sa, sb = a.stats(), b.stats()
        assert sa["cum_updated_voxels"] == sb["cum_updated_voxels"] > 0
        if layout is LABEL_MAP:
            # the voxel layers themselves, last_observed with them (likelihoods and label where the voxel holds any); labels of the
            # label image and stamps of more than one frame have arrived: a voxel the later frames no longer see keeps its stamp
            lb = _layers(b)
            for k in LAYERS:
                on = valid if k in ("likelihoods", "sem_label") else np.ones_like(valid)
                x, y = (np.moveaxis(l[k], 1, -1) if k == "likelihoods" else l[k] for l in (la, lb))
                assert np.array_equal(x[on], y[on]), k
            assert valid.any() and len(np.unique(la["last_observed"][la["weight"] > 0])) >= 2
            return da
        if len(sem_frames) >= 2:
            # state carried over at least two frames, and voxels whose first label arrived in a later frame of the launch
            assert (la["likelihoods"].sum(axis=1)[valid] >= 2).any()
            assert valid_first.any() and (valid & ~valid_first).any()
        else:
            assert not sem_frames and not valid.any()
        # the mesh of the updated map (every case has a surface), the prune counts, and the mesh of what the prune keeps (nothing where
        # the object layer saw misses only or was never written)
        for pruned in (False, True):
            if pruned:
                assert a.object_prune(0.5, 2.0) == b.object_prune(0.5, 2.0)
            a.generate_mesh(True, False)
            b.generate_mesh(True, False)
            ma, mb = a.download_mesh(), b.download_mesh()
            assert pruned or len(ma["points"]) > 0
            for k in ("points", "colors", "labels"):
                assert np.array_equal(ma[k], mb[k]), k
            if pruned and keeps_object:
                assert len(ma["points"]) > 0
        return da
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("n", [2, 7, 8, 15])
def test_batch_equals_frame_by_frame(window, n, exact, blend):
    """under, at and across kMultiChunk = 7 (8 and 15 end in a one-frame chunk), both arithmetic modes, both blend weights"""
    win, slots = window
    _run(win, slots[:n], [3] * n, exact=exact, blend=blend)


@pytest.mark.parametrize("exact", [1, 0])
def test_label_map_batch_equals_frame_by_frame(window, exact):
    """a map with tracking stamps and four labels, all N_MAX frames (three launches): k_fuse2<8, 4, ..> on the batch path"""
    win, slots = window
    _run(win, slots, None, exact=exact, layout=LABEL_MAP)


def test_frames_without_object_id_in_the_middle(window):
    """do_sem == 0 frames between labelled ones: colour and distance move, likelihoods / label / flag stay as they are"""
    win, slots = window
    _run(win, slots[:8], [3, 3, -1, -1, 3, 3, -1, 3])


def test_object_id_no_pixel_carries(window):
    """the object image holds 0 and 3: id 5 gives misses only (likelihood 0 grows, label stays 0)"""
    win, slots = window
    _run(win, slots[:8], [5] * 8)


def test_without_ids(window):
    """the call as tests/test_gpu_resource_lifetime.py makes it: no frame updates the object layer"""
    win, slots = window
    _run(win, slots[:8], None)


def test_dynamic_mask(window):
    """use_mask with dynamic images painted over part of the wall in some frames (the others clean: their mask is switched off per
    frame), and with clean images only; the painted run must differ from the clean one"""
    win, slots = window
    n = 9
    clean = _run(win, slots[:n], [3] * n, use_mask=True)
    assert clean == _run(win, slots[:n], [3] * n, use_mask=False)
    dyn = np.zeros((H, W), np.int32)
    dyn[60:200, 100:260] = 1
    painted = (1, 2, 5, 7, 8)
    try:
        for i in painted:
            win.set_frame_image(slots[i], 0, dyn)
        masked = _run(win, slots[:n], [3] * n, use_mask=True)
    finally:
        for i in painted:
            win.set_frame_image(slots[i], 0, None)
        win.sync()
    assert masked != clean
