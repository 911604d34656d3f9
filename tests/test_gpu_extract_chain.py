"""-m gpu: the object extractor's fused call sequence against the step-wise one it stands for, bit for bit.

Two fresh mini contexts per case and arithmetic mode, the same frames of the same window context:
  step-wise   khr_reset_map, khr_allocate_blocks, khr_integrate_shared_batch, khr_object_prune(0.5, 2.0), khr_generate_mesh
  fused       khr_begin_object_map (the box as arguments: k_reset_map + k_setup_box), khr_integrate_prune_batch (the pruning in the
              last launch of k_fuse_obj, over the items no frame touches as well), khr_generate_mesh
and then equal: the map digest, every layer of every block, the block indices, the prune count, the statistics, and the mesh --
khr_download_mesh of the step-wise context against khr_fetch_mesh of the fused one, triangles sorted.  The cases come from
tests/object_map_cases.py: frames and items nothing touches (C1, C4), batches of two and three launches (9 and 15 frames: the
pruning goes with the last launch only), two words of frame bits (R2's 40 frames), batches the multi-frame path declines (one
frame; the label layout, whose batch runs on k_fuse2) and therefore prunes with k_object_prune, and a context that has held a
smaller or a larger box before."""
import numpy as np
import pytest

import object_map_cases as oc
from khronos_amd import FusionContext
from khronos_amd.capi import KhronosAmdError

pytestmark = pytest.mark.gpu

# 36 blocks of 24 cm around the wall point of WALL_BOX_FINE (3 x 3 x 4)
WALL_BOX_FINE_36 = oc.box((5, 7), (11, 13), (5, 8))
STATS = ("n_allocated_blocks", "n_visible_blocks", "n_new_blocks", "n_visited_voxels", "n_updated_voxels", "n_band_voxels",
         "n_mesh_blocks", "n_mesh_vertices", "pool_exhausted", "cum_updated_voxels", "cum_band_voxels", "cum_visited_voxels",
         "cum_integrate_calls", "n_tsdf_blocks", "n_fuse_items")

_windows = {}


@pytest.fixture(scope="module")
def windows():
    """one window context per case of object_map_cases, its frames uploaded once and shared by every test of the module"""
    def get(name, layout=None):
        key = (name, layout)
        if key not in _windows:
            case = oc.variant(name, layout)
            _windows[key] = (case,) + oc._window(case)
        return _windows[key]
    yield get
    for _, win, _ in _windows.values():
        win.close()
    _windows.clear()


def _object(ctx, case, win, slots, scale, indices, ks, fused):
    """one object on `ctx`; returns ("ok", prune count) or ("error", message) of the sequence"""
    oid = oc.OBJECT_ID if oc.uses_object_image(case) else -1
    ids = [oid] * len(ks) if oc.uses_object_image(case) else None
    sl = [slots[k] for k in ks]
    try:
        if fused:
            ctx.begin_object_map(scale[0], scale[1], indices.min(0), indices.max(0))
            pruned = ctx.integrate_prune_batch(win, sl, ids, 0.5, 2.0)
        else:
            ctx.reset_map(*scale)
            ctx.allocate_blocks(indices)
            ctx.integrate_shared_batch(win, sl, ids)
            pruned = ctx.object_prune(0.5, 2.0)
        ctx.generate_mesh(True, False)
        return "ok", pruned
    except KhronosAmdError as e:
        return "error", str(e).split(":", 1)[-1].strip()


def _sorted_triangles(mesh, keys):
    n = len(mesh["points"]) // 3
    assert len(mesh["points"]) == 3 * n
    if n == 0:   # (a batch of one frame: no voxel reaches two observations, every surface voxel is pruned)
        return {k: np.ascontiguousarray(mesh[k]) for k in keys}
    cols = [np.ascontiguousarray(mesh[k]).reshape(n, -1).view(np.uint8).reshape(n, -1) for k in keys]
    rows = np.concatenate(cols, axis=1)
    order = np.lexsort(rows.T[::-1])
    return {k: np.ascontiguousarray(mesh[k]).reshape(n, -1)[order] for k in keys}


def _compare(case, a, b, ra, rb):
    """a: step-wise, b: fused"""
    print(case["name"], "step-wise", ra, "fused", rb)
    assert ra == rb
    da, db = [int(x) for x in a.map_digest()], [int(x) for x in b.map_digest()]
    assert da == db, [n for n, x, y in zip(FusionContext.DIGEST_LAYERS, da, db) if x != y]
    ia, la = oc._layers(a)
    ib, lb = oc._layers(b)
    assert np.array_equal(ia, ib) and a.num_blocks() == b.num_blocks() == len(ia)
    assert np.array_equal(a.block_indices(), b.block_indices())
    for k in oc.LAYERS:
        assert la[k].tobytes() == lb[k].tobytes(), k
    sa, sb = a.stats(), b.stats()
    print(case["name"], {k: (sa[k], sb[k]) for k in STATS})
    for k in STATS:
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    if ra[0] != "ok":
        return
    keys = oc.MESH_KEYS[:4 if oc.LAYOUTS[case["layout"]]["with_tracking"] else 3]
    ma, mb = a.download_mesh(), b.fetch_mesh()
    assert len(ma["points"]) == len(mb["points"])
    ta, tb = _sorted_triangles(ma, keys), _sorted_triangles(mb, keys)
    for k in keys:
        assert ta[k].tobytes() == tb[k].tobytes(), k


def _run(windows, name, exact, objects, layout=None, touched=True):
    """objects: [(scale, indices, frames)], one after the other on both contexts; compared after each of them"""
    case, win, slots = windows(name, layout)
    a = FusionContext(oc.mini_config(case, objects[0][0], exact))
    b = FusionContext(oc.mini_config(case, objects[0][0], exact))
    try:
        for scale, indices, ks in objects:
            ra = _object(a, case, win, slots, scale, indices, ks, False)
            rb = _object(b, case, win, slots, scale, indices, ks, True)
            _compare(case, a, b, ra, rb)
            if touched and ra[0] == "ok":   # the case is not an empty one: frames updated voxels, the pruning erased some
                assert a.stats()["cum_updated_voxels"] > 0 and ra[1] > 0
    finally:
        a.close()
        b.close()


def _own(case):
    obj = case["objects"][-1]
    (_, indices), (_, ks) = obj["steps"]
    return obj["scale"], indices, list(ks)


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("name", ["C1", "C4"])
def test_frames_and_items_nothing_touches(windows, name, exact):
    """C1: a frame that looks away; C4: four of six frames see nothing of the box -- and in both most items of the box lie in
    free space or behind the wall: the pruning launch reaches them through the list of untouched items and counts them"""
    _run(windows, name, exact, [_own(oc.CASES[name])])


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("n_frames", [9, 15])
def test_prune_goes_with_the_last_launch_only(windows, n_frames, exact):
    """launches of 7 frames: 9 frames are two launches, 15 are three; a voxel pruned too early would be integrated into again"""
    assert n_frames > oc.K_MULTI_CHUNK and -(-n_frames // oc.K_MULTI_CHUNK) == (2 if n_frames == 9 else 3)
    _run(windows, "R2", exact, [(oc.COARSE, oc.WALL_BOX, list(range(n_frames)))])


@pytest.mark.parametrize("exact", [1, 0])
def test_two_words_of_frame_bits(windows, exact):
    """R2's last object: 40 frames on WALL_BOX_FINE, six launches"""
    _run(windows, "R2", exact, [_own(oc.CASES["R2"])])


@pytest.mark.parametrize("exact", [1, 0])
def test_declined_one_frame_batch_is_pruned_by_the_kernel(windows, exact):
    """R4's batch of one frame: frame by frame, then k_object_prune"""
    _run(windows, "R4", exact, [(oc.COARSE, oc.WALL_BOX, [0])])


@pytest.mark.parametrize("exact", [1, 0])
def test_label_layout_prunes_or_refuses_as_step_wise(windows, exact):
    """R5: four labels, tracking stamps -- the batch runs on k_fuse2, the pruning is the step-wise call's, whatever it answers"""
    _run(windows, "R5", exact, [_own(oc.CASES["R5"])], touched=False)


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("order", ["after_smaller", "after_larger"])
def test_second_object_on_the_same_context(windows, order, exact):
    """27 blocks of 32 cm, then 36 of 24 cm -- and 36 of 24 cm, then 27 of 24 cm: the same slots, other blocks, other counts"""
    first, second = ((oc.COARSE, oc.WALL_BOX, [0, 20, 39]), (oc.FINE, WALL_BOX_FINE_36, list(range(0, 40, 4)))) if order == "after_smaller" \
        else ((oc.FINE, WALL_BOX_FINE_36, list(range(0, 40, 4))), (oc.FINE, oc.WALL_BOX_FINE, list(range(1, 40, 3))))
    _run(windows, "R2", exact, [first, second])
