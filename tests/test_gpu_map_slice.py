"""khr_map_slice / FusionContext.map_slice: one z-plane of the live map read on the device (ActiveWindowVisualizer's map slices,
active_window_visualizer.cpp:345-520), held bit for bit to a numpy restatement of the visualizer's loops over the per-block
downloads of the same context and over the oracle's blocks."""
import json
import os
import subprocess

import numpy as np
import pytest

from common import make_pair, step_both
from khronos_amd import FusionContext, default_config
from khronos_amd.capi import KHR_ENOMEM, slice_voxel_z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
FIELDS = ("block_xy", "positions", "distance", "weight", "last_observed", "flags")


def restate(indices, get_block, vps, voxel_size, voxel_z):
    """The visualizer's slice loops (:371-378): every block with index z == the key's block z, in (bx, by) order, voxels
    x-outer / y-inner at the key's local z; positions = block origin + (i + 0.5) * voxel_size in float32 (ASSUMPTIONS.md A.1)."""
    bz, lz = divmod(int(voxel_z), vps)
    f32 = np.float32
    vs = f32(voxel_size)
    bs = vs * f32(vps)
    x, y = (a.ravel() for a in np.meshgrid(np.arange(vps), np.arange(vps), indexing="ij"))
    lin = x + vps * (y + vps * lz)
    idx = np.asarray(indices, np.int32).reshape(-1, 3)
    idx = idx[idx[:, 2] == bz]
    idx = idx[np.lexsort((idx[:, 1], idx[:, 0]))]
    out = {k: [] for k in FIELDS}
    for b in idx:
        blk = get_block(b)
        out["block_xy"].append(b[:2])
        px = f32(b[0]) * bs + (x.astype(f32) + f32(0.5)) * vs
        py = f32(b[1]) * bs + (y.astype(f32) + f32(0.5)) * vs
        pz = np.full(vps * vps, f32(b[2]) * bs + (f32(lz) + f32(0.5)) * vs, f32)
        out["positions"].append(np.stack([px, py, pz], axis=1))
        for k, src in (("distance", "distance"), ("weight", "weight"), ("last_observed", "last_observed"), ("flags", "flags")):
            out[k].append(blk[src][lin])
    dt = {"block_xy": np.int32, "positions": np.float32, "distance": np.float32, "weight": np.float32, "last_observed": np.uint64,
          "flags": np.uint8}
    empty = {"block_xy": (0, 2), "positions": (0, 3)}
    return {k: (np.concatenate(v) if k != "block_xy" else np.stack(v)).astype(dt[k]) if v else np.zeros(empty.get(k, (0,)), dt[k])
            for k, v in out.items()}


def assert_same(a, b, what=""):
    for k in FIELDS:
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def run_stream(n_frames=30, archive_every=5, **cfg_kw):
    cfg, ctx, ora, s, sen, osen = make_pair(**cfg_kw)
    removed = []
    for i in range(n_frames):
        step_both(ctx, ora, sen, osen, s.render(i), motion=bool(cfg.with_tracking), track=bool(cfg.with_tracking))
        if archive_every and i % archive_every == archive_every - 1:
            rg, ro = np.asarray(ctx.reset_inactive()), np.asarray(ora.reset_inactive())
            assert np.array_equal(rg, ro)
            removed.extend(rg.reshape(-1, 3).tolist())
    return cfg, ctx, ora, removed


@pytest.fixture(scope="module")
def stream():
    # a short temporal window: blocks leave the window while the camera circles and the archival pass removes them
    return run_stream(temporal_window=0.6)


# mid-room layer, a negative z, an exact block boundary (1.6 = 1 block of 16 x 0.1), the map's floor plane, a layer with no blocks
HEIGHTS = (0.95, -0.05, 1.6, 0.0, 40.0)


@pytest.mark.gpu
@pytest.mark.parametrize("height", HEIGHTS)
def test_slice_matches_visualizer_loops(stream, height):
    cfg, ctx, ora, removed = stream
    vz = slice_voxel_z(height, cfg.voxel_size, cfg.voxels_per_side)
    got = ctx.map_slice(vz)
    assert got["voxel_z"] == vz
    mine = restate(ctx.block_indices(), ctx.download_block, cfg.voxels_per_side, cfg.voxel_size, vz)
    assert_same(got, mine, "download_block")
    oracle = restate(ora.block_indices(), ora.get_block, cfg.voxels_per_side, cfg.voxel_size, vz)
    assert_same(got, oracle, "oracle")
    n_blocks = len(got["block_xy"])
    if height == 40.0:
        assert n_blocks == 0
    elif height in (0.95, -0.05):
        assert n_blocks > 0
    # archived blocks are absent
    bz = vz // cfg.voxels_per_side
    live = {tuple(b) for b in ctx.block_indices().tolist()}
    on_layer = {tuple(b) for b in got["block_xy"].tolist()}
    for b in removed:
        if b[2] == bz and tuple(b) not in live:
            assert (b[0], b[1]) not in on_layer


@pytest.mark.gpu
def test_archival_happened_and_repeat_calls_are_identical(stream):
    cfg, ctx, ora, removed = stream
    assert len(removed) > 0, "the stream archived nothing: the absence check would be vacuous"
    vz = slice_voxel_z(0.95, cfg.voxel_size, cfg.voxels_per_side)
    a, b = ctx.map_slice(vz), ctx.map_slice(vz)
    assert_same(a, b, "repeat")
    assert (a["last_observed"] != 0).any()


@pytest.mark.gpu
def test_cap_too_small_leaves_buffers_untouched(stream):
    cfg, ctx, ora, removed = stream
    vz = slice_voxel_z(0.95, cfg.voxel_size, cfg.voxels_per_side)
    n = len(ctx.map_slice(vz)["distance"])
    assert n > 0
    cap = n - 1
    out = {"block_xy": np.full((n, 2), 7, np.int32), "positions": np.full((n, 3), 7, np.float32),
           "distance": np.full(n, 7, np.float32), "weight": np.full(n, 7, np.float32),
           "last_observed": np.full(n, 7, np.uint64), "flags": np.full(n, 7, np.uint8)}
    before = {k: v.copy() for k, v in out.items()}
    rc, count = ctx.map_slice_into(vz, cap, out)
    assert rc == KHR_ENOMEM and count == n
    for k in FIELDS:
        assert np.array_equal(out[k], before[k]), k
    # NULL outputs: only the count
    rc, count = ctx.map_slice_into(vz, 0, {})
    assert rc == KHR_ENOMEM and count == n
    rc, count = ctx.map_slice_into(vz, n, {"distance": out["distance"]})
    assert rc == 0 and count == n
    assert np.array_equal(out["distance"], ctx.map_slice(vz)["distance"])


@pytest.mark.gpu
def test_8vps_context():
    cfg, ctx, ora, removed = run_stream(n_frames=12, archive_every=0, voxels_per_side=8, voxel_size=0.05, truncation_distance=0.15,
                                        max_blocks=16384)
    for h in (0.5, -0.03, 0.4):
        vz = slice_voxel_z(h, cfg.voxel_size, 8)
        got = ctx.map_slice(vz)
        assert_same(got, restate(ctx.block_indices(), ctx.download_block, 8, cfg.voxel_size, vz), "8^3 %r" % h)
        assert_same(got, restate(ora.block_indices(), ora.get_block, 8, cfg.voxel_size, vz), "8^3 oracle %r" % h)
    assert len(ctx.map_slice(slice_voxel_z(0.5, cfg.voxel_size, 8))["block_xy"]) > 0


@pytest.mark.gpu
def test_without_tracking_stamps_are_zero():
    cfg, ctx, ora, removed = run_stream(n_frames=6, archive_every=0, with_tracking=0)
    vz = slice_voxel_z(0.95, cfg.voxel_size, cfg.voxels_per_side)
    got = ctx.map_slice(vz)
    assert len(got["block_xy"]) > 0
    assert not got["last_observed"].any()
    assert_same(got, restate(ctx.block_indices(), ctx.download_block, cfg.voxels_per_side, cfg.voxel_size, vz), "no tracking")


@pytest.mark.gpu
def test_layer_beyond_the_one_workgroup_sort():
    """9000 blocks on one layer (> the 4096 keys of the LDS sort; padded to 16384: two cross-tile merge stages)."""
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, voxels_per_side=8, with_semantics=0, with_tracking=1,
                         max_blocks=12000, max_frame_pixels=64 * 48)
    ctx = FusionContext(cfg)
    rng = np.random.default_rng(5)
    xs, ys = np.meshgrid(np.arange(-50, 50), np.arange(-45, 45), indexing="ij")
    layer = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, -3)], axis=1)
    other = np.stack([rng.integers(-60, 60, 500), rng.integers(-60, 60, 500), np.full(500, 2)], axis=1)
    other = np.unique(other, axis=0)
    idx = np.concatenate([layer, other]).astype(np.int32)
    idx = idx[rng.permutation(len(idx))]
    ctx.allocate_blocks(idx)
    vz = -3 * 8 + 5
    got = ctx.map_slice(vz)
    want_xy = layer[np.lexsort((layer[:, 1], layer[:, 0]))][:, :2].astype(np.int32)
    assert np.array_equal(got["block_xy"], want_xy)
    sub = want_xy[:: 97]
    check = restate(np.concatenate([sub, np.full((len(sub), 1), -3)], axis=1), ctx.download_block, 8, cfg.voxel_size, vz)
    rows = np.searchsorted(want_xy[:, 0] * 1000 + want_xy[:, 1], sub[:, 0] * 1000 + sub[:, 1])
    sel = (rows[:, None] * 64 + np.arange(64)[None, :]).ravel()
    for k in ("positions", "distance", "weight", "last_observed", "flags"):
        assert got[k][sel].tobytes() == check[k].tobytes(), k
    # the other layer and a smaller one still come out right after the multi-pass run
    got2 = ctx.map_slice(2 * 8)
    o = other[np.lexsort((other[:, 1], other[:, 0]))][:, :2].astype(np.int32)
    assert np.array_equal(got2["block_xy"], o)


YAML = """
active_window:
  type: "ActiveWindow"
  min_output_separation: 0.4
  frame_data_buffer:
    max_buffer_size: 40
    store_every_n_frames: 1
  volumetric_map:
    voxel_size: 0.1
    truncation_distance: 0.3
    voxels_per_side: 16
    with_semantics: true
  motion_detector:
    type: "FreeSpaceMotionDetector"
    min_cluster_size: 20
    min_separation_distance: 2
    max_range: 5
  tracking_integrator:
    temporal_window: 0.75
  device:
    num_labels: 20
    max_blocks: 4096
"""


@pytest.mark.gpu
def test_aw_demo_device_slices_equal_block_copies(tmp_path):
    cfgp = tmp_path / "aw_slices.yaml"
    cfgp.write_text(YAML)
    n_frames = 16
    # slice 0.55 m below the body (the camera circles at 1.5 m), then an absolute slice with the unknown voxels shown
    for args in (["-0.55", "1", "0"], ["0.35", "0", "1"]):
        out = subprocess.run([DEMO, "--slices", str(cfgp), "320", "240", str(n_frames)] + args, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        r = json.loads(out.stdout.strip().splitlines()[-1])
        assert r["frames"] == n_frames and r["agree_frames"] == n_frames, r
        assert r["blocks_on_layer_max"] > 0 and r["points"] > 0, r
