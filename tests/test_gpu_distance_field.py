"""khr_distance_field / FusionContext.distance_field: the exact Euclidean distance field of a box of the live map (ASSUMPTIONS.md
A.15), held bit for bit to tests/distance_replica.py -- on the hand-built maps of tests/distance_cases.py, on box shapes at which a
pass can go wrong, and on the 30-frame stream over this context's block downloads and over the CPU oracle's blocks."""
import itertools
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import distance_cases as dc
import distance_replica as dr
import mesh_cases as mc
import query_replica as qr
from common import DeviceArray, make_pair, step_both
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_DF_MAX_DIM, KHR_EINVAL, KHR_ESTATE

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
FIELDS = FusionContext.DF_FIELDS
N_FRAMES = 30
GUARD = 64  # entries after each output buffer that a call must leave alone
_maps = {}


def hand_built(name, vps):
    """(cfg, ctx, replica block set) of a hand-built map, loaded once per module"""
    if (name, vps) not in _maps:
        indices, layers = dc.CASES[name](vps)
        cfg = default_config(voxels_per_side=vps, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
        ctx = FusionContext(cfg)
        assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
        _maps[(name, vps)] = (cfg, ctx, qr.QueryBlocks(ctx.block_indices(), ctx.download_block, vps))
    return _maps[(name, vps)]


def assert_same(got, want, what):
    for k, dt in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), [got[k][tuple(b)].item() for b in bad[:4]], [want[k][tuple(b)].item() for b in bad[:4]]))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


def replica(cfg, blocks, origin, dims, ratio, max_distance, min_weight=None, **kw):
    return dr.distance_field(blocks, cfg.voxel_size, origin, dims, ratio, max_distance, cfg.mesh_min_weight if min_weight is None else min_weight, **kw)


@pytest.mark.parametrize("ratio", [1, 2, 4])
@pytest.mark.parametrize("vps", [16, 8])
@pytest.mark.parametrize("name", ["wall", "random"])
def test_hand_built_maps_match_the_replica_bit_for_bit(name, vps, ratio):
    cfg, ctx, blocks = hand_built(name, vps)
    origin, dims = dc.box_of(name, vps, ratio)
    assert origin[0] < 0 and origin[2] < 0 and any(o % (vps // ratio) for o in origin)
    cell = float(f32(cfg.voxel_size) * f32(ratio))
    seen = set()
    classes = {sd: dr.classify(blocks, origin, dims, ratio, cfg.mesh_min_weight, sd) for sd in (0.0, 0.4 * mc.TRUNCATION)}
    for far, unk, pos, sd in itertools.product((False, True), (False, True), (False, True), (0.0, 0.4 * mc.TRUNCATION)):
        max_distance = 100.0 if far else 5.5 * cell   # beyond the box / five cells
        kw = dict(surface_distance=sd, unknown_is_obstacle=unk, positive_only=pos)
        want = replica(cfg, blocks, origin, dims, ratio, max_distance, classes=classes[sd], **kw)
        got = ctx.distance_field(origin, dims, ratio, max_distance, **kw)
        assert_same(got, want, (name, vps, ratio, far, kw))
        n, st = want["d2"].size, want["stats"]
        assert 0 < st["n_obstacle"] and st["n_observed"] < n   # the box reaches past the blocks
        if name == "wall" and sd == 0.0:
            assert st["n_free"] > 0   # (random signs, or a surface distance among the magnitudes: a cell of 64 voxels is rarely free)
        if not far and not unk:
            assert 0 < st["n_in_range"] < n, (name, vps, ratio, kw, st)   # five cells: out-of-range cells occur
        seen.add(got["d2"].tobytes())
    print("%s vps %d ratio %d: %d distinct fields of 16" % (name, vps, ratio, len(seen)))
    assert len(seen) >= 4


SHAPES = [(1, 1, 1), (1, 257, 1), (1, 1, 257), (63, 3, 2), (64, 3, 2), (65, 3, 2), (256, 3, 2), (512, 2, 2), (2, 512, 2), (2, 2, 512)]


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_shapes_where_a_pass_can_go_wrong(dims):
    cfg, ctx, blocks = hand_built("wall", 16)
    first = dc.group_first_cell(dc.WALL_ORIGIN, 16, 1)
    s = dc.wall_start(16)
    # the box starts one column in front of the slab, a little inside the group on y and z; long boxes run out of the blocks
    for origin in ((first[0] + s - 1, first[1] + 1, first[2] + 1), (first[0] + s - 7, first[1] - 3, first[2] - 2)):
        for max_distance, kw in ((0.35, {}), (100.0, {}), (100.0, dict(unknown_is_obstacle=True)), (2.05, dict(unknown_is_obstacle=True, positive_only=True))):
            assert_same(ctx.distance_field(origin, dims, 1, max_distance, **kw), replica(cfg, blocks, origin, dims, 1, max_distance, **kw),
                        (dims, origin, max_distance, kw))


def guarded(n, fields, fill=7):
    return {k: np.full(n + GUARD, fill, dt) for k, dt in FIELDS if k in fields}


def test_513_is_rejected():
    cfg, ctx, blocks = hand_built("wall", 16)
    for dims in ((KHR_DF_MAX_DIM + 1, 1, 1), (1, KHR_DF_MAX_DIM + 1, 1), (1, 1, KHR_DF_MAX_DIM + 1)):
        out = guarded(KHR_DF_MAX_DIM + 1, [k for k, _ in FIELDS])
        rc, stats = ctx.distance_field_into(ctx.df_request((0, 0, 0), dims, 1, 1.0), out)
        assert rc == KHR_EINVAL and stats is None
        assert all((a == 7).all() for a in out.values())


# ---- the stream map ------------------------------------------------------------------------------------------------------------
def run_stream(n_frames=N_FRAMES, archive_every=5, **cfg_kw):
    """the stream of tests/test_gpu_query_points.py: tracking and motion detection on, archival every few frames"""
    cfg, ctx, ora, s, sen, osen = make_pair(**cfg_kw)
    st = SimpleNamespace(cfg=cfg, ctx=ctx, ora=ora, s=s, sen=sen, osen=osen, last=None, cache={})
    for i in range(n_frames):
        step(st, i)
        if archive_every and i % archive_every == archive_every - 1:
            assert np.array_equal(np.asarray(ctx.reset_inactive()), np.asarray(ora.reset_inactive()))
    return st


def step(st, i):
    st.last = st.s.render(i)
    st.last["step"] = step_both(st.ctx, st.ora, st.sen, st.osen, st.last, motion=bool(st.cfg.with_tracking), track=bool(st.cfg.with_tracking))
    st.cache.clear()


def blocks_of(st, which):
    if which not in st.cache:
        src, get = (st.ctx, st.ctx.download_block) if which == "ctx" else (st.ora, st.ora.get_block)
        st.cache[which] = qr.QueryBlocks(src.block_indices(), get, st.cfg.voxels_per_side)
    return st.cache[which]


@pytest.fixture(scope="module")
def stream():
    return run_stream(temporal_window=0.6)


def stream_request(st):
    origin, dims = dc.stream_box(st.last["pose"], st.cfg.voxel_size)
    return origin, dims, dc.STREAM_RATIO, dc.STREAM_MAX_DISTANCE


def test_stream_map_matches_the_replica_over_downloads_and_over_the_oracle(stream):
    st = stream
    rq = stream_request(st)
    for kw in ({}, dict(unknown_is_obstacle=True), dict(positive_only=True), dict(surface_distance=0.05, min_weight=3.0)):
        got = st.ctx.distance_field(*rq, **kw)
        mine = replica(st.cfg, blocks_of(st, "ctx"), *rq, **kw)
        n = mine["d2"].size
        print("stream %s: %s of %d cells" % (kw, mine["stats"], n))
        if not kw:
            assert mine["stats"]["n_obstacle"] > 0.01 * n and mine["stats"]["n_free"] > 0.01 * n and mine["stats"]["n_observed"] < 0.99 * n
        assert_same(got, mine, ("stream / download_block", kw))
        assert_same(got, replica(st.cfg, blocks_of(st, "ora"), *rq, **kw), ("stream / oracle", kw))
    assert st.ctx.distance_field(*rq, min_weight=3.0)["stats"] != st.ctx.distance_field(*rq)["stats"]


def test_fields_follow_archival():
    """the same box before and after a further reset_inactive() that removes blocks (the hash table is rebuilt)"""
    st = run_stream(temporal_window=0.6)
    rq = stream_request(st)
    before = replica(st.cfg, blocks_of(st, "ctx"), *rq)
    assert_same(st.ctx.distance_field(*rq), before, "before")
    for i in range(N_FRAMES, N_FRAMES + 4):
        step(st, i)
    removed = np.asarray(st.ctx.reset_inactive())
    assert np.array_equal(removed, np.asarray(st.ora.reset_inactive())) and len(removed) > 0
    st.cache.clear()
    after = replica(st.cfg, blocks_of(st, "ctx"), *rq)
    print("archival removed %d blocks: observed cells %d -> %d" % (len(removed), before["stats"]["n_observed"], after["stats"]["n_observed"]))
    assert after["status"].tobytes() != before["status"].tobytes()
    got = st.ctx.distance_field(*rq)
    assert_same(got, after, "after / download_block")
    assert_same(got, replica(st.cfg, blocks_of(st, "ora"), *rq), "after / oracle")
    st.ctx.close()


def test_device_form_equals_the_host_form(stream):
    st = stream
    origin, dims, ratio, md = stream_request(st)
    n = int(np.prod(dims))
    names = [k for k, _ in FIELDS]
    for kw in ({}, dict(positive_only=True)):
        host = st.ctx.distance_field(origin, dims, ratio, md, **kw)
        rq = st.ctx.df_request(origin, dims, ratio, md, **kw)
        # the host form itself leaves the guard entries alone, whichever outputs are asked for
        for fields in ([k] for k in names):
            out = guarded(n, fields)
            rc, stats = st.ctx.distance_field_into(rq, out, want_stats=False)
            assert rc == 0 and stats is None
            assert out[fields[0]][:n].tobytes() == host[fields[0]].tobytes() and (out[fields[0]][n:] == 7).all(), (kw, fields)
        rc, stats = st.ctx.distance_field_into(rq, {})
        assert rc == 0 and stats == host["stats"]
        # device pointers: all outputs with and without the counters (then stream order only: khr_sync, the same bytes), each
        # output alone, and none but the counters
        variants = [(names, True), (names, False)] + [([k], False) for k in names] + [([], True)]
        for fields, want_stats in variants:
            dev = {k: DeviceArray(v) for k, v in guarded(n, fields, fill=9).items()}
            rc, stats = st.ctx.distance_field_into(rq, {k: d.data_ptr() for k, d in dev.items()}, on_device=True, want_stats=want_stats)
            assert rc == 0 and (stats == host["stats"] if want_stats else stats is None), (kw, fields, want_stats, rc, stats)
            st.ctx.sync()
            for k, dt in FIELDS:
                if k in dev:
                    size = np.dtype(dt).itemsize
                    assert dev[k].read(0, n * size).tobytes() == host[k].tobytes(), (kw, fields, want_stats, k)
                    assert (dev[k].read(n * size, GUARD * size).view(dt) == 9).all(), (kw, fields, want_stats, k)
                    dev[k].free()


def test_the_call_only_reads_and_repeats_identically(stream):
    st = stream
    digest, idx, stats = st.ctx.map_digest(), st.ctx.block_indices().copy(), st.ctx.stats()
    origin, dims, ratio, md = stream_request(st)
    a, b = st.ctx.distance_field(origin, dims, ratio, md), st.ctx.distance_field(origin, dims, ratio, md)
    for k, _ in FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"] == b["stats"]
    # a small box after a large one: the work grids and the staging keep their size, the small box uses their front
    small = ((origin[0] + 11, origin[1] + 9, origin[2] + 5), (13, 17, 9))
    for kw in ({}, dict(unknown_is_obstacle=True)):
        assert_same(st.ctx.distance_field(*small, ratio, md, **kw), replica(st.cfg, blocks_of(st, "ctx"), *small, ratio, md, **kw), ("small after large", kw))
    assert np.array_equal(st.ctx.map_digest(), digest)
    assert np.array_equal(st.ctx.block_indices(), idx)
    assert st.ctx.stats() == stats


def test_error_codes_leave_the_buffers_untouched(stream):
    st = stream
    names = [k for k, _ in FIELDS]
    good = dict(origin=(-3, -3, -3), dims=(6, 6, 6), ratio=1, max_distance=1.0)
    nan, inf = float("nan"), float("inf")
    big = 1 << 30
    cases = {
        "zero dim": dict(dims=(6, 0, 6)), "negative dim": dict(dims=(-1, 6, 6)), "dim 513": dict(dims=(6, 6, 513)),
        "more than 2^24 cells": dict(dims=(512, 512, 65)), "ratio 0": dict(ratio=0), "ratio 3": dict(ratio=3), "ratio 8": dict(ratio=8),
        "ratio -1": dict(ratio=-1), "box above the index range": dict(origin=(big - 3, 0, 0)), "box below the index range": dict(origin=(0, -big, 0)),
        "box beyond the index range at ratio 4": dict(origin=(0, 0, big // 4 - 3), ratio=4),
        "nan surface_distance": dict(surface_distance=nan), "inf surface_distance": dict(surface_distance=-inf),
        "negative min_weight": dict(min_weight=-1.0), "nan min_weight": dict(min_weight=nan), "inf min_weight": dict(min_weight=inf),
        "zero max_distance": dict(max_distance=0.0), "negative max_distance": dict(max_distance=-1.0), "nan max_distance": dict(max_distance=nan),
        "inf max_distance": dict(max_distance=inf), "a range of 32768 cells": dict(max_distance=3277.0),
    }
    n = 6 * 6 * 6
    for what, kw in cases.items():
        out = guarded(n, names)
        rc, stats = st.ctx.distance_field_into(st.ctx.df_request(**dict(good, **kw)), out)
        assert rc == KHR_EINVAL and stats is None, (what, rc)
        for k, a in out.items():
            assert (a == 7).all(), (what, k)
    out = guarded(n, names)
    rc, stats = st.ctx.distance_field_into(None, out)
    assert rc == KHR_EINVAL and stats is None and all((a == 7).all() for a in out.values())
    # the edge of the index range is fine, and so is a range of just under 32768 cells
    for kw in (dict(origin=(big - 6, -big + 1, 0)), dict(max_distance=3276.0)):
        out = guarded(n, names)
        rc, stats = st.ctx.distance_field_into(st.ctx.df_request(**dict(good, **kw)), out)
        assert rc == 0 and all((a[n:] == 7).all() for a in out.values()), kw
    # a ratio that does not divide voxels_per_side cannot be had with 8 or 16 and the ratios 1, 2, 4; a shard cannot answer
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=64 * 48, rank=0, world_size=2)
    shard = FusionContext(cfg)
    out = guarded(n, names)
    rc, stats = shard.distance_field_into(shard.df_request(**good), out)
    assert rc == KHR_ESTATE and stats is None
    for k, a in out.items():
        assert (a == 7).all(), k
    shard.close()


def test_the_field_agrees_with_the_scene(stream):
    """independent of the replica: a free cell beside an obstacle cell is one cell away from it (the median over such cells is
    exactly cell_size), and the cells that hold the last frame's back-projected surface lie within two cells of an obstacle for at
    least 95 % of the non-dynamic pixels whose cell is observed (the CPU oracle's map: 0.9996, tests/test_cpu_distance_field.py)"""
    st = stream
    origin, dims, ratio, md = stream_request(st)
    out = st.ctx.distance_field(origin, dims, ratio, md)
    status, dist = out["status"], out["distance"]
    free, obst = (status & 3) == 1, (status & 2) != 0
    nb = np.zeros_like(obst)
    for axis in range(3):
        for sh in (1, -1):
            r = np.roll(obst, sh, axis=axis)
            edge = [slice(None)] * 3
            edge[axis] = 0 if sh == 1 else -1
            r[tuple(edge)] = False
            nb |= r
    assert (free & nb).sum() > 100
    assert float(np.median(dist[free & nb])) == out["cell_size"]
    c = dc.surface_cells(st.last, st.sen, st.last["step"]["dyn_gpu"], out["cell_size"], origin, dims)
    seen = (status[c[:, 2], c[:, 1], c[:, 0]] & 1) != 0
    near = np.abs(dist[c[:, 2], c[:, 1], c[:, 0]][seen]) <= f32(2) * f32(out["cell_size"])
    print("surface pixels in the box: %d, observed cell: %d, within two cells: %.4f" % (len(c), seen.sum(), near.mean()))
    assert seen.sum() > 1000 and near.mean() >= 0.95


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
frontend:
  freespace_places:
    gvd:
      max_distance_m: 1.5
      min_weight: 1.0e-6
      positive_distance_only: false
    tsdf_interpolator:
      type: downsample
      ratio: 2
"""


def test_aw_demo_distance_mode_agrees_with_block_copies(tmp_path):
    """aw_demo --distance: a Khronos sink asks for the field of a box around the sensor through VolumetricMap::distanceField and
    computes the same from cloneBlock copies with A.15's arithmetic on the host; the two agree bit for bit on every output"""
    W, H, N = 320, 240, 8
    cfgp = tmp_path / "aw_distance.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--distance", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N and res["agree_frames"] == N and res["first_mismatch"] == ""
    assert res["cells"] > 0 and res["last_stats"]["n_obstacle"] > 0 and res["last_stats"]["n_free"] > 0
    assert res["last_stats"]["n_in_range"] > 0 and res["device_ms"] > 0 and res["block_copy_ms"] > 0
