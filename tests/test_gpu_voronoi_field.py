"""khr_voronoi_field / FusionContext.voronoi_field: nearest obstacle cell and generalized Voronoi cells of a box of the live map
(ASSUMPTIONS.md A.20), every dense output, every list array and every counter held bit for bit to tests/voronoi_replica.py -- on
the hand-built maps of tests/distance_cases.py and tests/voronoi_cases.py, on box shapes at which a pass can go wrong, and on the
30-frame stream over this context's block downloads and over the CPU oracle's blocks."""
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
import voronoi_cases as vc
import voronoi_replica as vr
from common import DeviceArray, make_pair, step_both
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ESTATE

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
FIELDS = FusionContext.VOR_FIELDS
NAMES = [k for k, _, _, _ in FIELDS]
N_FRAMES = 30
GUARD = 64  # entries after each output buffer that a call must leave alone
_maps = {}


def load(key, vps, indices, layers):
    """(cfg, ctx, replica block set) of a hand-built map, loaded once per module"""
    if key not in _maps:
        cfg = default_config(voxels_per_side=vps, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
        ctx = FusionContext(cfg)
        assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
        _maps[key] = (cfg, ctx, qr.QueryBlocks(ctx.block_indices(), ctx.download_block, vps))
    return _maps[key]


def hand_built(name, vps):
    if (name, vps) not in _maps:
        load((name, vps), vps, *dc.CASES[name](vps))
    return _maps[(name, vps)]


def assert_same(got, want, what):
    for k, dt, _, _ in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), [got[k][tuple(b)].item() for b in bad[:4]], [want[k][tuple(b)].item() for b in bad[:4]]))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])


def keywords(mode, l1, cs, min_distance, **more):
    return dict(mode=mode, parent_l1_separation=l1, parent_cos_angle_separation=cs, min_distance=min_distance, **more)


def replica(cfg, blocks, origin, dims, ratio, max_distance, **kw):
    return vr.voronoi_field(blocks, cfg.voxel_size, origin, dims, ratio, max_distance, kw.pop("min_weight", cfg.mesh_min_weight), **kw)


# the cells with basis >= 2 under (L1, 4, 100 m), min_distance 2 cells, of a prototype of A.20 that shares no code with the replica
PROTOTYPE_COUNTS = {("wall", 16, 1, True): 3108, ("wall", 8, 2, True): 155, ("wall", 16, 4, True): 108,
                    ("random", 16, 1, False): 5232, ("random", 8, 2, False): 1415, ("random", 16, 4, False): 1415}


@pytest.mark.parametrize("ratio", [1, 2, 4])
@pytest.mark.parametrize("vps", [16, 8])
@pytest.mark.parametrize("name", ["wall", "random"])
def test_hand_built_maps_match_the_replica_bit_for_bit(name, vps, ratio):
    cfg, ctx, blocks = hand_built(name, vps)
    origin, dims = dc.box_of(name, vps, ratio)
    cell = f32(cfg.voxel_size) * f32(ratio)
    classes = dr.classify(blocks, origin, dims, ratio, cfg.mesh_min_weight, 0.0)
    for unk, (mode, l1, cs, max_distance) in itertools.product((False, True), vc.params(cell)):
        kw = keywords(mode, l1, cs, vc.MIN_DISTANCE_CELLS * float(cell), unknown_is_obstacle=unk)
        want = replica(cfg, blocks, origin, dims, ratio, max_distance, classes=classes, **kw)
        got = ctx.voronoi_field(origin, dims, ratio, max_distance, **kw)
        assert_same(got, want, (name, vps, ratio, max_distance, kw))
        # the first three outputs are khr_distance_field's with positive_only
        df = ctx.distance_field(origin, dims, ratio, max_distance, unknown_is_obstacle=unk, positive_only=True)
        for k in ("distance", "d2", "status"):
            assert got[k].tobytes() == df[k].tobytes(), (name, vps, ratio, kw, k)
        assert {k: got["stats"][k] for k in dr.STATS} == df["stats"]
        st = got["stats"]
        voronoi = st["n_basis2"] + st["n_basis3"] + st["n_basis4"]
        print("%s vps %d ratio %d unk %d mode %d range %.3g: %s" % (name, vps, ratio, unk, mode, max_distance, st))
        assert st["n_listed"] == voronoi == len(got["cells"])
        if name == "wall" and not unk:
            assert voronoi == 0 and st["n_eligible"] > 0   # one flat wall: every cell's neighbours look at the same face
        if name == "random" and unk:
            # obstacles everywhere: no cell is two cells away from one.  The free cells (a few thousand voxels at ratio 1, six cells
            # at ratio 2, none at ratio 4) touch an obstacle and have a site; every other cell has none
            assert st["n_eligible"] == 0 and voronoi == 0 and not got["basis"].any()
            assert len(got["cells"]) == len(got["cell_distance"]) == len(got["cell_basis"]) == len(got["cell_sites"]) == 0
            free = (got["status"] & 3) == 1
            assert np.array_equal(got["site"] >= 0, free) and (got["d2"][free] <= 3).all()
            if ratio == 4:
                assert (got["site"] == -1).all()
        if mode == vr.L1 and ((name == "wall" and unk) or (name == "random" and not unk)):
            if (name, vps, ratio, unk) in PROTOTYPE_COUNTS:
                assert voronoi == PROTOTYPE_COUNTS[(name, vps, ratio, unk)]
            if (name, vps, ratio) == ("wall", 8, 4):
                # cells of 4 voxels at 8 voxels per block: the free space in front of the slab (11 voxel columns) is nowhere two cells
                # from the slab and from the unknown cells around the group -- the replica on the CPU says so
                assert st["n_eligible"] == 0
            else:
                assert voronoi > 0
                if name == "random":   # (at (8, 4) the box holds 40 obstacle cells: 516 cells of basis 2, none above)
                    assert st["n_basis2"] > 0 and ((vps, ratio) == (8, 4) or min(st["n_basis3"], st["n_basis4"]) > 0)


SHAPES = [(1, 1, 1), (1, 257, 1), (1, 1, 257), (63, 3, 2), (64, 3, 2), (65, 3, 2), (256, 3, 2), (512, 2, 2), (2, 512, 2), (2, 2, 512)]


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_shapes_where_a_pass_can_go_wrong(dims):
    """the tile edge (64 lanes, 256 threads), the full-length line, the strip tail (2 or 3 of 16 x), lines of one cell"""
    cfg, ctx, blocks = hand_built("wall", 16)
    first = dc.group_first_cell(dc.WALL_ORIGIN, 16, 1)
    s = dc.wall_start(16)
    cell = float(f32(cfg.voxel_size))
    for origin in ((first[0] + s - 1, first[1] + 1, first[2] + 1), (first[0] + s - 7, first[1] - 3, first[2] - 2)):
        for max_distance, unk, (mode, l1, cs) in ((0.35, False, (vr.L1_THEN_ANGLE, 20, 0.2)), (100.0, False, (vr.L1, 4, 0.0)), (100.0, True, (vr.L1, 4, 0.0)),
                                                 (2.05, True, (vr.ANGLE, 1, 0.2))):
            kw = keywords(mode, l1, cs, cell, unknown_is_obstacle=unk)
            assert_same(ctx.voronoi_field(origin, dims, 1, max_distance, **kw), replica(cfg, blocks, origin, dims, 1, max_distance, **kw),
                        (dims, origin, max_distance, kw))


@pytest.mark.parametrize("mode,l1,cs", [(vr.L1, 4, 0.0), (vr.ANGLE, 1, 0.2), (vr.L1_THEN_ANGLE, 20, 0.2)])
def test_corridors_and_posts_match_their_construction(mode, l1, cs):
    cell = float(f32(mc.VOXEL_SIZE))
    kw = keywords(mode, l1, cs, vc.MIN_DISTANCE_CELLS * cell)
    for key, case in (("even", vc.corridor(vc.CORRIDOR_EVEN)), ("odd", vc.corridor(vc.CORRIDOR_ODD)), ("posts", vc.posts())):
        indices, layers, origin, dims, in_set = case
        cfg, ctx, blocks = load(key, vc.VPS, indices, layers)
        got = ctx.voronoi_field(origin, dims, 1, 100.0, **kw)
        assert_same(got, replica(cfg, blocks, origin, dims, 1, 100.0, **kw), (key, kw))
        assert np.array_equal((got["status"] & 2) != 0, in_set)
        columns = sorted(set((got["cells"][:, 0] - origin[0]).tolist()))
        if key == "even":
            assert columns == [6, 7] and len(got["cells"]) == 2 * dims[1] * dims[2]
        elif key == "odd":
            assert columns == [7, 8] and (got["site"][:, :, 7] % dims[0] == 2).all() and (got["site"][:, :, 8] % dims[0] == 12).all()
        else:
            x, y, z = vc.POSTS_CENTRE
            assert got["basis"][z, y, x] == 4
            row = np.flatnonzero((got["cells"] - np.asarray(origin) == np.asarray(vc.POSTS_CENTRE)).all(axis=1))
            assert len(row) == 1 and got["cell_basis"][row[0]] == 4
            assert {tuple(int(v) for v in p - np.asarray(origin)) for p in got["cell_sites"][row[0]]} == {(px, py, 3) for px, py in vc.POSTS}
            for mb in (0, 3, 4):
                sel = ctx.voronoi_field(origin, dims, 1, 100.0, min_basis=mb, **kw)
                assert_same(sel, replica(cfg, blocks, origin, dims, 1, 100.0, min_basis=mb, **kw), (key, kw, mb))
                assert sel["stats"]["n_listed"] == int((got["basis"] >= max(mb, 2)).sum()) > 0


def test_an_empty_obstacle_set_is_ok_with_no_sites_and_an_empty_list():
    cfg, ctx, blocks = hand_built("wall", 16)
    first = dc.group_first_cell(dc.WALL_ORIGIN, 16, 1)
    origin, dims = first, (dc.wall_start(16) - 1, 9, 7)
    got = ctx.voronoi_field(origin, dims, 1, 50.0)
    assert_same(got, replica(cfg, blocks, origin, dims, 1, 50.0), "empty O")
    assert (got["site"] == -1).all() and not got["basis"].any() and len(got["cells"]) == 0 and got["stats"]["n_in_range"] == 0
    assert got["stats"]["n_free"] == got["d2"].size and (got["d2"] == dr.FAR).all()


# ---- the stream map ------------------------------------------------------------------------------------------------------------
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
    """the stream of tests/test_gpu_distance_field.py: tracking and motion detection on, archival every five frames"""
    cfg, ctx, ora, s, sen, osen = make_pair(temporal_window=0.6)
    st = SimpleNamespace(cfg=cfg, ctx=ctx, ora=ora, s=s, sen=sen, osen=osen, last=None, cache={})
    for i in range(N_FRAMES):
        step(st, i)
        if i % 5 == 4:
            assert np.array_equal(np.asarray(ctx.reset_inactive()), np.asarray(ora.reset_inactive()))
    return st


def stream_request(st, **more):
    """the box and the parameters tests/test_cpu_voronoi_replica.py proves not to be vacuous"""
    origin, dims = dc.stream_box(st.last["pose"], st.cfg.voxel_size)
    kw = dict(vc.STREAM)
    ratio, max_distance = kw.pop("ratio"), kw.pop("max_distance")
    kw["min_distance"] = vc.MIN_DISTANCE_CELLS * float(f32(st.cfg.voxel_size) * f32(ratio))
    kw.update(more)
    return (origin, dims, ratio, max_distance), kw


def guarded(shapes, fields, fill=7):
    """flat buffers of the fields' sizes plus GUARD entries"""
    return {k: np.full(int(np.prod(shapes[w] + sh)) + GUARD * int(np.prod(sh + (1,))), fill, dt) for k, dt, sh, w in FIELDS if k in fields}


def shapes_of(out):
    return {"d": out["d2"].shape, "l": (len(out["cells"]),)}


def test_stream_map_matches_the_replica_over_downloads_and_over_the_oracle(stream):
    st = stream
    for more in ({}, dict(unknown_is_obstacle=True), dict(mode=vr.L1_THEN_ANGLE, parent_l1_separation=20, parent_cos_angle_separation=0.2, min_basis=3),
                 dict(surface_distance=0.05, min_weight=3.0, mode=vr.ANGLE)):
        rq, kw = stream_request(st, **more)
        got = st.ctx.voronoi_field(*rq, **kw)
        mine = replica(st.cfg, blocks_of(st, "ctx"), *rq, **kw)
        print("stream %s: %s of %d cells" % (more, mine["stats"], mine["d2"].size))
        if not more:
            assert mine["stats"]["n_basis2"] > 0 and mine["stats"]["n_basis3"] + mine["stats"]["n_basis4"] > 0 and mine["stats"]["n_listed"] > 0
        assert_same(got, mine, ("stream / download_block", more))
        assert_same(got, replica(st.cfg, blocks_of(st, "ora"), *rq, **kw), ("stream / oracle", more))


def test_device_form_equals_the_host_form(stream):
    st = stream
    rq, kw = stream_request(st)
    host = st.ctx.voronoi_field(*rq, **kw)
    shapes = shapes_of(host)
    assert shapes["l"][0] > 0
    # the host form leaves the guard entries alone, whichever outputs are asked for; each output alone, then all
    for fields in [[k] for k in NAMES] + [NAMES]:
        out = guarded(shapes, fields)
        assert st.ctx.voronoi_field_into(out) == 0
        for k in fields:
            n = host[k].size
            assert out[k][:n].tobytes() == host[k].tobytes() and (out[k][n:] == 7).all() and len(out[k]) > n, (fields, k)
    assert st.ctx.voronoi_field_into({}) == 0
    # device pointers: copied device-to-device in stream order (khr_sync, then the same bytes)
    for fields in [NAMES] + [[k] for k in NAMES] + [[]]:
        dev = {k: DeviceArray(v) for k, v in guarded(shapes, fields, fill=9).items()}
        assert st.ctx.voronoi_field_into({k: d.data_ptr() for k, d in dev.items()}, on_device=True) == 0
        st.ctx.sync()
        for k, dt, sh, _ in FIELDS:
            if k in dev:
                nbytes = host[k].size * np.dtype(dt).itemsize
                tail = GUARD * int(np.prod(sh + (1,)))
                assert dev[k].read(0, nbytes).tobytes() == host[k].tobytes(), (fields, k)
                assert (dev[k].read(nbytes, tail * np.dtype(dt).itemsize).view(dt) == 9).all(), (fields, k)
                dev[k].free()


def test_into_without_a_result_is_a_state_error():
    cfg = default_config(voxels_per_side=16, max_blocks=64, max_frame_pixels=64 * 48, **mc.CONFIG)
    ctx = FusionContext(cfg)
    out = guarded({"d": (2, 2, 2), "l": (3,)}, NAMES)
    assert ctx.voronoi_field_into(out) == KHR_ESTATE and all((a == 7).all() for a in out.values())
    # a call that fails its argument checks leaves no result behind either
    rc, stats = ctx.voronoi_field_rc(ctx.voronoi_request((0, 0, 0), (2, 2, 2), ratio=3))
    assert rc == KHR_EINVAL and not any(stats.values())
    assert ctx.voronoi_field_into(out) == KHR_ESTATE and all((a == 7).all() for a in out.values())
    # an empty map answers: nothing observed, no obstacle, no site
    got = ctx.voronoi_field((0, 0, 0), (2, 2, 2))
    assert not any(got["stats"].values()) and (got["site"] == -1).all() and ctx.voronoi_field_into(out) == 0
    # reset_map and load_map discard the result
    ctx.reset_map(cfg.voxel_size, cfg.truncation_distance)
    assert ctx.voronoi_field_into(out) == KHR_ESTATE
    ctx.voronoi_field((0, 0, 0), (2, 2, 2))
    indices, layers = dc.wall(16)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    assert ctx.voronoi_field_into(out) == KHR_ESTATE
    ctx.close()


def test_the_call_only_reads_and_repeats_identically(stream):
    st = stream
    digest, idx, stats = st.ctx.map_digest(), st.ctx.block_indices().copy(), st.ctx.stats()
    rq, kw = stream_request(st)
    a, b = st.ctx.voronoi_field(*rq, **kw), st.ctx.voronoi_field(*rq, **kw)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"] == b["stats"]
    # a small box after a large one: the buffers keep their size, the small box uses their front
    origin = rq[0]
    small = ((origin[0] + 11, origin[1] + 9, origin[2] + 5), (13, 17, 9))
    for more in ({}, dict(unknown_is_obstacle=True)):
        k2 = dict(kw, **more)
        assert_same(st.ctx.voronoi_field(*small, *rq[2:], **k2), replica(st.cfg, blocks_of(st, "ctx"), *small, *rq[2:], **k2), ("small after large", more))
    # the distance field uses the same seed grid and is what it was
    df = st.ctx.distance_field(*rq)
    want = dr.distance_field(blocks_of(st, "ctx"), st.cfg.voxel_size, *rq, st.cfg.mesh_min_weight)
    assert all(df[k].tobytes() == want[k].tobytes() for k in dr.FIELDS) and df["stats"] == want["stats"]
    assert np.array_equal(st.ctx.map_digest(), digest)
    assert np.array_equal(st.ctx.block_indices(), idx)
    assert st.ctx.stats() == stats


def test_error_codes_keep_the_earlier_result(stream):
    """every KHR_EINVAL case, and a shard's KHR_ESTATE: nothing is done -- the earlier result stays what it was and the caller's
    buffers are only written by the khr_voronoi_field_into that follows, inside their bounds.  (The failures that discard a result,
    KHR_ENOMEM and device errors, cannot be had on purpose.)"""
    st = stream
    rq, kw = stream_request(st)
    host = st.ctx.voronoi_field(*rq, **kw)
    shapes = shapes_of(host)
    good = dict(origin=(-3, -3, -3), dims=(6, 6, 6), ratio=1, max_distance=1.0)
    nan, inf = float("nan"), float("inf")
    big = 1 << 30
    cases = {
        "zero dim": dict(dims=(6, 0, 6)), "negative dim": dict(dims=(-1, 6, 6)), "dim 513": dict(dims=(6, 6, 513)),
        "more than 2^24 cells": dict(dims=(512, 512, 65)), "ratio 0": dict(ratio=0), "ratio 3": dict(ratio=3), "ratio 8": dict(ratio=8),
        "box above the index range": dict(origin=(big - 3, 0, 0)), "box below the index range": dict(origin=(0, -big, 0)),
        "nan surface_distance": dict(surface_distance=nan), "inf surface_distance": dict(surface_distance=-inf),
        "negative min_weight": dict(min_weight=-1.0), "nan min_weight": dict(min_weight=nan), "inf min_weight": dict(min_weight=inf),
        "zero max_distance": dict(max_distance=0.0), "nan max_distance": dict(max_distance=nan), "inf max_distance": dict(max_distance=inf),
        "a range of 32768 cells": dict(max_distance=3277.0),
        "negative min_distance": dict(min_distance=-0.1), "nan min_distance": dict(min_distance=nan), "inf min_distance": dict(min_distance=inf),
        "mode 3": dict(mode=3), "mode -1": dict(mode=-1),
        "l1 separation 0": dict(mode=vr.L1, parent_l1_separation=0), "l1 separation 0, then angle": dict(mode=vr.L1_THEN_ANGLE, parent_l1_separation=0),
        "cos 1.5": dict(mode=vr.ANGLE, parent_cos_angle_separation=1.5), "cos -1.5": dict(mode=vr.L1_THEN_ANGLE, parent_cos_angle_separation=-1.5),
        "nan cos": dict(mode=vr.ANGLE, parent_cos_angle_separation=nan),
        "min_basis 1": dict(min_basis=1), "min_basis 5": dict(min_basis=5), "min_basis -2": dict(min_basis=-2),
    }
    for what, more in cases.items():
        rc, stats = st.ctx.voronoi_field_rc(st.ctx.voronoi_request(**dict(good, **more)))
        assert rc == KHR_EINVAL and not any(stats.values()), (what, rc)
        out = guarded(shapes, ["site", "cell_sites"])
        assert st.ctx.voronoi_field_into(out) == 0, what
        for k, a in out.items():
            n = host[k].size
            assert a[:n].tobytes() == host[k].tobytes() and (a[n:] == 7).all(), (what, k)
    rc, stats = st.ctx.voronoi_field_rc(None)
    assert rc == KHR_EINVAL
    # a parameter the mode does not use is not looked at; the edges of the valid ranges are fine
    for more in (dict(mode=vr.ANGLE, parent_l1_separation=0), dict(mode=vr.L1, parent_cos_angle_separation=nan), dict(mode=vr.ANGLE, parent_cos_angle_separation=-1.0),
                 dict(mode=vr.ANGLE, parent_cos_angle_separation=1.0), dict(min_basis=0), dict(min_basis=4), dict(min_distance=0.0), dict(max_distance=3276.0)):
        rc, stats = st.ctx.voronoi_field_rc(st.ctx.voronoi_request(**dict(good, **more)))
        assert rc == 0, more
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=64 * 48, rank=0, world_size=2)
    shard = FusionContext(cfg)
    rc, stats = shard.voronoi_field_rc(shard.voronoi_request(**good))
    assert rc == KHR_ESTATE and not any(stats.values())
    out = guarded({"d": (6, 6, 6), "l": (1,)}, NAMES)
    assert shard.voronoi_field_into(out) == KHR_ESTATE and all((a == 7).all() for a in out.values())
    shard.close()


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
      positive_distance_only: true
      min_basis_for_extraction: 1
      voronoi_config:
        mode: L1_THEN_ANGLE
        min_distance_m: 0.30
        parent_l1_separation: 20
        parent_cos_angle_separation: 0.2
    tsdf_interpolator:
      type: downsample
      ratio: 2
"""


def test_aw_demo_voronoi_mode_checks_the_field_on_the_host(tmp_path):
    """aw_demo --voronoi: a Khronos sink asks for the Voronoi field of a box around the sensor through VolumetricMap::voronoiField and
    checks, from the returned arrays alone, the sites, their distances, the basis rule and the list"""
    W, H, N = 320, 240, 8
    cfgp = tmp_path / "aw_voronoi.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--voronoi", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["frames"] == N and res["agree_frames"] == N and res["first_mismatch"] == ""
    assert res["cells"] > 0 and res["n_listed"] > 0 and res["last_stats"]["n_eligible"] > 0 and res["device_ms"] > 0


def test_the_result_survives_later_frames_and_archival(stream):
    """(last: it moves the shared stream on) the result of a call stays what it was across two further frames and a reset_inactive()"""
    st = stream
    rq, kw = stream_request(st)
    host = st.ctx.voronoi_field(*rq, **kw)
    for i in range(N_FRAMES, N_FRAMES + 2):
        step(st, i)
    assert np.array_equal(np.asarray(st.ctx.reset_inactive()), np.asarray(st.ora.reset_inactive()))
    st.cache.clear()
    out = {k: np.zeros(host[k].shape, dt) for k, dt, _, _ in FIELDS}
    assert st.ctx.voronoi_field_into(out) == 0
    for k in NAMES:
        assert out[k].tobytes() == host[k].tobytes(), k
    # and a new call sees the new map
    now = st.ctx.voronoi_field(*rq, **kw)
    assert_same(now, replica(st.cfg, blocks_of(st, "ctx"), *rq, **kw), "after two frames and archival")
