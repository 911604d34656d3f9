"""khr_places_graph / khr_places_graph_from (ASSUMPTIONS.md A.21): every array and every counter held byte for byte to
tests/places_replica.py -- after khr_voronoi_field on the hand-built maps of tests/voronoi_cases.py and tests/distance_cases.py and on
the 30-frame stream, and on the synthetic member sets of tests/places_cases.py through host and device inputs; the hand counts of
tests/places_cases.py stand on top.  The calls only read: the Voronoi result and the map digest are what they were."""
import json
import os
import subprocess

import numpy as np
import pytest

import distance_cases as dc
import mesh_cases as mc
import places_cases as pc
import places_replica as pr
import query_replica as qr
import voronoi_cases as vc
import voronoi_replica as vr
from common import DeviceArray, make_pair, step_both
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ESTATE

pytestmark = pytest.mark.gpu
f32 = np.float32
FIELDS = FusionContext.PL_FIELDS
NAMES = [k for k, _, _, _ in FIELDS]
VOR_NAMES = [k for k, _, _, _ in FusionContext.VOR_FIELDS]
GUARD = 64  # entries after each output buffer that a call must leave alone
N_FRAMES = 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
_maps = {}


def load(key, vps, indices, layers):
    if key not in _maps:
        cfg = default_config(voxels_per_side=vps, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
        ctx = FusionContext(cfg)
        assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
        _maps[key] = (cfg, ctx)
    return _maps[key]


def bare():
    """a context without a map, for khr_places_graph_from"""
    if "bare" not in _maps:
        cfg = default_config(voxels_per_side=16, max_blocks=64, max_frame_pixels=64 * 48, **mc.CONFIG)
        _maps["bare"] = (cfg, FusionContext(cfg))
    return _maps["bare"][1]


def assert_same(got, want, what):
    for k, dt, _, _ in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), [got[k][tuple(b)].item() for b in bad[:4]], [want[k][tuple(b)].item() for b in bad[:4]]))
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    n = np.maximum(got["n_cells"], 1).astype(np.float64)[:, None]
    assert got["centroid"].tobytes() == (want["sum"].astype(np.float64) / n).tobytes()


def shapes_of(out):
    return {"d": out["place"].shape, "p": (len(out["n_cells"]),), "e": (len(out["edge_a"]),)}


def guarded(shapes, fields, fill=7):
    return {k: np.full(int(np.prod(shapes[w] + sh)) + GUARD * int(np.prod(sh + (1,))), fill, dt) for k, dt, sh, w in FIELDS if k in fields}


def voronoi_bytes(ctx, field):
    out = {k: np.zeros_like(field[k]) for k in VOR_NAMES}
    assert ctx.voronoi_field_into(out) == 0
    return {k: out[k].tobytes() for k in VOR_NAMES}


@pytest.mark.parametrize("key", ["even", "odd", "posts"])
def test_corridors_and_posts_give_their_hand_counts(key):
    case = pc.voronoi_case(key)
    indices, layers, origin, dims, _ = case
    cfg, ctx = load(key, vc.VPS, indices, layers)
    cell = float(f32(mc.VOXEL_SIZE))
    digest = ctx.map_digest()
    field = ctx.voronoi_field(origin, dims, 1, 100.0, min_distance=vc.MIN_DISTANCE_CELLS * cell, **pc.VORONOI_KW)
    before = {k: field[k].tobytes() for k in VOR_NAMES}
    ctx.places_graph()
    assert ctx.places_graph_box() == (tuple(origin), tuple(dims))   # the Voronoi field's box, as the context remembers it
    for (k, compression, min_size), (places, sizes, edges) in sorted(pc.VORONOI_COUNTS.items()):
        if k != key:
            continue
        got = ctx.places_graph(compression=compression, min_component_size=min_size)
        assert_same(got, pr.of_voronoi(field, origin, compression=compression, min_component_size=min_size), (key, compression, min_size))
        assert got["stats"]["n_places"] == places and got["stats"]["n_edges"] == edges, (key, compression, min_size, got["stats"])
        if sizes is not None:
            assert sorted(got["n_cells"].tolist()) == sizes
    for kw in (dict(compression=3, min_basis=3), dict(compression=2, min_node_distance=3.5 * cell), dict(compression=16, min_basis=4, min_component_size=-2)):
        assert_same(ctx.places_graph(**kw), pr.of_voronoi(field, origin, **kw), (key, kw))
    # the Voronoi result is only read, the map is not touched
    assert voronoi_bytes(ctx, field) == before
    assert np.array_equal(ctx.map_digest(), digest)


@pytest.mark.parametrize("ratio", [1, 2, 4])
@pytest.mark.parametrize("vps", [16, 8])
@pytest.mark.parametrize("name", ["wall", "random"])
def test_hand_built_maps_match_the_replica_byte_for_byte(name, vps, ratio):
    cfg, ctx = load((name, vps), vps, *dc.CASES[name](vps))
    origin, dims = dc.box_of(name, vps, ratio)
    cell = float(f32(cfg.voxel_size) * f32(ratio))
    field = ctx.voronoi_field(origin, dims, ratio, 100.0, min_distance=vc.MIN_DISTANCE_CELLS * cell, unknown_is_obstacle=(name == "wall"), **pc.VORONOI_KW)
    before = {k: field[k].tobytes() for k in VOR_NAMES}
    for kw in (dict(compression=4), dict(compression=7, min_component_size=3), dict(compression=1, min_node_distance=2.5 * cell), dict(compression=16, min_basis=3)):
        got = ctx.places_graph(**kw)
        print(name, vps, ratio, kw, got["stats"])
        assert_same(got, pr.of_voronoi(field, origin, **kw), (name, vps, ratio, kw))
    assert voronoi_bytes(ctx, field) == before


@pytest.mark.parametrize("name,build", pc.SYNTHETIC, ids=[n for n, _ in pc.SYNTHETIC])
def test_synthetic_member_sets_through_host_and_device_inputs(name, build):
    origin, dims, f, kw, exp = build()
    ctx = bare()
    want = pr.places_graph(origin, dims, f["distance"], f["d2"], f["basis"], f["site"], **kw)
    got = ctx.places_graph_from(origin, dims, f["distance"], f["d2"], f["basis"], f["site"], **kw)
    assert_same(got, want, (name, "host"))
    st = got["stats"]
    if "places" in exp:
        assert st["n_places"] == exp["places"] and st["n_edges"] == exp["edges"], st
    if "sizes" in exp:
        assert sorted(got["n_cells"].tolist()) == exp["sizes"]
    if "components" in exp:
        assert st["n_components"] == exp["components"]
    if "first" in exp:
        x, y, z = exp["first"]
        assert got["place"][z, y, x] == 0
    if "sites" in exp:   # a site outside [0, nx ny nz) gives zeros, like -1
        assert [tuple(int(v) for v in row) for row in got["site"]] == exp["sites"]
    if "centre" in exp:
        assert tuple(got["centre"][0]) == exp["centre"] and got["centre_d2"][0] == exp["centre_d2"]
    if "chain" in exp:
        deg = got["degree"][[int(got["place"][z, y, x]) for x, y, z in exp["chain"]]]
        assert deg[0] == deg[-1] == 1 and (deg[1:-1] == 2).all()
    dev = {k: DeviceArray(np.ascontiguousarray(f[k], dt)) for k, dt in FusionContext.PL_INPUTS}
    got = ctx.places_graph_from(origin, dims, *[dev[k].data_ptr() for k, _ in FusionContext.PL_INPUTS], on_device=True, **kw)
    ctx.sync()
    assert_same(got, want, (name, "device"))
    # a second request on the same field: the filter, and another compression
    for more in (dict(min_component_size=2), dict(compression=max(1, kw["compression"] // 2))):
        k2 = dict(kw, **more)
        got = ctx.places_graph_from(origin, dims, *[dev[k].data_ptr() for k, _ in FusionContext.PL_INPUTS], on_device=True, **k2)
        assert_same(got, pr.places_graph(origin, dims, f["distance"], f["d2"], f["basis"], f["site"], **k2), (name, k2))
    ctx.sync()
    for d in dev.values():
        d.free()


@pytest.mark.parametrize("compression", pc.RANDOM_COMPRESSIONS)
def test_the_random_field_filters_renumbers_and_compacts(compression):
    if "random_field" not in _maps:
        _maps["random_field"] = pc.random_field()
    f, ctx = _maps["random_field"], bare()
    for min_size in pc.RANDOM_SIZES:
        kw = dict(compression=compression, min_component_size=min_size, min_node_distance=pc.RANDOM_MIN_NODE_DISTANCE)
        got = ctx.places_graph_from(pc.RANDOM_ORIGIN, pc.RANDOM_DIMS, f["distance"], f["d2"], f["basis"], f["site"], **kw)
        assert_same(got, pr.of_voronoi(f, pc.RANDOM_ORIGIN, **kw), kw)
        assert got["stats"]["n_components_all"] == pc.RANDOM_COMPONENTS
        assert got["stats"]["n_components"] == (pc.RANDOM_COMPONENTS if min_size == 1 else pc.RANDOM_KEPT[compression])


def test_into_twice_with_guards_in_host_and_device_form():
    origin, dims, f, kw, _ = dict(pc.SYNTHETIC)["37x21x45"]()
    ctx = bare()
    host = ctx.places_graph_from(origin, dims, f["distance"], f["d2"], f["basis"], f["site"], **kw)
    shapes = shapes_of(host)
    assert shapes["p"][0] > 0 and shapes["e"][0] > 0
    assert ctx.places_graph_box() == (tuple(origin), tuple(dims))
    for fields in [NAMES, NAMES] + [[k] for k in NAMES]:
        out = guarded(shapes, fields)
        assert ctx.places_graph_into(out) == 0
        for k in fields:
            n = host[k].size
            assert out[k][:n].tobytes() == host[k].tobytes() and (out[k][n:] == 7).all() and len(out[k]) > n, (fields, k)
    assert ctx.places_graph_into({}) == 0
    for fields in [NAMES, [NAMES[0], NAMES[7], NAMES[-1]], []]:
        dev = {k: DeviceArray(v) for k, v in guarded(shapes, fields, fill=9).items()}
        assert ctx.places_graph_into({k: d.data_ptr() for k, d in dev.items()}, on_device=True) == 0
        ctx.sync()
        for k, dt, sh, _ in FIELDS:
            if k in dev:
                nbytes = host[k].size * np.dtype(dt).itemsize
                tail = GUARD * int(np.prod(sh + (1,)))
                assert dev[k].read(0, nbytes).tobytes() == host[k].tobytes(), (fields, k)
                assert (dev[k].read(nbytes, tail * np.dtype(dt).itemsize).view(dt) == 9).all(), (fields, k)
                dev[k].free()


def test_error_codes_keep_the_earlier_result():
    """every KHR_EINVAL / KHR_ESTATE case: nothing is done, the earlier result stays what it was.  (Argument checks only: the failures
    that discard a result, KHR_ENOMEM and device errors, cannot be had on purpose.)"""
    origin, dims, f, kw, _ = dict(pc.SYNTHETIC)["65x3x2"]()
    cfg = default_config(voxels_per_side=16, max_blocks=64, max_frame_pixels=64 * 48, **mc.CONFIG)
    ctx = FusionContext(cfg)
    out = guarded({"d": (2, 2, 2), "p": (3,), "e": (3,)}, NAMES)
    assert ctx.places_graph_into(out) == KHR_ESTATE and all((a == 7).all() for a in out.values())
    assert ctx.lib.khr_places_graph_box(ctx.h, None, None) == KHR_ESTATE
    # no Voronoi result: a state error, and still no result
    rc, stats = ctx.places_graph_rc(ctx.places_request())
    assert rc == KHR_ESTATE and not any(stats.values())
    assert ctx.places_graph_into(out) == KHR_ESTATE
    host = ctx.places_graph_from(origin, dims, f["distance"], f["d2"], f["basis"], f["site"], **kw)
    shapes = shapes_of(host)

    def intact(what):
        got = guarded(shapes, ["place", "sum", "edge_b"])
        assert ctx.places_graph_into(got) == 0, what
        for k, a in got.items():
            n = host[k].size
            assert a[:n].tobytes() == host[k].tobytes() and (a[n:] == 7).all(), (what, k)

    nan, inf = float("nan"), float("inf")
    bad_requests = {"min_basis 1": dict(min_basis=1), "min_basis 5": dict(min_basis=5), "min_basis -1": dict(min_basis=-1), "compression 0": dict(compression=0),
                    "compression 17": dict(compression=17), "compression -4": dict(compression=-4), "negative distance": dict(min_node_distance=-0.1),
                    "nan distance": dict(min_node_distance=nan), "inf distance": dict(min_node_distance=inf)}
    for what, more in bad_requests.items():
        rq = ctx.places_request(**more)
        rc, stats = ctx.places_graph_from_rc(rq, origin, dims, f)
        assert rc == KHR_EINVAL and not any(stats.values()), (what, rc)
        rc, stats = ctx.places_graph_rc(rq)   # (the request is looked at before the state)
        assert rc == KHR_EINVAL and not any(stats.values()), (what, rc)
        intact(what)
    good = ctx.places_request(**kw)
    big = 1 << 30
    bad_boxes = {"zero dim": (origin, (65, 0, 2)), "negative dim": (origin, (-1, 3, 2)), "dim 513": (origin, (513, 1, 1)), "more than 2^24 cells": (origin, (512, 512, 65)),
                 "box above the index range": ((big - 3, 0, 0), dims), "box below the index range": ((0, -big, 0), dims), "no origin": (None, dims),
                 "no dims": (origin, None)}
    for what, (o, d) in bad_boxes.items():
        rc, stats = ctx.places_graph_from_rc(good, o, d, f)
        assert rc == KHR_EINVAL and not any(stats.values()), (what, rc)
        intact(what)
    for k, _ in FusionContext.PL_INPUTS:
        rc, stats = ctx.places_graph_from_rc(good, origin, dims, dict(f, **{k: None}))
        assert rc == KHR_EINVAL, k
        intact(k)
    assert ctx.places_graph_from_rc(None, origin, dims, f)[0] == KHR_EINVAL and ctx.places_graph_rc(None)[0] == KHR_EINVAL
    rc, _ = ctx.places_graph_rc(good)
    assert rc == KHR_ESTATE   # still no Voronoi result
    intact("no voronoi result")
    # the edges of the valid ranges are fine
    for more in (dict(min_basis=0), dict(min_basis=4), dict(compression=1), dict(compression=16), dict(min_node_distance=0.0), dict(min_component_size=-5)):
        rc, _ = ctx.places_graph_from_rc(ctx.places_request(**more), origin, dims, f)
        assert rc == 0, more
    shard = FusionContext(default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=64 * 48, rank=0, world_size=2))
    rc, stats = shard.places_graph_from_rc(good, origin, dims, f)
    assert rc == KHR_ESTATE and not any(stats.values())
    assert shard.places_graph_rc(good)[0] == KHR_ESTATE and shard.places_graph_into(out) == KHR_ESTATE and all((a == 7).all() for a in out.values())
    shard.close()
    ctx.close()


# ---- the stream map ------------------------------------------------------------------------------------------------------------
def test_the_stream_map_over_this_contexts_blocks():
    """the stream of tests/test_gpu_voronoi_field.py: the Voronoi field of the replica over this context's block downloads, the places
    of the replica over that field, against the two device calls"""
    cfg, ctx, ora, s, sen, osen = make_pair(temporal_window=0.6)
    last = None
    for i in range(N_FRAMES):
        last = s.render(i)
        step_both(ctx, ora, sen, osen, last, motion=bool(cfg.with_tracking), track=bool(cfg.with_tracking))
        if i % 5 == 4:
            assert np.array_equal(np.asarray(ctx.reset_inactive()), np.asarray(ora.reset_inactive()))
    origin, dims = dc.stream_box(last["pose"], cfg.voxel_size)
    kw = dict(vc.STREAM)
    ratio, max_distance = kw.pop("ratio"), kw.pop("max_distance")
    kw["min_distance"] = vc.MIN_DISTANCE_CELLS * float(f32(cfg.voxel_size) * f32(ratio))
    blocks = qr.QueryBlocks(ctx.block_indices(), ctx.download_block, cfg.voxels_per_side)
    field = vr.voronoi_field(blocks, cfg.voxel_size, origin, dims, ratio, max_distance, cfg.mesh_min_weight, **kw)
    digest, stats = ctx.map_digest(), ctx.stats()
    got_field = ctx.voronoi_field(origin, dims, ratio, max_distance, **kw)
    for k in VOR_NAMES:
        assert got_field[k].tobytes() == field[k].tobytes(), k
    for more in (dict(compression=4), dict(compression=7, min_component_size=3), dict(compression=1), dict(compression=16, min_basis=3)):
        got = ctx.places_graph(**more)
        print("stream %s: %s" % (more, got["stats"]))
        assert_same(got, pr.of_voronoi(field, origin, **more), ("stream", more))
        if more == dict(compression=4):
            assert got["stats"]["n_places"] >= 2 and got["stats"]["n_edges"] >= 1
    assert voronoi_bytes(ctx, field) == {k: field[k].tobytes() for k in VOR_NAMES}
    assert np.array_equal(ctx.map_digest(), digest) and ctx.stats() == stats
    ctx.close()


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
    filter_places: true
    min_places_component_size: 3
    gvd:
      max_distance_m: 1.5
      min_weight: 1.0e-6
      positive_distance_only: true
      min_basis_for_extraction: 1
      extract_graph: true
      voronoi_config:
        mode: L1_THEN_ANGLE
        min_distance_m: 0.30
        parent_l1_separation: 20
        parent_cos_angle_separation: 0.2
    graph:
      type: CompressionGraphExtractor
      compression_distance_m: 1.5
      min_node_distance_m: 0.4
    tsdf_interpolator:
      type: downsample
      ratio: 2
"""


def test_aw_demo_places_mode_agrees_with_the_host_flood_fill(tmp_path):
    """aw_demo --places: a Khronos sink asks for the places graph of the Voronoi field of a box around the sensor through
    VolumetricMap::placesGraph and holds it against the flood fill and pair search over the downloaded field that it replaces"""
    W, H, N = 320, 240, 8
    cfgp = tmp_path / "aw_places.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--places", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["frames"] == N and res["agree_frames"] == N and res["first_mismatch"] == ""
    assert res["cells"] > 0 and res["last_stats"]["n_members"] > 0 and res["last_stats"]["n_places_all"] > 0 and res["device_ms"] > 0
