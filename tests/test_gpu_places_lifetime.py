"""khr_places_graph's buffers -- the device copy of a host field, the per-cell work arrays, the work lists, the scan's and sort's
storage, the result lists, the counters with their page-locked mirror, the page-locked staging -- have owners: the counts of
khr_debug_live_resources rise with the first calls, stay put when a larger box grows the buffers in place, and return to where they
were after close() (tests/test_gpu_resource_lifetime.py explains the counts).  The result stays what it was across later frames and
is discarded by reset_map, load_map and -- for the form that reads the Voronoi result -- a new Voronoi field."""
import gc

import numpy as np
import pytest

import distance_cases as dc
import mesh_cases as mc
import places_cases as pc
import places_replica as pr
from common import DeviceArray, make_pair, step_both
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_ESTATE, KHR_VOR_L1, live_resources

pytestmark = pytest.mark.gpu
NAMES = [k for k, _, _, _ in FusionContext.PL_FIELDS]


def test_a_context_that_answered_places_graphs_leaves_nothing():
    gc.collect()
    start = live_resources()
    cfg = default_config(voxels_per_side=16, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
    ctx = FusionContext(cfg)
    indices, layers = dc.random(16)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    origin, _ = dc.box_of("random", 16, 1)
    dims = (20, 12, 16)
    kw = dict(max_distance=100.0, min_distance=0.2, mode=KHR_VOR_L1, parent_l1_separation=4)
    field = ctx.voronoi_field(origin, dims, 1, **kw)
    before = live_resources()
    host = ctx.places_graph(compression=3)
    assert host["stats"]["n_places"] > 1 and host["stats"]["n_edges"] > 0
    n = int(np.prod(dims))
    d = DeviceArray(np.zeros(n, np.int32))
    assert ctx.places_graph_into({"place": d.data_ptr()}, on_device=True) == 0
    ctx.sync()
    assert d.read(0, 4 * n).tobytes() == host["place"].tobytes()
    d.free()
    again = ctx.places_graph_from(origin, dims, field["distance"], field["d2"], field["basis"], field["site"], compression=3)
    assert all(again[k].tobytes() == host[k].tobytes() for k in NAMES) and again["stats"] == host["stats"]
    now = live_resources()
    # the work arrays, the work lists, the temporary storage, the result, the counters, the copy of a host field; the counters' mirror
    # and the host staging
    assert now[0] >= before[0] + 6 and now[1] >= before[1] + 2 and now[2:] == before[2:], (start, before, now)
    # a larger box, with more places, grows all of them in place: no further owners
    larger_field = ctx.voronoi_field(tuple(o - 8 for o in origin), tuple(v + 16 for v in dims), 1, **kw)
    larger = ctx.places_graph(compression=1)
    assert larger["stats"]["n_places"] > host["stats"]["n_places"]
    o2, d2 = tuple(o - 8 for o in origin), tuple(v + 16 for v in dims)
    ctx.places_graph_from(o2, d2, larger_field["distance"], larger_field["d2"], larger_field["basis"], larger_field["site"], compression=1)
    assert live_resources() == now
    # an empty graph keeps its owners too
    assert ctx.places_graph(min_node_distance=1000.0)["stats"]["n_members"] == 0
    assert live_resources() == now
    ctx.close()
    assert live_resources() == start


def test_the_result_survives_later_frames_and_is_discarded_with_what_it_describes():
    cfg, ctx, ora, s, sen, osen = make_pair(temporal_window=0.6)
    fr = None
    for i in range(6):
        fr = s.render(i)
        step_both(ctx, ora, sen, osen, fr, motion=bool(cfg.with_tracking), track=bool(cfg.with_tracking))
    origin, dims = dc.stream_box(fr["pose"], cfg.voxel_size)
    kw = dict(max_distance=dc.STREAM_MAX_DISTANCE, min_distance=0.2, mode=KHR_VOR_L1, parent_l1_separation=4)
    field = ctx.voronoi_field(origin, dims, dc.STREAM_RATIO, **kw)
    host = ctx.places_graph(compression=4)
    assert host["stats"]["n_members"] > 0
    want = pr.of_voronoi(field, origin, compression=4)
    assert all(host[k].tobytes() == want[k].tobytes() for k in NAMES) and host["stats"] == want["stats"]

    def fetch():
        out = {k: np.zeros_like(host[k]) for k in NAMES}
        rc = ctx.places_graph_into(out)
        return rc, out

    # two further frames and an archival: the result is what it was
    for i in range(6, 8):
        step_both(ctx, ora, sen, osen, s.render(i), motion=bool(cfg.with_tracking), track=bool(cfg.with_tracking))
    ctx.reset_inactive(), ora.reset_inactive()
    rc, out = fetch()
    assert rc == 0 and all(out[k].tobytes() == host[k].tobytes() for k in NAMES)
    # a new Voronoi field discards the graph that was read from the old one ...
    ctx.voronoi_field(origin, dims, dc.STREAM_RATIO, **kw)
    assert fetch()[0] == KHR_ESTATE
    # ... but not a graph of a field the caller brought
    o, d, f, pkw, _ = dict(pc.SYNTHETIC)["65x3x2"]()
    own = ctx.places_graph_from(o, d, f["distance"], f["d2"], f["basis"], f["site"], **pkw)
    ctx.voronoi_field(origin, dims, dc.STREAM_RATIO, **kw)
    got = {k: np.zeros_like(own[k]) for k in NAMES}
    assert ctx.places_graph_into(got) == 0 and all(got[k].tobytes() == own[k].tobytes() for k in NAMES)
    # reset_map discards both results
    ctx.reset_map(cfg.voxel_size, cfg.truncation_distance)
    assert ctx.places_graph_into(got) == KHR_ESTATE and ctx.places_graph_rc(ctx.places_request())[0] == KHR_ESTATE
    ctx.close()
    # load_map too
    cfg = default_config(voxels_per_side=16, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
    ctx = FusionContext(cfg)
    ctx.places_graph_from(o, d, f["distance"], f["d2"], f["basis"], f["site"], **pkw)
    assert ctx.places_graph_into(got) == 0
    indices, layers = dc.wall(16)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    assert ctx.places_graph_into(got) == KHR_ESTATE
    ctx.close()
