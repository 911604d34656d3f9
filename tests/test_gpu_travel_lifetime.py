"""khr_travel_field's buffers -- the device copy of a host field and goals, the per-cell keys, masks, flags and result arrays, the
counters with their page-locked mirror, the page-locked staging, the per-start arrays, the scan's storage and the path cells -- have
owners: the counts of khr_debug_live_resources rise with the first calls, stay put when a larger box grows the buffers in place or a
smaller one reuses them, and return to where they were after close() (tests/test_gpu_resource_lifetime.py explains the counts).  The
result stays what it was across later frames and is discarded by reset_map, load_map and -- for the form that reads the Voronoi
result -- a new Voronoi field."""
import gc

import numpy as np
import pytest

import distance_cases as dc
import mesh_cases as mc
import travel_cases as tc
import travel_replica as tr
from common import make_pair, step_both
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_ESTATE, KHR_VOR_L1, live_resources

pytestmark = pytest.mark.gpu
NAMES = [k for k, _ in FusionContext.TF_FIELDS]


def same(got, want):
    return all(got[k].tobytes() == want[k].tobytes() for k in NAMES) and all(got["stats"][k] == want["stats"][k] for k in tr.RESULT_STATS)


def from_case(ctx, c, connectivity=26):
    return ctx.travel_field(c["goals"], connectivity=connectivity, field=(c["origin"], c["dims"], c["distance"], c["status"]), **c["kw"])


def test_a_context_that_answered_travel_fields_leaves_nothing():
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
    free = np.argwhere((field["status"] & 3) == 1)
    assert len(free) > 10
    goals = (free[[0, -1]][:, ::-1] + np.asarray(origin)).astype(np.int32)
    before = live_resources()
    host = ctx.travel_field(goals, 0.0)
    assert host["stats"]["n_reached"] > 1
    assert same(host, tr.travel_field(origin, field["distance"], field["status"], goals, 0.0))
    paths = ctx.travel_paths(goals)
    assert np.diff(paths["offsets"]).tolist() == [1, 1]
    again = ctx.travel_field(goals, 0.0, field=(origin, dims, field["distance"], field["status"]))
    assert same(again, host)
    ctx.travel_paths(goals)
    now = live_resources()
    # the per-cell arrays, the counters, the copy of a host field and goals, the per-start arrays, the scan's storage, the path cells;
    # the counters' mirror and the host staging
    assert now[0] >= before[0] + 6 and now[1] >= before[1] + 2 and now[2:] == before[2:], (start, before, now)
    # a larger box grows all of them in place, a smaller one reuses them: no further owners
    for name in ("random", "tie", "open", "random", "pocket"):
        c = tc.built(name)
        assert same(from_case(ctx, c), tc.expected(name, 26)), name
        ctx.travel_paths(np.concatenate([c["goals"]] * 50))
        assert live_resources() == now, name
    # repeated calls on the Voronoi field, and a result without a reached cell
    for _ in range(3):
        assert same(ctx.travel_field(goals, 0.0), host)
    assert ctx.travel_field(goals, 1000.0)["stats"]["n_traversable"] == 0
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
    free = np.argwhere(((field["status"] & 3) == 1) & (field["distance"] >= 0.2))
    assert len(free) > 10
    goals = (free[[len(free) // 2]][:, ::-1] + np.asarray(origin)).astype(np.int32)
    host = ctx.travel_field(goals, 0.2)
    assert host["stats"]["n_reached"] > 10
    assert same(host, tr.travel_field(origin, field["distance"], field["status"], goals, 0.2))
    starts = (free[[0, -1]][:, ::-1] + np.asarray(origin)).astype(np.int32)
    paths = ctx.travel_paths(starts)

    def fetch():
        out = {k: np.zeros_like(host[k]) for k in NAMES}
        p = {k: np.zeros_like(paths[k]) for k in ("offsets", "cells", "path_cost", "path_goal")}
        return ctx.travel_field_into(out), out, ctx.travel_paths_into(p), p

    # two further frames and an archival: the result is what it was
    for i in range(6, 8):
        step_both(ctx, ora, sen, osen, s.render(i), motion=bool(cfg.with_tracking), track=bool(cfg.with_tracking))
    ctx.reset_inactive(), ora.reset_inactive()
    rc, out, prc, p = fetch()
    assert rc == 0 and all(out[k].tobytes() == host[k].tobytes() for k in NAMES)
    assert prc == 0 and all(p[k].tobytes() == paths[k].tobytes() for k in p)
    # a new Voronoi field discards the travel field that was read from the old one, and its paths ...
    ctx.voronoi_field(origin, dims, dc.STREAM_RATIO, **kw)
    rc, _, prc, _ = fetch()
    assert rc == KHR_ESTATE and prc == KHR_ESTATE
    # ... but not a travel field of a field the caller brought
    c = tc.built("wall_negative_origin")
    own = from_case(ctx, c)
    ctx.voronoi_field(origin, dims, dc.STREAM_RATIO, **kw)
    got = {k: np.zeros_like(own[k]) for k in NAMES}
    assert ctx.travel_field_into(got) == 0 and all(got[k].tobytes() == own[k].tobytes() for k in NAMES)
    # reset_map discards both results
    ctx.reset_map(cfg.voxel_size, cfg.truncation_distance)
    assert ctx.travel_field_into(got) == KHR_ESTATE and ctx.travel_field_rc(ctx.travel_request(), c["goals"])[0] == KHR_ESTATE
    assert ctx.travel_paths_rc(c["goals"])[0] == KHR_ESTATE
    ctx.close()
    # load_map too
    cfg = default_config(voxels_per_side=16, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
    ctx = FusionContext(cfg)
    from_case(ctx, c)
    assert ctx.travel_field_into(got) == 0
    indices, layers = dc.wall(16)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    assert ctx.travel_field_into(got) == KHR_ESTATE
    ctx.close()
