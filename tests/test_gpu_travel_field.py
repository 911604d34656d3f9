"""khr_travel_field / khr_travel_field_from / khr_travel_paths (ASSUMPTIONS.md A.22): cost, goal, parent, the four counters that
describe the result and the paths held bit for bit to tests/travel_replica.py at connectivity 6, 18 and 26 -- on the hand-built fields
of tests/travel_cases.py through host and device inputs, with the hand numbers of that file on top, and after khr_voronoi_field on a
hand-built map, with given goals and with the place centres.  The calls only read: the Voronoi result, the places graph and the map
digest are what they were."""
import json
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import places_cases as pc
import travel_cases as tc
import travel_replica as tr
import voronoi_cases as vc
from common import DeviceArray
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ESTATE, KHR_TF_ROUNDS_PER_WAIT, KHR_TF_TILE_EDGE, KHR_TF_UNREACHED

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = [k for k, _ in FusionContext.TF_FIELDS]
VOR_NAMES = [k for k, _, _, _ in FusionContext.VOR_FIELDS]
PL_NAMES = [k for k, _, _, _ in FusionContext.PL_FIELDS]
PATH_TYPES = {"offsets": np.int64, "cells": np.int32, "path_cost": np.uint32, "path_goal": np.int32}
GUARD = 64  # entries after each output buffer that a call must leave alone
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
_ctx = {}


def bare():
    """a context without a map, for khr_travel_field_from"""
    if "bare" not in _ctx:
        cfg = default_config(voxels_per_side=16, max_blocks=64, max_frame_pixels=64 * 48, **mc.CONFIG)
        _ctx["bare"] = FusionContext(cfg)
    return _ctx["bare"]


def assert_same(got, want, what):
    for k, dt in FusionContext.TF_FIELDS:
        assert got[k].dtype == want[k].dtype == dt and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), [got[k][tuple(b)].item() for b in bad[:4]], [want[k][tuple(b)].item() for b in bad[:4]]))
    for k in tr.RESULT_STATS:
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"], want["stats"])
    # the schedule's two words: a wait per KHR_TF_ROUNDS_PER_WAIT rounds queued, and no more rounds with work than were queued
    st = got["stats"]
    assert st["n_waits"] >= 1 and st["n_rounds"] <= KHR_TF_ROUNDS_PER_WAIT * st["n_waits"], st
    assert (st["n_rounds"] == 0) == (st["n_goals_used"] == 0), st


def assert_same_paths(got, want, what):
    for k, dt in PATH_TYPES.items():
        assert got[k].dtype == want[k].dtype == dt and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k][:12].tolist(), want[k][:12].tolist())


def run_from(ctx, c, connectivity, on_device=False, **more):
    """khr_travel_field_from on a case of travel_cases, through host or device arrays -> result dict"""
    kw = dict(c["kw"], connectivity=connectivity, **more)
    rq = ctx.travel_request(**kw)
    if not on_device:
        rc, stats = ctx.travel_field_from_rc(rq, c["origin"], c["dims"], c, c["goals"])
    else:
        dev = [DeviceArray(np.ascontiguousarray(c[k], dt)) for k, dt in FusionContext.TF_INPUTS] + [DeviceArray(np.ascontiguousarray(c["goals"], np.int32))]
        rc, stats = ctx.travel_field_from_rc(rq, c["origin"], c["dims"], dict(distance=dev[0].data_ptr(), status=dev[1].data_ptr()), dev[2].data_ptr(),
                                             on_device=True, n_goals=len(c["goals"]))
        ctx.sync()
        for d in dev:
            d.free()
    assert rc == 0, (rc, kw)
    return ctx._travel_result(stats)


def some_starts(c, res, n=12, seed=5):
    """random cells of the box, the first goal, a cell that is not reached (if there is one) and two cells outside the box"""
    o = np.asarray(c["origin"])
    nx, ny, nz = c["dims"]
    rng = np.random.default_rng(seed)
    starts = [np.stack([rng.integers(0, nx, n), rng.integers(0, ny, n), rng.integers(0, nz, n)], 1) + o, c["goals"][:1], o[None] + (nx, 0, 0), o[None] - (0, 1, 0)]
    lost = np.argwhere(res["cost"] == tr.UNREACHED)
    if len(lost):
        starts.append(lost[len(lost) // 2][None, ::-1] + o)
    return np.concatenate(starts).astype(np.int32)


@pytest.mark.parametrize("connectivity", tc.CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(tc.BUILDERS))
def test_hand_built_fields_through_host_and_device_inputs(name, connectivity):
    c, want, ctx = tc.built(name), tc.expected(name, connectivity), bare()
    got = run_from(ctx, c, connectivity)
    print(name, connectivity, got["stats"])
    assert_same(got, want, (name, connectivity, "host"))
    tc.check_hand_numbers(name, connectivity, got)
    assert ctx.travel_field_box() == (tuple(c["origin"]), tuple(c["dims"]))
    starts = some_starts(c, want)
    want_paths = tr.travel_paths(c["origin"], want, starts)
    assert_same_paths(ctx.travel_paths(starts), want_paths, (name, connectivity, "host"))
    got = run_from(ctx, c, connectivity, on_device=True)
    assert_same(got, want, (name, connectivity, "device"))
    # the starts from device memory, the paths into device memory
    d_starts = DeviceArray(starts)
    rc, total = ctx.travel_paths_rc(d_starts.data_ptr(), on_device=True, n_starts=len(starts))
    assert rc == 0 and total == len(want_paths["cells"])
    dev = {k: DeviceArray(np.full(want_paths[k].size + GUARD, 9, dt)) for k, dt in PATH_TYPES.items()}
    assert ctx.travel_paths_into({k: d.data_ptr() for k, d in dev.items()}, on_device=True) == 0
    ctx.sync()
    for k, dt in PATH_TYPES.items():
        nbytes = want_paths[k].nbytes
        assert dev[k].read(0, nbytes).tobytes() == want_paths[k].tobytes(), (name, k)
        assert (dev[k].read(nbytes, GUARD * np.dtype(dt).itemsize).view(dt) == 9).all(), (name, k)
        dev[k].free()
    d_starts.free()


def test_the_walls_path_and_the_three_kinds_of_empty_paths():
    c, ctx = tc.built("wall_negative_origin"), bare()
    run_from(ctx, c, 26)
    o = np.asarray(c["origin"])
    starts = np.array([o + tc.WALL_PATH_START, o + (12, 3, 0), o + (24, 0, 0), o + (0, 0, 0)], np.int32)   # far corner, in the wall, outside, the goal
    p = ctx.travel_paths(starts)
    assert np.diff(p["offsets"]).tolist() == [tc.WALL_PATH_CELLS, 0, 0, 1]
    assert p["path_cost"].tolist() == [412, KHR_TF_UNREACHED, KHR_TF_UNREACHED, 0] and p["path_goal"].tolist() == [0, -1, -1, 0]
    assert tuple(p["paths"][0][0]) == tuple(starts[0]) and tuple(p["paths"][0][-1]) == tuple(o) and tuple(p["paths"][3][0]) == tuple(o)
    assert_same_paths(p, tr.travel_paths(c["origin"], tc.expected("wall_negative_origin", 26), starts), "wall")
    # a later travel field discards the paths, not the other way round
    run_from(ctx, c, 6)
    assert ctx.travel_paths_into({"offsets": np.zeros(5, np.int64)}) == KHR_ESTATE
    assert ctx.travel_paths_rc(starts)[0] == 0 and ctx.travel_paths_into({"offsets": np.zeros(5, np.int64)}) == 0


def test_a_long_serpentine_takes_at_least_three_waits():
    nx, ny = tc.long_serpentine_dims(KHR_TF_TILE_EDGE, KHR_TF_ROUNDS_PER_WAIT)
    c, ctx = tc.serpentine(nx, ny), bare()
    for connectivity in tc.CONNECTIVITIES:
        want = tr.travel_field(c["origin"], c["distance"], c["status"], c["goals"], connectivity=connectivity, **c["kw"])
        got = run_from(ctx, c, connectivity)
        print(connectivity, got["stats"])
        assert got["stats"]["n_waits"] >= 3 and got["stats"]["n_rounds"] > 2 * KHR_TF_ROUNDS_PER_WAIT, got["stats"]
        assert_same(got, want, ("long serpentine", connectivity))
        blocked = ~tc.serpentine_mask(nx, ny)
        assert (got["cost"][blocked] == KHR_TF_UNREACHED).all() and (got["goal"][blocked] == -1).all() and (got["parent"][blocked] == 255).all()
        assert got["stats"]["n_reached"] == int((~blocked).sum())


def test_unknown_cells_nan_and_the_obstacle_class():
    distance = np.array([[[1.0, 1.0, np.nan, 1.0, 1.0, 0.4, 1.0, 0.5]]], np.float32)
    status = np.array([[[1, 0, 1, 1, 3, 1, 5, 4]]], np.uint8)
    c = dict(origin=(3, -2, 7), dims=(8, 1, 1), distance=distance, status=status, goals=np.array([[3, -2, 7], [9, -2, 7], [10, -2, 7]], np.int32), kw=dict(clearance=0.5))
    ctx = bare()
    for allow in (False, True):
        want = tr.travel_field(c["origin"], distance, status, c["goals"], 0.5, 6, allow_unknown=allow)
        got = run_from(ctx, c, 6, allow_unknown=allow)
        assert_same(got, want, ("classes", allow))
    assert got["cost"][0, 0].tolist() == [0, 10] + [KHR_TF_UNREACHED] * 4 + [0, 0] and got["goal"][0, 0].tolist() == [0, 0, -1, -1, -1, -1, 1, 2]
    # no usable goal is not an error: everything unreached
    rc, stats = ctx.travel_field_from_rc(ctx.travel_request(0.5, 6), c["origin"], c["dims"], c, np.array([[5, -2, 7], [100, 0, 0]], np.int32))
    assert rc == 0 and stats["n_goals_used"] == 0 and stats["n_reached"] == 0 and stats["max_cost"] == 0 and stats["n_rounds"] == 0, stats
    got = ctx._travel_result(stats)
    assert (got["cost"] == KHR_TF_UNREACHED).all() and (got["goal"] == -1).all() and (got["parent"] == 255).all()
    p = ctx.travel_paths(c["goals"])
    assert p["offsets"].tolist() == [0, 0, 0, 0] and (p["path_goal"] == -1).all()


def test_into_twice_with_guards_in_host_and_device_form():
    c, ctx = tc.built("random"), bare()
    host = run_from(ctx, c, 18)
    n = host["cost"].size
    for fields in [NAMES, NAMES] + [[k] for k in NAMES]:
        out = {k: np.full(n + GUARD, 7, dt) for k, dt in FusionContext.TF_FIELDS if k in fields}
        assert ctx.travel_field_into(out) == 0
        for k in fields:
            assert out[k][:n].tobytes() == host[k].tobytes() and (out[k][n:] == 7).all(), (fields, k)
    assert ctx.travel_field_into({}) == 0
    dev = {k: DeviceArray(np.full(n + GUARD, 9, dt)) for k, dt in FusionContext.TF_FIELDS}
    assert ctx.travel_field_into({k: d.data_ptr() for k, d in dev.items()}, on_device=True) == 0
    ctx.sync()
    for k, dt in FusionContext.TF_FIELDS:
        nbytes = n * np.dtype(dt).itemsize
        assert dev[k].read(0, nbytes).tobytes() == host[k].tobytes() and (dev[k].read(nbytes, GUARD * np.dtype(dt).itemsize).view(dt) == 9).all(), k
        dev[k].free()


def test_after_a_voronoi_field_with_given_goals_and_with_the_place_centres():
    """a hand-built map of tests/voronoi_cases.py: khr_voronoi_field, khr_places_graph, then khr_travel_field against the replica fed
    with the downloaded distance and status; the Voronoi result, the places graph and the map are only read"""
    indices, layers, origin, dims, _ = pc.voronoi_case("posts")
    cfg = default_config(voxels_per_side=vc.VPS, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
    ctx = FusionContext(cfg)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    cell = float(f32(mc.VOXEL_SIZE))
    field = ctx.voronoi_field(origin, dims, 1, 100.0, min_distance=vc.MIN_DISTANCE_CELLS * cell, **pc.VORONOI_KW)
    places = ctx.places_graph(compression=3)
    assert places["stats"]["n_places"] >= 2
    digest, stats = ctx.map_digest(), ctx.stats()
    o = np.asarray(origin)
    free = np.argwhere((field["status"] & 3) == 1)
    goals = np.concatenate([free[[0, len(free) // 2, -1]][:, ::-1] + o, o[None] - 1]).astype(np.int32)
    some = 0
    for connectivity in tc.CONNECTIVITIES:
        for clearance, allow in ((0.0, False), (1.5 * cell, False), (2.5 * cell, True)):
            kw = dict(clearance=clearance, connectivity=connectivity, allow_unknown=allow)
            got = ctx.travel_field(goals, **kw)
            want = tr.travel_field(origin, field["distance"], field["status"], goals, **kw)
            print(kw, got["stats"])
            assert_same(got, want, kw)
            assert (got["origin"], got["dims"]) == (tuple(origin), tuple(dims))
            some += got["stats"]["n_reached"] > 1
        kw = dict(clearance=1.5 * cell, connectivity=connectivity)
        got = ctx.travel_field("places", **kw)
        want = tr.travel_field(origin, field["distance"], field["status"], places["centre"], **kw)
        assert_same(got, want, ("places", kw))
        assert got["stats"]["n_goals_used"] >= 1 and got["goal"].max() < places["stats"]["n_places"]
        starts = some_starts(dict(origin=origin, dims=dims, goals=places["centre"]), want)
        assert_same_paths(ctx.travel_paths(starts), tr.travel_paths(origin, want, starts), ("places", kw))
    assert some >= 6
    # the Voronoi result, the places graph, the map and its counters are what they were
    out = {k: np.zeros_like(field[k]) for k in VOR_NAMES}
    assert ctx.voronoi_field_into(out) == 0 and all(out[k].tobytes() == field[k].tobytes() for k in VOR_NAMES)
    out = {k: np.zeros_like(places[k]) for k in PL_NAMES}
    assert ctx.places_graph_into(out) == 0 and all(out[k].tobytes() == places[k].tobytes() for k in PL_NAMES)
    assert np.array_equal(ctx.map_digest(), digest) and ctx.stats() == stats
    ctx.close()


def test_error_codes_keep_the_earlier_result():
    """every KHR_EINVAL / KHR_ESTATE case: nothing is done, the earlier result stays what it was.  (Argument checks only: the failures
    that discard a result, KHR_ENOMEM and device errors, cannot be had on purpose.)"""
    c = tc.built("wall_negative_origin")
    origin, dims, goals = c["origin"], c["dims"], c["goals"]
    cfg = default_config(voxels_per_side=16, max_blocks=64, max_frame_pixels=64 * 48, **mc.CONFIG)
    ctx = FusionContext(cfg)
    n = int(np.prod(dims))
    out = {k: np.full(n + GUARD, 7, dt) for k, dt in FusionContext.TF_FIELDS}
    assert ctx.travel_field_into(out) == KHR_ESTATE and all((a == 7).all() for a in out.values())
    assert ctx.lib.khr_travel_field_box(ctx.h, None, None) == KHR_ESTATE
    assert ctx.travel_paths_rc(goals)[0] == KHR_ESTATE and ctx.travel_paths_into({}) == KHR_ESTATE
    good = ctx.travel_request(0.5, 26)
    # no Voronoi result: a state error, and still no result
    rc, stats = ctx.travel_field_rc(good, goals)
    assert rc == KHR_ESTATE and not any(stats.values())
    assert ctx.travel_field_into(out) == KHR_ESTATE
    host = run_from(ctx, c, 26)
    starts = np.array([np.asarray(origin) + tc.WALL_PATH_START], np.int32)
    paths = ctx.travel_paths(starts)

    def intact(what):
        got = {k: np.full(n + GUARD, 7, dt) for k, dt in FusionContext.TF_FIELDS}
        assert ctx.travel_field_into(got) == 0, what
        for k, a in got.items():
            assert a[:n].tobytes() == host[k].tobytes() and (a[n:] == 7).all(), (what, k)
        p = {k: np.zeros_like(paths[k]) for k in PATH_TYPES}
        assert ctx.travel_paths_into(p) == 0 and all(p[k].tobytes() == paths[k].tobytes() for k in PATH_TYPES), what

    nan, inf = float("nan"), float("inf")
    bad_requests = {"connectivity 0": dict(connectivity=0), "connectivity 8": dict(connectivity=8), "connectivity 27": dict(connectivity=27),
                    "connectivity -6": dict(connectivity=-6), "negative clearance": dict(clearance=-0.1), "nan clearance": dict(clearance=nan),
                    "inf clearance": dict(clearance=inf)}
    for what, more in bad_requests.items():
        rq = ctx.travel_request(**dict(dict(clearance=0.5, connectivity=26), **more))
        rc, stats = ctx.travel_field_from_rc(rq, origin, dims, c, goals)
        assert rc == KHR_EINVAL and not any(stats.values()), (what, rc)
        rc, stats = ctx.travel_field_rc(rq, goals)   # (the request is looked at before the state)
        assert rc == KHR_EINVAL and not any(stats.values()), (what, rc)
        intact(what)
    many = np.zeros(((1 << 20) + 1, 3), np.int32)
    for what, g, ng in (("no goals", None, 1), ("zero goals", goals, 0), ("more than 2^20 goals", many, None)):
        assert ctx.travel_field_from_rc(good, origin, dims, c, g, n_goals=ng)[0] == KHR_EINVAL, what
        assert ctx.travel_field_rc(good, g, n_goals=ng)[0] == KHR_EINVAL, what
        intact(what)
    big = 1 << 30
    bad_boxes = {"zero dim": (origin, (24, 0, 1)), "negative dim": (origin, (-1, 17, 1)), "dim 513": (origin, (513, 1, 1)), "more than 2^24 cells": (origin, (512, 512, 65)),
                 "box above the index range": ((big - 3, 0, 0), dims), "box below the index range": ((0, -big, 0), dims), "no origin": (None, dims),
                 "no dims": (origin, None)}
    for what, (o, d) in bad_boxes.items():
        rc, stats = ctx.travel_field_from_rc(good, o, d, c, goals)
        assert rc == KHR_EINVAL and not any(stats.values()), (what, rc)
        intact(what)
    for k, _ in FusionContext.TF_INPUTS:
        assert ctx.travel_field_from_rc(good, origin, dims, dict(c, **{k: None}), goals)[0] == KHR_EINVAL, k
        intact(k)
    assert ctx.travel_field_from_rc(None, origin, dims, c, goals)[0] == KHR_EINVAL and ctx.travel_field_rc(None, goals)[0] == KHR_EINVAL
    assert ctx.travel_field_rc(good, goals)[0] == KHR_ESTATE   # still no Voronoi result
    intact("no voronoi result")
    for what, s, ns in (("no starts", None, 1), ("zero starts", starts, 0), ("more than 2^20 starts", many, None)):
        assert ctx.travel_paths_rc(s, n_starts=ns)[0] == KHR_EINVAL, what
        intact(what)
    # the edges of the valid ranges are fine
    for more in (dict(clearance=0.0), dict(connectivity=6), dict(connectivity=18), dict(max_cost=1), dict(max_cost=0xFFFFFFFF)):
        rc, _ = ctx.travel_field_from_rc(ctx.travel_request(**dict(dict(clearance=0.5, connectivity=26), **more)), origin, dims, c, goals)
        assert rc == 0, more
    shard = FusionContext(default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=64 * 48, rank=0, world_size=2))
    rc, stats = shard.travel_field_from_rc(good, origin, dims, c, goals)
    assert rc == KHR_ESTATE and not any(stats.values())
    assert shard.travel_field_rc(good, goals)[0] == KHR_ESTATE and shard.travel_field_into(out) == KHR_ESTATE and all((a == 7).all() for a in out.values())
    shard.close()
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
    travel:
      clearance_m: 0.3
      connectivity: 26
      allow_unknown: false
    tsdf_interpolator:
      type: downsample
      ratio: 2
"""


def test_aw_demo_travel_mode_agrees_with_dijkstra_on_the_host(tmp_path):
    """aw_demo --travel: a Khronos sink asks for the travel field from the camera's cell through VolumetricMap::travelField and holds it
    against Dijkstra over the downloaded field, which it replaces; the path from the furthest reached cell ends at the camera"""
    W, H, N = 320, 240, 8
    cfgp = tmp_path / "aw_travel.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--travel", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(res)
    assert res["frames"] == N and res["agree_frames"] == N and res["path_frames"] == N and res["first_mismatch"] == ""
    assert res["last_stats"]["n_reached"] > 100 and res["last_path"]["cells"] > 2
