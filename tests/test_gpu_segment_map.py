"""khr_segment_map (FusionContext.segment_map; ASSUMPTIONS.md A.19): the connected components of the live map's occupied voxels,
found on the device.  The hand-built maps of tests/segment_cases.py, a fused map with deferred stamps, the two forms of
khr_segment_map_into and the life of the result, errors (each leaves the map's digest as it was) and resources -- every array and
statistic byte for byte against the plain restatement (tests/segment_replica.py: a breadth-first flood fill)."""
import ctypes as C
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import diff_cases as dc
import segment_cases as sc
import segment_replica as sr
from khronos_amd import FusionContext, checkpoint as ck
from khronos_amd.capi import KHR_EINVAL, KHR_ESTATE, KHR_OK, live_resources
from test_gpu_merge_map import digests_equal, last_error, load, make_cfg

pytestmark = pytest.mark.gpu
COMPONENT, VOXEL = sr.COMPONENT_FIELDS, sr.VOXEL_FIELDS
ZERO_STATS = dict.fromkeys(sr.STATS, 0)


def assert_result(got, want, what, want_voxels=True):
    print(what, got["stats"])
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    for name, dt, sh in COMPONENT + (VOXEL if want_voxels else ()):
        g, w = got[name], want[name]
        assert g.dtype == dt and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first rows", bad[:4].tolist(), g[bad[:4]].tolist(), w[bad[:4]].tolist()))
    if not want_voxels:
        assert "voxels" not in got and "voxel_component" not in got
    assert got["centroid"].dtype == np.float64 and got["centroid"].tobytes() == want["centroid"].tobytes(), what


def replica_from_stream(ctx, **kw):
    """the replica on what the context saves"""
    h, idx, layers = ck.unpack(ctx.save_map())
    return sr.segment({k: h[k] for k in ck.CONFIG_FIELDS}, idx, layers, mesh_min_weight=float(ctx.cfg.mesh_min_weight), **kw)


@pytest.mark.parametrize("name", [c["name"] for c in sc.CASES])
def test_cases(name):
    c = sc.BY_NAME[name]
    ctx = load(c["cfg"], *c["now"])
    assert float(ctx.cfg.mesh_min_weight) == float(np.float32(sc.MESH_MIN_WEIGHT))
    before = ctx.map_digest()
    for i, run in enumerate(c["runs"]):
        for want_voxels in (True, False):
            got = ctx.segment_map(want_voxels=want_voxels, **sc.request_of(run))
            assert_result(got, sc.replica_of(c, i, want_voxels), (name, sc.request_of(run), want_voxels), want_voxels)
        if run["expect"] is not None:  # (the count written into the case by hand)
            assert got["stats"]["n_components"] == run["expect"], (name, run)
    assert digests_equal(ctx.map_digest(), before), name
    if name == "order":
        got = ctx.segment_map(connectivity=6)
        assert [sc.block_of(v, 16) for v in got["representative"].tolist()] == c["blocks"] and got["voxel_component"].tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    if name == "big":
        got = ctx.segment_map(connectivity=26, by_label=False)
        assert got["n_voxels"].tolist() == [8 * 16 ** 3] * 2 and (np.abs(got["sum"]) > 2 ** 32).all() and got["first"].tolist() == [0, 8 * 16 ** 3]
    if name.startswith("checker"):
        vps = c["cfg"]["voxels_per_side"]
        got = ctx.segment_map(connectivity=6, by_label=True)
        assert got["stats"]["n_components"] == vps ** 3 and (got["n_voxels"] == 1).all()
    ctx.close()


@pytest.fixture(scope="module")
def fused():
    """a map fused from 3 frames at 320 x 240 / 10 cm with semantics and tracking (deferred stamps), and its mesh"""
    from common import make_pair
    cfg, ctx, ora, s, sen, osen = make_pair(width=320, height=240, max_blocks=2048)
    ora.close()
    for i in range(3):
        fr = s.render(i)
        ctx.integrate(ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"]))
        ctx.update_tracking(fr["stamp"])
    ctx.generate_mesh(only_mesh_updated=False)
    yield dict(cfg=cfg, ctx=ctx, stream=s, sensor=sen)
    ctx.close()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_fused_map(fused, connectivity):
    ctx = fused["ctx"]
    before = ctx.map_digest()
    got = ctx.segment_map(connectivity=connectivity)
    assert digests_equal(ctx.map_digest(), before)
    assert_result(got, replica_from_stream(ctx, connectivity=connectivity), ("fused", connectivity))
    st = got["stats"]
    assert st["n_blocks"] == ctx.num_blocks() and st["n_components"] > 1 and st["n_voxels"] == st["n_member_voxels"] > 1000
    assert (got["last_observed_max"] > 0).all()
    # sized by the live blocks now (num_blocks has brought the host index up to date): the same result
    again = ctx.segment_map(connectivity=connectivity)
    assert all(again[k].tobytes() == got[k].tobytes() for k, _, _ in COMPONENT + VOXEL) and again["stats"] == st


def test_into_forms_and_the_life_of_the_result(fused):
    ctx = fused["ctx"]
    ref = ctx.segment_map(min_voxels=2)
    m, n = len(ref["label"]), len(ref["voxel_component"])
    assert m > 0 and n > 0

    def host_copy(names=None):
        out = {k: np.zeros((m if w == "c" else n,) + sh, dt) for k, dt, sh, w in ctx.SEGMENT_FIELDS}
        for a in out.values():
            a.view(np.uint8)[...] = 0xAB
        assert ctx.segment_map_into({k: v for k, v in out.items() if names is None or k in names}) == KHR_OK
        return out

    full = host_copy()
    for k, _, _ in COMPONENT + VOXEL:
        assert full[k].tobytes() == ref[k].tobytes(), k
    part = host_copy(names=("sum", "voxel_component"))  # NULL pointers are skipped; the call can be repeated
    for k, _, _ in COMPONENT + VOXEL:
        if k in ("sum", "voxel_component"):
            assert part[k].tobytes() == ref[k].tobytes(), k
        else:
            assert (part[k].view(np.uint8) == 0xAB).all(), k
    # the device form: device-to-device in stream order (device arrays through the runtime the library is linked against)
    from common import DeviceArray
    dev = {k: DeviceArray(np.zeros((m if w == "c" else n,) + sh, dt)) for k, dt, sh, w in ctx.SEGMENT_FIELDS}
    assert ctx.segment_map_into({k: d.data_ptr() for k, d in dev.items()}, on_device=True) == KHR_OK
    ctx.sync()
    for k, _, _ in COMPONENT + VOXEL:
        assert dev[k].read(0, ref[k].nbytes).tobytes() == ref[k].tobytes(), k
    for d in dev.values():
        d.free()
    # the result survives a frame, a meshing, a weld and a diff; the mesh, the weld and the diff survive a segmentation
    fr = fused["stream"].render(3)
    ctx.integrate(ctx.upload_frame(fused["sensor"], fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"]))
    ctx.update_tracking(fr["stamp"])
    ctx.generate_mesh(only_mesh_updated=False)
    weld = ctx.weld_mesh(0.01)
    c = dc.BY_NAME["one_block"]
    other = load(c["cfg"], *c["then"])
    side = load(c["cfg"], *c["now"])
    diff = side.diff_map(other, **dc.request_of(c))
    later = host_copy()
    for k, _, _ in COMPONENT + VOXEL:
        assert later[k].tobytes() == ref[k].tobytes(), k
    mesh, digest, stats = ctx.fetch_mesh(), ctx.map_digest(), ctx.stats()
    now = ctx.segment_map(want_voxels=False)
    side.segment_map()
    assert now["stats"]["n_components"] > 0
    assert digests_equal(ctx.map_digest(), digest)
    after = ctx.fetch_mesh()
    assert all(after[k].tobytes() == mesh[k].tobytes() for k in mesh)
    assert ctx.stats() == stats  # (every counter of khr_stats, the cumulative ones among them)
    w2 = {k: np.zeros_like(v) for k, v in weld.items() if k != "stats"}
    assert ctx.weld_mesh_into(w2) == KHR_OK and all(w2[k].tobytes() == weld[k].tobytes() for k in w2)
    d2 = {k: np.zeros_like(v) for k, v in diff.items() if k != "stats"}
    assert side.diff_map_into(d2) == KHR_OK and all(d2[k].tobytes() == diff[k].tobytes() for k in d2)
    # the voxel arrays of a result without the list; a failed call discards the result, a new one brings it back
    assert ctx.segment_map_into({"label": np.zeros(len(now["label"]), np.int32)}) == KHR_OK
    assert ctx.segment_map_into({"voxels": np.zeros((n + 4096, 3), np.int32)}) == KHR_ESTATE and "want_voxels" in last_error(ctx)
    assert ctx.segment_map_into({"voxel_component": np.zeros(n + 4096, np.uint32)}) == KHR_ESTATE
    rc, _ = ctx.segment_map_rc(ctx.segment_request(connectivity=7))
    assert rc == KHR_EINVAL
    assert ctx.segment_map_into({}) == KHR_ESTATE and "khr_segment_map" in last_error(ctx)
    got = ctx.segment_map(connectivity=18)
    assert_result(got, replica_from_stream(ctx, connectivity=18), "after a frame")
    assert ctx.segment_map_into({}) == KHR_OK
    other.close()
    side.close()


def test_no_result_before_a_call_after_a_reset_and_after_a_load():
    c = sc.BY_NAME["filter"]
    ctx = load(c["cfg"], *c["now"])
    assert ctx.segment_map_into({}) == KHR_ESTATE
    assert ctx.segment_map(connectivity=6)["stats"]["n_components"] == 5
    assert ctx.segment_map_into({}) == KHR_OK
    ctx.reset_map(c["cfg"]["voxel_size"], c["cfg"]["truncation_distance"])
    assert ctx.segment_map_into({}) == KHR_ESTATE
    assert ctx.segment_map()["stats"] == ZERO_STATS  # (an empty map: KHR_OK with zero counts)
    assert ctx.segment_map_into({}) == KHR_OK
    assert ctx.load_map(ck.pack(ctx.cfg, *c["now"])) == len(c["now"][0])
    assert ctx.segment_map_into({}) == KHR_ESTATE
    assert ctx.segment_map(connectivity=6)["stats"]["n_components"] == 5
    ctx.close()


BAD_REQUESTS = {
    "connectivity_0": (dict(connectivity=0), "connectivity"),
    "connectivity_8": (dict(connectivity=8), "connectivity"),
    "min_weight_negative": (dict(min_weight=-1.0), "min_weight"),
    "min_weight_nan": (dict(min_weight=float("nan")), "min_weight"),
    "min_weight_inf": (dict(min_weight=float("inf")), "min_weight"),
    "surface_distance_nan": (dict(surface_distance=float("nan")), "surface_distance"),
    "surface_distance_inf": (dict(surface_distance=float("-inf")), "surface_distance"),
    "too_many_labels": (dict(labels=list(range(65))), "n_labels"),
    "max_below_min": (dict(min_voxels=5, max_voxels=4), "max_voxels"),
    "max_below_one": (dict(min_voxels=-2, max_voxels=0), None),  # (fine: min_voxels < 1 means 1, max_voxels <= 0 unlimited)
}


@pytest.fixture(scope="module")
def single():
    c = sc.BY_NAME["filter"]
    ctx = load(c["cfg"], *c["now"])
    yield ctx, ctx.map_digest()
    ctx.close()


@pytest.mark.parametrize("what", sorted(BAD_REQUESTS))
def test_bad_requests(single, what):
    ctx, digest = single
    assert ctx.segment_map(connectivity=6)["stats"]["n_components"] == 5
    kw, text = BAD_REQUESTS[what]
    rc, st = ctx.segment_map_rc(ctx.segment_request(**kw))
    if text is None:
        assert rc == KHR_OK and st["n_components"] == 5
        return
    assert rc == KHR_EINVAL and "khr_segment_map" in last_error(ctx) and text in last_error(ctx), (rc, last_error(ctx))
    assert st == ZERO_STATS and digests_equal(ctx.map_digest(), digest)
    assert ctx.segment_map_into({}) == KHR_ESTATE  # the earlier result is gone


def test_null_arguments_and_label_pointers(single):
    ctx, digest = single
    rq = ctx.segment_request()
    rc, _ = ctx.segment_map_rc(None)
    assert rc == KHR_EINVAL and "null" in last_error(ctx)
    assert ctx.lib.khr_segment_map(None, C.byref(rq), None) == KHR_EINVAL
    assert ctx.lib.khr_segment_map_into(None, 0, *([None] * 10)) == KHR_EINVAL
    assert ctx.lib.khr_segment_map(ctx.h, C.byref(rq), None) == KHR_OK  # (stats may be NULL)
    rq.n_labels = -1
    assert ctx.segment_map_rc(rq)[0] == KHR_EINVAL and "n_labels" in last_error(ctx)
    rq.n_labels, rq.labels = 3, None
    assert ctx.segment_map_rc(rq)[0] == KHR_EINVAL and "labels" in last_error(ctx)
    assert digests_equal(ctx.map_digest(), digest)


def test_a_sharded_context_is_refused():
    sharded = FusionContext(make_cfg(sc.CFG16, rank=0, world_size=2))
    rc, st = sharded.segment_map_rc(sharded.segment_request())
    assert rc == KHR_ESTATE and "world_size" in last_error(sharded) and st == ZERO_STATS
    sharded.close()


def test_resources():
    """the scratch and the result belong to the context: a repeat of the same size allocates nothing, a failed call frees nothing
    early and leaks nothing, and nothing outlives the context"""
    gc.collect()
    start = live_resources()
    c = sc.BY_NAME["rich_vps8"]
    ctx = load(c["cfg"], *c["now"])
    idle = live_resources()
    first_result = ctx.segment_map(connectivity=6)
    first = live_resources()
    assert first != idle
    again = ctx.segment_map(connectivity=6)
    assert live_resources() == first
    for k, _, _ in COMPONENT + VOXEL:
        assert again[k].tobytes() == first_result[k].tobytes(), k
    assert ctx.segment_map_rc(ctx.segment_request(connectivity=5))[0] == KHR_EINVAL
    assert live_resources() == first
    ctx.close()
    assert live_resources() == start
    failed = load(c["cfg"], *c["now"])
    assert failed.segment_map_rc(failed.segment_request(min_weight=-1.0))[0] == KHR_EINVAL
    failed.close()
    assert live_resources() == start


def test_aw_demo_segment_mode_equals_its_host_flood_fill(tmp_path):
    """aw_demo --segment: one ActiveWindow takes the stream, at the end its map is segmented through hydra::VolumetricMap::segment
    and, from block copies, by a breadth-first flood fill on one host thread: equal array for array"""
    from test_gpu_render_view import YAML
    W, H, N = 64, 48, 6
    cfgp = tmp_path / "aw_segment.yaml"
    cfgp.write_text(YAML)
    demo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khronos_amd", "lib", "aw_demo")
    out = subprocess.run([demo, "--segment", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N and res["equal"] is True and res["first_mismatch"] == ""
    assert res["n_blocks"] > 0 and res["n_components"] > 0 and res["n_voxels"] == res["n_member_voxels"] > 0
