"""khr_weld_mesh (ASSUMPTIONS.md A.16) on the device against tests/weld_replica.py, the numpy restatement of its definition, fed with
the same context's download_mesh(): every output array and every statistic byte for byte.  The maps are the hand-built ones of
tests/mesh_cases.py and reach the device as in tests/test_gpu_mesh_cases.py (checkpoint stream -> load_map -> generate_mesh), plus a
smooth sphere and a short stream whose output stage archives blocks.  tests/test_cpu_weld_replica.py checks the replica itself."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as mc
import weld_replica as wr
from common import DeviceArray
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ENOMEM, KHR_ESTATE, KHR_OK, KhrWeldStats, live_resources
from khronos_amd.synth import SyntheticStream

pytestmark = pytest.mark.gpu
VS = mc.VOXEL_SIZE
RESOLUTIONS = {"voxel": VS, "half": VS / 2, "two": 2 * VS, "5mm": 0.005}
OUTPUTS = wr.FIELDS + ("faces", "soup_to_vertex")
MAPS = {"all_cases8": lambda: (8,) + mc.all_cases(8), "all_cases16": lambda: (16,) + mc.all_cases(16), "edges": lambda: (16,) + mc.edges(16),
        "relations": lambda: (16,) + mc.relations(), "dense8": lambda: (8,) + mc.dense(8), "shortcut": lambda: (16,) + mc.shortcut(),
        "sphere8": lambda: (8,) + wr.sphere(8), "sphere16": lambda: (16,) + wr.sphere(16)}


def make_cfg(vps, **kw):
    return default_config(voxels_per_side=vps, max_blocks=4096, max_frame_pixels=320 * 240, exact_arithmetic=1, **dict(mc.CONFIG, **kw))


def load(vps, indices, layers, **kw):
    cfg = make_cfg(vps, **kw)
    ctx = FusionContext(cfg)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    return ctx


def assert_same(got, want, what):
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))
            raise AssertionError((what, k, len(bad), "of", len(got[k]), "first", bad[:4], got[k][bad[:4]], want[k][bad[:4]]))


def assert_weld(ctx, r, what, soup=None):
    """the device's weld of the current mesh == the replica's weld of the downloaded soup"""
    soup = ctx.download_mesh() if soup is None else soup
    got, want = ctx.weld_mesh(r), wr.weld(soup, r)
    assert_same(got, want, what)
    return got


def last_error(ctx):
    return ctx.lib.khr_last_error().decode()


@pytest.fixture(scope="module", params=list(MAPS))
def meshed(request):
    """one context per map with its mesh, and the soup as download_mesh hands it out (read-only, shared by the resolutions)"""
    vps, idx, layers = MAPS[request.param]()
    ctx = load(vps, idx, layers)
    ctx.generate_mesh(False, False)
    soup = ctx.download_mesh()
    assert len(soup["points"]) > 6
    for a in soup.values():
        a.setflags(write=False)
    yield request.param, ctx, soup
    ctx.close()


@pytest.mark.parametrize("res", list(RESOLUTIONS))
def test_maps(meshed, res):
    name, ctx, soup = meshed
    got = assert_weld(ctx, RESOLUTIONS[res], (name, res), soup)
    st = got["stats"]
    print(name, res, st)
    assert st["n_soup_vertices"] == len(soup["points"]) and st["n_faces"] + st["n_degenerate_faces"] == len(soup["points"]) // 3
    if res == "two":   # most faces collapse
        assert st["n_degenerate_faces"] > st["n_faces"]
    if res == "5mm" and name != "shortcut":   # welds almost nothing: only vertices the cubes round an edge computed alike
        assert st["n_degenerate_faces"] <= st["n_faces"] // 20
    if name.startswith("sphere") and res == "voxel":
        assert st["n_vertices"] <= st["n_soup_vertices"] / 5 and st["n_faces"] >= 0.4 * (st["n_soup_vertices"] // 3)


def test_device_outputs_equal_the_host_form(meshed):
    """khr_weld_mesh_into(on_device = 1) into device arrays: stream order, nothing awaited; after khr_sync the host form's bytes, and
    not a byte behind them.  (Device memory through tests/common.DeviceArray, like the other device-form tests: the test process
    holds one HIP runtime, the library's.)"""
    name, ctx, soup = meshed
    host = ctx.weld_mesh(VS)
    guard = 16
    dev = {k: DeviceArray(np.full((len(host[k]) + guard,) + host[k].shape[1:], 9, host[k].dtype)) for k in OUTPUTS}
    assert ctx.weld_mesh_into({k: d.data_ptr() for k, d in dev.items()}, on_device=True) == KHR_OK
    ctx.sync()
    for k in OUTPUTS:
        n, row = host[k].nbytes, int(np.prod(host[k].shape[1:], dtype=np.int64)) * host[k].dtype.itemsize
        assert dev[k].read(0, n).tobytes() == host[k].tobytes(), (name, k)
        assert (dev[k].read(n, guard * row).view(host[k].dtype) == 9).all(), (name, k)
        dev[k].free()
    # a second copy of the same weld, a subset of the arrays: one device array, two host arrays
    only = DeviceArray(np.full(host["faces"].size + guard, 9, np.uint32))
    assert ctx.weld_mesh_into({"faces": only.data_ptr()}, on_device=True) == KHR_OK
    ctx.sync()
    assert only.read(0, host["faces"].nbytes).tobytes() == host["faces"].tobytes() and (only.read(host["faces"].nbytes, 4 * guard).view(np.uint32) == 9).all()
    only.free()
    again = {"faces": np.zeros_like(host["faces"]), "points": np.zeros_like(host["points"])}
    assert ctx.weld_mesh_into(again) == KHR_OK
    assert again["faces"].tobytes() == host["faces"].tobytes() and again["points"].tobytes() == host["points"].tobytes()


def test_empty_mesh():
    """a map without a sign change: KHR_OK, zeros, and _into has nothing to copy"""
    vps = 8
    g = mc.Group(np.random.default_rng(5), vps, (3, 4, 5), signs=1.0)
    ctx = load(vps, *mc.to_map([g]))
    ctx.generate_mesh(False, False)
    st = KhrWeldStats(1, 1, 1, 1)
    assert ctx.lib.khr_weld_mesh(ctx.h, VS, C.byref(st)) == KHR_OK
    assert (st.n_soup_vertices, st.n_vertices, st.n_faces, st.n_degenerate_faces) == (0, 0, 0, 0)
    w = ctx.weld_mesh(VS)
    assert w["stats"] == wr.weld(ctx.download_mesh(), VS)["stats"] and all(len(w[k]) == 0 for k in OUTPUTS)
    assert w["faces"].shape == (0, 3)
    assert ctx.lib.khr_weld_mesh(ctx.h, VS, None) == KHR_OK   # (stats may be NULL)
    ctx.close()


def test_partial_meshings():
    """the device buffer's order differs from the soup's: the flagged half alone, all blocks, the half again with carried-over blocks"""
    idx, layers, flagged = mc.partial(with_plan=True)
    ctx = load(16, idx, layers)
    sizes = []
    for step, (only, clear) in enumerate([(True, False), (False, False), (True, True), (True, True)]):
        ctx.generate_mesh(only, clear)
        for res in ("voxel", "half"):
            sizes.append(assert_weld(ctx, RESOLUTIONS[res], ("partial", step, res))["stats"]["n_soup_vertices"])
    assert 0 < sizes[0] < sizes[2] == sizes[4] == sizes[6]
    ctx.close()


def test_stream_with_archived_blocks():
    """a short 320 x 240, 10 cm stream with tracking whose output stage archives blocks: the vertex buffer then still holds the
    ranges of blocks that are no longer live, and the weld skips them as download_mesh does"""
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, with_semantics=1, with_tracking=1, max_blocks=4096,
                         max_frame_pixels=320 * 240, exact_arithmetic=1, temporal_window=0.55)
    ctx = FusionContext(cfg)
    s = SyntheticStream(320, 240, seed=1234)
    sen = ctx.make_sensor(320, 240, s.fx, s.fy, s.cx, s.cy)
    archived, kept = 0, None
    for i in range(12):
        fr = s.render(i)
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        ctx.integrate(slot, allocate_blocks=True, use_mask=False)
        ctx.update_tracking(fr["stamp"])
        if i % 4 == 3:
            ctx.generate_mesh(True, True)
            if kept is not None:   # four more frames fused and meshed: the result of the last weld is still that weld's
                out = {k: np.zeros_like(kept[k]) for k in OUTPUTS}
                assert ctx.weld_mesh_into(out) == KHR_OK
                assert all(out[k].tobytes() == kept[k].tobytes() for k in OUTPUTS)
                assert len(ctx.download_mesh()["points"]) != kept["stats"]["n_soup_vertices"]
            before = assert_weld(ctx, VS, ("stream", i, "meshed"))
            n_arch = len(ctx.reset_inactive())
            ctx.clear_updated()
            after = assert_weld(ctx, VS, ("stream", i, "archived"))
            kept = after
            if n_arch and after["stats"]["n_soup_vertices"] < before["stats"]["n_soup_vertices"]:
                archived += 1
                assert after["stats"]["n_soup_vertices"] < ctx.lib.khr_mesh_num_vertices(ctx.h)   # (the buffer keeps the archived ranges)
                kept = assert_weld(ctx, VS / 2, ("stream", i, "archived, half a voxel"))
    assert archived > 0
    ctx.close()


def test_life_cycle():
    """two welds on one context; the result is a copy: it survives a meshing of other content, until the next weld"""
    idx, layers, flagged = mc.partial(with_plan=True)
    ctx = load(16, idx, layers)
    ctx.generate_mesh(True, False)          # the flagged half
    soup = ctx.download_mesh()
    first = assert_weld(ctx, VS, "first", soup)
    second = assert_weld(ctx, VS / 2, "second resolution", soup)
    assert second["stats"]["n_vertices"] > first["stats"]["n_vertices"]
    kept = assert_weld(ctx, VS, "first resolution again", soup)
    ctx.generate_mesh(False, False)         # every block: another mesh, and the vertex buffers have flipped
    assert len(ctx.download_mesh()["points"]) > len(soup["points"])
    for _ in range(2):                      # (_into may be called several times)
        out = {k: np.zeros_like(kept[k]) for k in OUTPUTS}
        assert ctx.weld_mesh_into(out) == KHR_OK
        for k in OUTPUTS:
            assert out[k].tobytes() == kept[k].tobytes(), k
    third = assert_weld(ctx, VS, "after the second meshing")
    assert third["stats"]["n_soup_vertices"] > kept["stats"]["n_soup_vertices"]
    # khr_reset_map ends the result's life
    ctx.reset_map(VS, mc.TRUNCATION)
    assert ctx.weld_mesh_into({}) == KHR_ESTATE
    ctx.close()


@pytest.mark.parametrize("r", [0.0, -0.1, float("nan"), float("inf"), -float("inf")])
def test_bad_resolution(r):
    ctx = FusionContext(make_cfg(8))
    assert ctx.lib.khr_weld_mesh(ctx.h, r, None) == KHR_EINVAL
    assert "resolution" in last_error(ctx)
    ctx.close()


@pytest.mark.parametrize("vps", [8, 16])
def test_resolution_too_fine_for_the_extent(vps):
    """all_cases lies at block x = -2001: at 1 mm its cell index is about -1.6 M (vps 8) / -3.2 M (vps 16), the limit is 2^20"""
    ctx = load(vps, *mc.all_cases(vps))
    ctx.generate_mesh(False, False)
    good = ctx.weld_mesh(VS)
    assert good["stats"]["n_vertices"] > 0
    with pytest.raises(wr.OutOfRange):
        wr.weld(ctx.download_mesh(), 0.001)
    st = KhrWeldStats(1, 1, 1, 1)
    assert ctx.lib.khr_weld_mesh(ctx.h, 0.001, C.byref(st)) == KHR_EINVAL
    msg = last_error(ctx)
    assert "0.001" in msg and "too fine for the extent of the map" in msg, msg
    assert (st.n_soup_vertices, st.n_vertices, st.n_faces, st.n_degenerate_faces) == (0, 0, 0, 0)
    assert ctx.weld_mesh_into({}) == KHR_ESTATE      # the failed weld has discarded the earlier result
    assert "khr_weld_mesh" in last_error(ctx)
    assert_weld(ctx, VS, "after the failure")
    ctx.close()


def test_overflow_state():
    """max_mesh_vertices one below the need: KHR_ENOMEM with both numbers, as the other mesh queries; after meshing what fits, a weld"""
    vps = 8
    need = mc.dense_vertices(vps)
    idx, layers = mc.dense(vps, flagged=mc.DENSE_HALF)
    ctx = load(vps, idx, layers, max_mesh_vertices=need - 1)
    ctx.generate_mesh(False, False)
    for _ in range(2):
        assert ctx.lib.khr_weld_mesh(ctx.h, VS, None) == KHR_ENOMEM
        msg = last_error(ctx)
        assert str(need) in msg and str(need - 1) in msg, msg
    assert ctx.lib.khr_mesh_num_vertices(ctx.h) == KHR_ENOMEM
    assert last_error(ctx) == msg                    # the same text as the other mesh queries give
    assert ctx.weld_mesh_into({}) == KHR_ESTATE
    ctx.generate_mesh(True, True)                    # the flagged half fits
    got = assert_weld(ctx, VS, "flagged half after an overflow")
    assert got["stats"]["n_soup_vertices"] == mc.dense_vertices(vps, mc.DENSE_HALF)
    ctx.close()


def test_sharded_context_is_refused():
    ctx = FusionContext(make_cfg(8, rank=0, world_size=2))
    assert ctx.lib.khr_weld_mesh(ctx.h, VS, None) == KHR_ESTATE
    assert "world_size is 2" in last_error(ctx)
    ctx.close()


def test_into_before_any_weld():
    ctx = load(8, *mc.all_cases(8))
    ctx.generate_mesh(False, False)
    assert ctx.weld_mesh_into({}) == KHR_ESTATE
    assert "khr_weld_mesh" in last_error(ctx)
    ctx.close()


def test_no_resource_outlives_the_context():
    before = live_resources()
    ctx = load(8, *mc.all_cases(8))
    ctx.generate_mesh(False, False)
    assert_weld(ctx, VS, "small")
    assert_weld(ctx, 0.005, "small, fine")
    assert live_resources() != before
    ctx.close()
    assert live_resources() == before


def test_aw_demo_weld_mode_equals_its_host_weld_and_the_python_path(tmp_path):
    """aw_demo --weld: the window's mesh through hydra::VolumetricMap::weldedMesh equals the fetched soup welded on one host thread
    with a first-come unordered_map, array for array; the same stream stepped through the C ABI as ActiveWindow::spinOnce steps it
    (tests/test_gpu_align_frame.py) gives the same counts from FusionContext.weld_mesh"""
    from common import make_pair
    from test_gpu_render_view import YAML
    W, H, N = 320, 240, 14
    cfgp = tmp_path / "aw_weld.yaml"
    cfgp.write_text(YAML)
    demo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khronos_amd", "lib", "aw_demo")
    out = subprocess.run([demo, "--weld", str(cfgp), str(W), str(H), str(N), "0.1", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N and res["equal"] is True and res["first_mismatch"] == ""
    assert res["n_soup_vertices"] > 3000 and res["n_faces"] + res["n_degenerate_faces"] == res["n_soup_vertices"] // 3
    assert res["soup_bytes"] == 36 * res["n_soup_vertices"] and res["indexed_bytes"] == 36 * res["n_vertices"] + 12 * res["n_faces"]
    assert res["indexed_bytes"] < res["soup_bytes"] // 2
    cfg, ctx, ora, s, sen, osen = make_pair(width=W, height=H, temporal_window=0.75, truncation_distance=0.3, exact_arithmetic=1,
                                            md_min_cluster_size=20, md_min_separation_distance=2.0, md_max_range=5.0)
    ora.close()
    last_full = 0
    for i in range(N):
        fr = s.render(i)
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        ctx.detect_motion(slot)
        ctx.integrate(slot, allocate_blocks=True, use_mask=True)
        ctx.update_tracking(fr["stamp"])
        if not (last_full + int(float(np.float32(0.4)) * 1e9) > fr["stamp"]):
            ctx.generate_mesh(True, True)
            ctx.reset_inactive()
            ctx.clear_updated()
            last_full = fr["stamp"]
    mine = assert_weld(ctx, np.float32(0.1), "the demo's stream")["stats"]
    ctx.close()
    assert mine == {k: res[k] for k in mine}
