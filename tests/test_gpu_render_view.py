"""khr_render_view / FusionContext.render_view: the live map ray-cast on the device into depth, normal, colour, label, voxel-flag and
status images (ASSUMPTIONS.md A.12), held bit for bit to tests/render_replica.py over this context's block downloads and over the
CPU oracle's blocks."""
import json
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import render_replica as rr
from common import DeviceArray, _mix64, make_pair, step_both
from khronos_amd import FusionContext, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ESTATE
from khronos_amd.synth import camera_pose, circle_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
IMAGES = ("depth", "normal", "color", "label", "flags", "status")
N_FRAMES = 30


def run_stream(n_frames=N_FRAMES, archive_every=5, **cfg_kw):
    """the stream of tests/test_gpu_map_slice.py: tracking and motion detection on, archival every few frames"""
    cfg, ctx, ora, s, sen, osen = make_pair(**cfg_kw)
    last = None
    for i in range(n_frames):
        last = s.render(i)
        last["step"] = step_both(ctx, ora, sen, osen, last, motion=bool(cfg.with_tracking), track=bool(cfg.with_tracking))
        if archive_every and i % archive_every == archive_every - 1:
            assert np.array_equal(np.asarray(ctx.reset_inactive()), np.asarray(ora.reset_inactive()))
    return SimpleNamespace(cfg=cfg, ctx=ctx, ora=ora, sen=sen, last=last, cache={})


def small_sensor(width=160, height=120, min_range=0.1, max_range=5.0):
    return FusionContext.make_sensor(width, height, width / 2.0, width / 2.0, width / 2.0, height / 2.0, min_range, max_range)


def views(last_pose, last_sensor):
    """name -> (sensor, pose, step_voxels)"""
    yaw_last = math.atan2(last_pose[1, 2], last_pose[0, 2])
    return {
        # the last frame's own pose and sensor, the default half-voxel step
        "own": (last_sensor, last_pose, 0.0),
        # a pose the stream never had: translated and yawed, whole-voxel steps
        "moved": (small_sensor(), camera_pose(last_pose[:3, 3] + np.array([0.3, -0.2, 0.1]), yaw_last + 0.4), 1.0),
        # outside the map, looking in at the room's centre from 9 m away and above the camera's circle
        "outside_in": (small_sensor(max_range=12.0), camera_pose(np.array([9.0, 0.5, 2.2]), math.pi), 0.5),
        # far from every block, looking away from the map
        "nothing": (small_sensor(64, 48), camera_pose(np.array([60.0, 60.0, 30.0]), 0.25 * math.pi), 0.5),
        # one pixel
        "one_pixel": (FusionContext.make_sensor(1, 1, 1.0, 1.0, 0.5, 0.5, 0.1, 5.0), last_pose, 0.5),
    }


def replica(st, which, sensor, pose, step):
    """the replica over this context's downloads ("ctx") or the oracle's blocks ("ora"); the block sets are built once"""
    if which not in st.cache:
        src = st.ctx if which == "ctx" else st.ora
        get = st.ctx.download_block if which == "ctx" else st.ora.get_block
        st.cache[which] = rr.BlockSet(src.block_indices(), get, st.cfg.voxels_per_side)
    return rr.render(None, None, st.cfg.voxels_per_side, st.cfg.voxel_size, sensor, pose, step_voxels=step,
                     min_weight=st.cfg.mesh_min_weight, with_semantics=bool(st.cfg.with_semantics), blocks=st.cache[which])


def assert_same_images(got, want, what):
    for k in IMAGES:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k] != want[k])
            raise AssertionError((what, k, len(bad), bad[:4].tolist()))
    assert got["stats"]["n_hit"] == want["n_hit"] and got["stats"]["n_blocked"] == want["n_blocked"], (what, got["stats"], want["n_hit"], want["n_blocked"])
    px = want["status"].size
    assert got["stats"]["n_samples_total"] == want["samples_per_ray"] * px
    assert 0 < got["stats"]["n_samples_evaluated"] <= got["stats"]["n_samples_total"]


@pytest.fixture(scope="module")
def stream():
    return run_stream(temporal_window=0.6)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["own", "moved", "outside_in", "nothing", "one_pixel"])
def test_views_match_the_replica_bit_for_bit(stream, name):
    st = stream
    sensor, pose, step = views(st.last["pose"], st.sen)[name]
    got = st.ctx.render_view(sensor, pose, step_voxels=step)
    mine = replica(st, "ctx", sensor, pose, step)
    # non-vacuity: conditions on the replica alone
    if name == "own":
        valid_in = st.last["depth"] > 0
        hits = (mine["status"] == 1) & valid_in
        print("own pose: %d of %d pixels with input depth are hits" % (hits.sum(), valid_in.sum()))
        assert 2 * hits.sum() >= valid_in.sum()
    if name == "outside_in":
        print("outside_in: hit %d blocked %d none %d" % (mine["n_hit"], mine["n_blocked"], (mine["status"] == 0).sum()))
        assert (mine["status"] == 2).any() and (mine["status"] == 0).any()
    if name == "nothing":
        assert not mine["status"].any()
    assert_same_images(got, mine, name + " / download_block")
    assert_same_images(got, replica(st, "ora", sensor, pose, step), name + " / oracle")
    if name == "outside_in":  # the skipping is live
        assert got["stats"]["n_samples_evaluated"] < got["stats"]["n_samples_total"], got["stats"]


@pytest.mark.gpu
def test_rendered_depth_lies_on_the_frames_surface(stream):
    """independent of the replica: at the last frame's own pose the zero crossing lies inside the truncation band around the
    observed surface, so the median |rendered - input| depth over hit, valid, non-dynamic pixels is below truncation_distance"""
    st = stream
    got = st.ctx.render_view(st.sen, st.last["pose"])
    dyn = np.asarray(st.last["step"]["dyn_gpu"]).reshape(st.last["depth"].shape) != 0
    sel = (got["status"] == 1) & (st.last["depth"] > 0) & ~dyn
    assert sel.sum() > 1000
    med = float(np.median(np.abs(got["depth"][sel] - st.last["depth"][sel])))
    print("median |rendered - input| depth = %.4f m over %d pixels (truncation %.2f m)" % (med, sel.sum(), st.cfg.truncation_distance))
    assert med < st.cfg.truncation_distance


@pytest.mark.gpu
def test_the_call_only_reads_and_repeats_identically(stream):
    st = stream
    sensor, pose, step = views(st.last["pose"], st.sen)["moved"]
    digest, idx, stats = st.ctx.map_digest(), st.ctx.block_indices().copy(), st.ctx.stats()
    a = st.ctx.render_view(sensor, pose, step_voxels=step)
    b = st.ctx.render_view(sensor, pose, step_voxels=step)
    for k in IMAGES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"] == b["stats"] and a["stats"]["n_hit"] > 0
    assert np.array_equal(st.ctx.map_digest(), digest)
    assert np.array_equal(st.ctx.block_indices(), idx)
    assert st.ctx.stats() == stats


@pytest.mark.gpu
def test_device_form_null_outputs_and_min_weight(stream):
    st = stream
    sensor, pose, step = views(st.last["pose"], st.sen)["moved"]
    host = st.ctx.render_view(sensor, pose, step_voxels=step)
    rq = st.ctx.render_request(sensor, pose, step)
    # on_device: the same bytes in device buffers
    dev = {n: DeviceArray(np.full(host[n].shape, 7, dt)) for n, dt, _ in st.ctx.RENDER_FIELDS}
    rc, stats = st.ctx.render_view_into(rq, {n: d.data_ptr() for n, d in dev.items()}, on_device=True)
    assert rc == 0 and stats == host["stats"]
    for n in IMAGES:
        assert dev[n].read(0, host[n].nbytes).tobytes() == host[n].tobytes(), n
    # on_device without counters: stream order only; khr_sync, then the same bytes
    for n, dt, _ in st.ctx.RENDER_FIELDS:
        dev[n].free()
        dev[n] = DeviceArray(np.full(host[n].shape, 9, dt))
    rc, stats = st.ctx.render_view_into(rq, {n: d.data_ptr() for n, d in dev.items()}, on_device=True, want_stats=False)
    assert rc == 0 and stats is None
    st.ctx.sync()
    for n in IMAGES:
        assert dev[n].read(0, host[n].nbytes).tobytes() == host[n].tobytes(), n
        dev[n].free()
    # NULL outputs: none at all, then a single image
    rc, stats = st.ctx.render_view_into(rq, {})
    assert rc == 0 and stats == host["stats"]
    only = {"status": np.full(host["status"].shape, 7, np.uint8)}
    rc, stats = st.ctx.render_view_into(rq, only, want_stats=False)
    assert rc == 0 and only["status"].tobytes() == host["status"].tobytes()
    # an explicit min_weight goes through to the observed test (the replica with the same value)
    heavy = st.ctx.render_view(sensor, pose, step_voxels=step, min_weight=3.0)
    replica(st, "ctx", sensor, pose, step)  # (builds the block set if this test runs alone)
    want = rr.render(None, None, st.cfg.voxels_per_side, st.cfg.voxel_size, sensor, pose, step_voxels=step, min_weight=3.0,
                     blocks=st.cache["ctx"])
    assert_same_images(heavy, want, "min_weight 3")
    assert heavy["stats"]["n_hit"] != host["stats"]["n_hit"]


@pytest.mark.gpu
def test_error_codes_leave_the_buffers_untouched(stream):
    st = stream
    pose = st.last["pose"]

    def sensor(**kw):
        d = dict(width=32, height=24, fx=16.0, fy=16.0, cx=16.0, cy=12.0, min_range=0.1, max_range=5.0)
        d.update(kw)
        return FusionContext.make_sensor(**d)

    nan_pose = pose.copy()
    nan_pose[1, 3] = np.nan
    inf_pose = pose.copy()
    inf_pose[0, 0] = np.inf
    cases = {
        "null request": None,
        "nan pose": st.ctx.render_request(sensor(), nan_pose),
        "inf pose": st.ctx.render_request(sensor(), inf_pose),
        "zero width": st.ctx.render_request(sensor(width=0), pose),
        "negative height": st.ctx.render_request(sensor(height=-24), pose),
        "max below min": st.ctx.render_request(sensor(min_range=2.0, max_range=1.0), pose),
        "negative min": st.ctx.render_request(sensor(min_range=-0.1), pose),
        "negative step": st.ctx.render_request(sensor(), pose, -0.5),
        # 0.01 voxel = 1 mm steps over 70 m: 70001 samples per ray
        "too many samples": st.ctx.render_request(sensor(max_range=70.1), pose, 0.01),
    }
    for what, rq in cases.items():
        out = {n: np.full((24, 32) + sh, 7, dt) for n, dt, sh in st.ctx.RENDER_FIELDS}
        rc, stats = st.ctx.render_view_into(rq, out)
        assert rc == KHR_EINVAL and stats is None, (what, rc)
        for n, a in out.items():
            assert (a == 7).all(), (what, n)
    # 65536 samples per ray are still accepted: 0.01-voxel steps over 65.535 m + the sample at min_range
    rc, stats = st.ctx.render_view_into(st.ctx.render_request(FusionContext.make_sensor(2, 2, 1.0, 1.0, 1.0, 1.0, 0.0, 65.535), pose, 0.01), {})
    assert rc == 0 and stats["n_samples_total"] <= 4 * 65536
    # a shard cannot render
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=64 * 48, rank=0, world_size=2)
    shard = FusionContext(cfg)
    out = {"depth": np.full((24, 32), 7, np.float32)}
    rc, stats = shard.render_view_into(shard.render_request(sensor(), pose), out)
    assert rc == KHR_ESTATE and (out["depth"] == 7).all()
    shard.close()


@pytest.mark.gpu
def test_8vps_context_without_semantics():
    st = run_stream(n_frames=12, archive_every=0, voxels_per_side=8, voxel_size=0.05, truncation_distance=0.15, max_blocks=16384,
                    with_semantics=0)
    for name in ("own", "moved"):
        sensor, pose, step = views(st.last["pose"], small_sensor())[name]
        got = st.ctx.render_view(sensor, pose, step_voxels=step)
        mine = replica(st, "ctx", sensor, pose, step)
        assert mine["n_hit"] > 1000, (name, mine["n_hit"])
        assert_same_images(got, mine, "8^3 %s / download_block" % name)
        assert_same_images(got, replica(st, "ora", sensor, pose, step), "8^3 %s / oracle" % name)
        assert not got["label"].any()


@pytest.mark.gpu
def test_without_tracking():
    st = run_stream(n_frames=6, archive_every=0, with_tracking=0)
    sensor, pose, step = views(st.last["pose"], small_sensor())["own"]
    got = st.ctx.render_view(sensor, pose, step_voxels=step)
    mine = replica(st, "ctx", sensor, pose, step)
    assert mine["n_hit"] > 1000
    assert_same_images(got, mine, "no tracking")
    assert (got["label"] != 0).any()


def image_digest(a):
    """aw_demo's imageDigest: sum_i mix(i * L + byte_i) mod 2^64"""
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(_mix64(np.arange(b.size, dtype=np.uint64) * np.uint64(0x632BE59BD9B4E019) + b).sum(dtype=np.uint64))


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
def test_aw_demo_render_mode_equals_the_python_path(tmp_path):
    """aw_demo --render: a Khronos sink renders the map at the last frame's pose (VolumetricMap::render(frame)); the same stream
    stepped through the C ABI as ActiveWindow::spinOnce steps it (tests/test_gpu_host.py) gives the same image digests"""
    W, H, N = 320, 240, 14
    cfgp = tmp_path / "aw_render.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--render", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N
    assert res["shapes"] == {"depth": [H, W], "normal": [H, W, 3], "color": [H, W, 4], "label": [H, W], "flags": [H, W], "status": [H, W]}
    cfg, ctx, ora, s, sen, osen = make_pair(width=W, height=H, temporal_window=0.75, truncation_distance=0.3,
                                            md_min_cluster_size=20, md_min_separation_distance=2.0, md_max_range=5.0)
    last_full, view = 0, None
    for i in range(N):
        fr = s.render(i)
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        ctx.detect_motion(slot)
        ctx.integrate(slot, allocate_blocks=True, use_mask=True)
        ctx.update_tracking(fr["stamp"])
        if i == N - 1:  # the sinks run before the frame's output and its archival (active_window.cpp:152 before :163)
            view = ctx.render_view(sen, fr["pose"])
        if not (last_full + int(float(np.float32(0.4)) * 1e9) > fr["stamp"]):
            ctx.generate_mesh(True, True)
            ctx.reset_inactive()
            ctx.clear_updated()
            last_full = fr["stamp"]
    assert view["stats"]["n_hit"] > 1000
    assert res["stats"]["n_hit"] == view["stats"]["n_hit"] and res["stats"]["n_blocked"] == view["stats"]["n_blocked"]
    assert res["stats"]["n_samples_total"] == view["stats"]["n_samples_total"]
    for k in IMAGES:
        assert res["digests"][k] == "%016x" % image_digest(view[k]), k
