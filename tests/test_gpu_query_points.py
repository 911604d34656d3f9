"""khr_query_points / FusionContext.query_points: the live map at world points (ASSUMPTIONS.md A.13) -- trilinear distance, index-space
gradient and the attributes of the point's voxel -- held bit for bit to tests/query_replica.py over this context's block downloads
and over the CPU oracle's blocks, on the point sets tests/test_cpu_query_points.py fixes (tests/query_cases.py)."""
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import query_cases as qc
import query_replica as qr
from common import DeviceArray, make_pair, step_both
from khronos_amd import FusionContext, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ESTATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
FIELDS = FusionContext.QUERY_FIELDS
N_FRAMES = 30
GUARD = 64  # entries after each output buffer that a call must leave alone


def run_stream(n_frames=N_FRAMES, archive_every=5, **cfg_kw):
    """the stream of tests/test_gpu_map_slice.py / test_gpu_render_view.py: tracking and motion detection on, archival every few
    frames"""
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
    """the replica's block set over this context's downloads ("ctx") or the oracle's blocks ("ora"), built once per map state"""
    if which not in st.cache:
        src, get = (st.ctx, st.ctx.download_block) if which == "ctx" else (st.ora, st.ora.get_block)
        st.cache[which] = qr.QueryBlocks(src.block_indices(), get, st.cfg.voxels_per_side)
    return st.cache[which]


def replica(st, which, points, min_weight=None):
    return qr.query(blocks_of(st, which), points, st.cfg.voxel_size, st.cfg.mesh_min_weight if min_weight is None else min_weight,
                    with_semantics=bool(st.cfg.with_semantics), with_tracking=bool(st.cfg.with_tracking))


def point_sets(st):
    if "sets" not in st.cache:
        st.cache["sets"] = qc.all_sets(blocks_of(st, "ctx"), st.last, st.sen, st.cfg.voxel_size, st.cfg.truncation_distance, st.cfg.mesh_min_weight)
    return st.cache["sets"]


def assert_same(got, want, what):
    for k, dt, sh in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))
            raise AssertionError((what, k, len(bad), bad[:4].tolist(), got[k][bad[:4]].tolist(), want[k][bad[:4]].tolist()))
    assert got["stats"] == {k: want[k] for k in ("n_value", "n_gradient", "n_voxel")}, (what, got["stats"])


@pytest.fixture(scope="module")
def stream():
    return run_stream(temporal_window=0.6)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["surface", "box", "lattice", "bad", "mixed"])
def test_point_sets_match_the_replica_bit_for_bit(stream, name):
    st = stream
    pts = point_sets(st)[name]
    got = st.ctx.query_points(pts)
    mine = replica(st, "ctx", pts)
    print("%s: %d points, value %d gradient %d voxel %d" % (name, len(pts), mine["n_value"], mine["n_gradient"], mine["n_voxel"]))
    if name != "bad":
        assert mine["n_gradient"] > 0 and mine["n_value"] > mine["n_gradient"] and mine["n_voxel"] > mine["n_value"]
    assert_same(got, mine, name + " / download_block")
    assert_same(got, replica(st, "ora", pts), name + " / oracle")


@pytest.mark.gpu
def test_8vps_object_map_without_tracking():
    """the object mini-map configuration of tests/test_gpu_parity.py (vps 8, binary labels, no tracking, no label image): blocks
    allocated over a box, frames integrated without allocation"""
    cfg, ctx, ora, s, sen, osen = make_pair(voxels_per_side=8, voxel_size=0.04, truncation_distance=0.08, with_tracking=0, semantic_mode=1,
                                            num_labels=2)
    st = SimpleNamespace(cfg=cfg, ctx=ctx, ora=ora, s=s, sen=sen, osen=osen, last=None, cache={})
    fr0 = s.render(0)
    bl = np.array([[x, y, z] for x in range(2, 8) for y in range(-3, 3) for z in range(0, 6)], np.int32)
    ctx.allocate_blocks(bl)
    ora.allocate_blocks(bl)
    for i in range(4):
        fr = s.render(i)
        obj = (fr["label"] == fr0["label"][120, 160]).astype(np.int32) * 3
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], None)
        ctx.set_frame_image(slot, 1, obj)
        ctx.integrate(slot, allocate_blocks=False, use_mask=False, object_id=3)
        ora.integrate(osen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], None, object_image=obj, object_id=3, allocate_blocks=False)
        st.last = fr
    sets = point_sets(st)
    for name in ("box", "lattice", "mixed"):  # (the frame's own surface points lie outside the box: they are part of `mixed`)
        got = ctx.query_points(sets[name])
        mine = replica(st, "ctx", sets[name])
        print("8^3 %s: %d points, value %d gradient %d voxel %d" % (name, len(sets[name]), mine["n_value"], mine["n_gradient"], mine["n_voxel"]))
        assert mine["n_gradient"] > 0 and mine["n_voxel"] > mine["n_value"] > mine["n_gradient"]
        assert_same(got, mine, "8^3 %s / download_block" % name)
        assert_same(got, replica(st, "ora", sets[name]), "8^3 %s / oracle" % name)
        assert not got["last_observed"].any()
    ctx.close()


@pytest.mark.gpu
def test_without_tracking_and_semantics():
    st = run_stream(n_frames=6, archive_every=0, with_tracking=0, with_semantics=0)
    pts = point_sets(st)["mixed"]
    got = st.ctx.query_points(pts)
    mine = replica(st, "ctx", pts)
    assert mine["n_gradient"] > 1000
    assert_same(got, mine, "no tracking, no semantics / download_block")
    assert_same(got, replica(st, "ora", pts), "no tracking, no semantics / oracle")
    assert not got["label"].any() and not got["last_observed"].any() and got["color"].any()
    st.ctx.close()


@pytest.mark.gpu
def test_batch_sizes_cover_the_wave_and_workgroup_tails(stream):
    st = stream
    pts = point_sets(st)["mixed"]
    full = st.ctx.query_points(pts)
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        got = st.ctx.query_points(pts[:n])
        for k, dt, sh in FIELDS:
            assert got[k].shape == (n,) + sh and got[k].tobytes() == full[k][:n].tobytes(), (n, k)
        s = full["status"][:n]
        assert got["stats"] == {"n_value": int((s & 1 != 0).sum()), "n_gradient": int((s & 2 != 0).sum()), "n_voxel": int((s & 4 != 0).sum())}, n


def guarded(n, fields, fill=7):
    return {k: np.full((n + GUARD,) + sh, fill, dt) for k, dt, sh in FIELDS if k in fields}


@pytest.mark.gpu
def test_null_outputs_remove_their_columns_only(stream):
    st = stream
    pts = point_sets(st)["mixed"][:5000]
    n = len(pts)
    full = st.ctx.query_points(pts)
    assert full["stats"]["n_gradient"] > 0 and full["stats"]["n_voxel"] < n
    attrs = ("weight", "color", "label", "flags", "last_observed")
    variants = {"distance only": ("distance",), "gradient only": ("gradient",), "attributes only": attrs, "status only": ("status",),
                "everything": tuple(k for k, _, _ in FIELDS), "nothing": ()}
    for what, fields in variants.items():
        for want_stats in (True, False):
            out = guarded(n, fields)
            rc, stats = st.ctx.query_points_into(n, pts, out, want_stats=want_stats)
            assert rc == 0 and (stats == full["stats"] if want_stats else stats is None), (what, rc, stats)
            for k in fields:
                assert out[k][:n].tobytes() == full[k].tobytes(), (what, want_stats, k)
                assert (out[k][n:] == 7).all(), (what, want_stats, k)


@pytest.mark.gpu
def test_device_form_equals_the_host_form(stream):
    st = stream
    pts = point_sets(st)["mixed"][:5000]
    n = len(pts)
    host = st.ctx.query_points(pts)
    d_pts = DeviceArray(pts)
    for want_stats in (True, False):  # without counters: stream order only; khr_sync, then the same bytes
        dev = {k: DeviceArray(v) for k, v in guarded(n, [k for k, _, _ in FIELDS], fill=9).items()}
        rc, stats = st.ctx.query_points_into(n, d_pts.data_ptr(), {k: d.data_ptr() for k, d in dev.items()}, on_device=True, want_stats=want_stats)
        assert rc == 0 and (stats == host["stats"] if want_stats else stats is None)
        st.ctx.sync()
        for k, dt, sh in FIELDS:
            row = int(np.prod(sh, dtype=np.int64)) * np.dtype(dt).itemsize
            assert dev[k].read(0, n * row).tobytes() == host[k].tobytes(), k
            assert (dev[k].read(n * row, GUARD * row).view(dt) == 9).all(), k
            dev[k].free()
    # a single device output, the others NULL
    only = DeviceArray(np.full(n + GUARD, 9, np.float32))
    rc, stats = st.ctx.query_points_into(n, d_pts.data_ptr(), {"distance": only.data_ptr()}, on_device=True, want_stats=False)
    assert rc == 0
    st.ctx.sync()
    assert only.read(0, 4 * n).tobytes() == host["distance"].tobytes() and (only.read(4 * n, 4 * GUARD).view(np.float32) == 9).all()
    only.free()
    d_pts.free()


@pytest.mark.gpu
def test_an_explicit_min_weight_reaches_the_observed_test(stream):
    st = stream
    pts = point_sets(st)["surface"][::3]
    heavy = st.ctx.query_points(pts, min_weight=3.0)
    assert_same(heavy, replica(st, "ctx", pts, min_weight=3.0), "min_weight 3")
    assert heavy["stats"]["n_value"] != st.ctx.query_points(pts)["stats"]["n_value"]


@pytest.mark.gpu
def test_the_call_only_reads_and_repeats_identically(stream):
    st = stream
    digest, idx, stats = st.ctx.map_digest(), st.ctx.block_indices().copy(), st.ctx.stats()
    for name, pts in point_sets(st).items():
        a, b = st.ctx.query_points(pts), st.ctx.query_points(pts)
        for k, _, _ in FIELDS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        assert a["stats"] == b["stats"]
    assert np.array_equal(st.ctx.map_digest(), digest)
    assert np.array_equal(st.ctx.block_indices(), idx)
    assert st.ctx.stats() == stats


@pytest.mark.gpu
def test_queries_follow_archival():
    """the same points before and after a further reset_inactive() that removes blocks (the hash table is rebuilt): bit-exact
    against a replica over the new block set, and points lose their value with the blocks"""
    st = run_stream(temporal_window=0.6)
    sets = point_sets(st)
    pts = np.concatenate([sets["surface"][::7], sets["box"]])
    before = replica(st, "ctx", pts)
    assert_same(st.ctx.query_points(pts), before, "before")
    for i in range(N_FRAMES, N_FRAMES + 4):
        step(st, i)
    removed = np.asarray(st.ctx.reset_inactive())
    assert np.array_equal(removed, np.asarray(st.ora.reset_inactive())) and len(removed) > 0
    st.cache.clear()
    after = replica(st, "ctx", pts)
    lost = ((before["status"] & qr.QP_VALUE) != 0) & ((after["status"] & qr.QP_VALUE) == 0)
    print("archival removed %d blocks, %d of %d valued points lost their value" % (len(removed), lost.sum(), before["n_value"]))
    assert lost.sum() >= 1
    got = st.ctx.query_points(pts)
    assert_same(got, after, "after / download_block")
    assert_same(got, replica(st, "ora", pts), "after / oracle")
    st.ctx.close()


@pytest.mark.gpu
def test_error_codes_leave_the_buffers_untouched(stream):
    st = stream
    pts = point_sets(st)["box"][:100]
    n = len(pts)
    names = [k for k, _, _ in FIELDS]
    cases = {"negative n": dict(n=-1, points=pts), "null points": dict(n=n, points=None), "negative min_weight": dict(n=n, points=pts, min_weight=-1.0),
             "nan min_weight": dict(n=n, points=pts, min_weight=float("nan")), "inf min_weight": dict(n=n, points=pts, min_weight=float("inf"))}
    for what, kw in cases.items():
        out = guarded(n, names)
        rc, stats = st.ctx.query_points_into(kw["n"], kw["points"], out, min_weight=kw.get("min_weight", 0.0))
        assert rc == KHR_EINVAL and stats is None, (what, rc)
        for k, a in out.items():
            assert (a == 7).all(), (what, k)
    # the empty batch: fine, nothing touched (NULL points included), zeroed counters
    out = guarded(n, names)
    for p in (pts, None):
        rc, stats = st.ctx.query_points_into(0, p, out)
        assert rc == 0 and stats == {"n_value": 0, "n_gradient": 0, "n_voxel": 0}
    for k, a in out.items():
        assert (a == 7).all(), k
    # a shard cannot answer
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=64 * 48, rank=0, world_size=2)
    shard = FusionContext(cfg)
    out = guarded(n, names)
    rc, stats = shard.query_points_into(n, pts, out)
    assert rc == KHR_ESTATE and stats is None
    for k, a in out.items():
        assert (a == 7).all(), k
    shard.close()


@pytest.mark.gpu
def test_distance_changes_sign_across_the_frames_surface(stream):
    """independent of the replica: over the last frame's non-dynamic pixels the median queried distance is positive half a
    truncation distance in front of the observed surface, negative as far behind it, and below one voxel in magnitude on it (the
    CPU oracle's median there, tests/test_cpu_query_points.py: 0.0023 m at 0.1 m voxels)"""
    st = stream
    (at, front, behind), sel = qc.surface_points(st.last, st.sen, st.cfg.truncation_distance)
    static = np.asarray(st.last["step"]["dyn_gpu"]).ravel()[sel] == 0
    med = []
    for pts in (at, front, behind):
        got = st.ctx.query_points(pts)
        use = static & ((got["status"] & qr.QP_VALUE) != 0)
        assert use.sum() > 1000
        med.append(float(np.median(got["distance"][use])))
    print("median distance on / in front of / behind the surface: %.4f %.4f %.4f m" % tuple(med))
    assert med[1] > 0 and med[2] < 0 and abs(med[0]) < st.cfg.voxel_size


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
def test_aw_demo_query_mode_agrees_with_block_copies(tmp_path):
    """aw_demo --query: a Khronos sink asks the map about the frame's back-projected pixels through VolumetricMap::query and through
    a cloneBlock loop with A.13's arithmetic on the host, in image order and shuffled; the two agree bit for bit on every frame"""
    W, H, N = 320, 240, 8
    cfgp = tmp_path / "aw_query.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--query", str(cfgp), str(W), str(H), str(N), "20000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N and res["agree_frames"] == N and res["first_mismatch"] == ""
    assert res["points_mean"] == 20000 and res["last_stats"]["n_gradient"] > 1000
    assert res["last_stats"]["n_voxel"] >= res["last_stats"]["n_value"] >= res["last_stats"]["n_gradient"]
    assert res["device_query_ms"] > 0 and res["block_copy_ms"] > 0
