"""khr_merge_map (FusionContext.merge_map; ASSUMPTIONS.md A.17): another context's map fused into the live map on the device.
The hand-built cases of tests/merge_cases.py, a fused map with deferred stamps, life after a merge, partial meshing, errors
(each leaves the destination's digest as it was) and resources -- every map comparison byte for byte against the numpy replica
(tests/merge_replica.py) through the checkpoint stream."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import merge_cases as mc
import merge_replica as mr
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ENOMEM, KHR_ESTATE, KHR_MERGE_ALIGNED, KHR_MERGE_RESAMPLE, KhrConfig, live_resources

pytestmark = pytest.mark.gpu
MESH_FIELDS = ("points", "colors", "labels", "first_seen", "stamps")


def clone_cfg(cfg, **kw):
    out = KhrConfig()
    C.memmove(C.byref(out), C.byref(cfg), C.sizeof(KhrConfig))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def make_cfg(fields, **kw):
    base = dict(max_blocks=64, max_frame_pixels=64 * 48, exact_arithmetic=1, max_weight=float(mc.MAX_WEIGHT))
    base.update(fields)
    base.update(kw)
    return default_config(**base)


def load(fields, idx, layers, **kw):
    cfg = make_cfg(fields, **kw)
    ctx = FusionContext(cfg)
    if len(idx):
        assert ctx.load_map(ck.pack(cfg, idx, layers)) == len(idx)
    return ctx


def last_error(ctx):
    return ctx.lib.khr_last_error().decode()


def digests_equal(a, b):
    return [hex(int(x)) for x in a] == [hex(int(x)) for x in b]


def assert_stream(got, want, what):
    """two checkpoint streams section by section, then as a whole"""
    gh, gi, gl = ck.unpack(got)
    wh, wi, wl = ck.unpack(want)
    assert gi.tolist() == wi.tolist(), (what, "block sets", gi.tolist(), wi.tolist())
    for k in wl:
        if gl[k].tobytes() != wl[k].tobytes():
            bad = np.argwhere(gl[k].view(np.uint8 if gl[k].dtype != np.uint64 else np.uint64) != wl[k].view(np.uint8 if wl[k].dtype != np.uint64 else np.uint64))
            raise AssertionError((what, k, len(bad), "first (block, voxel, ..)", bad[:4].tolist(), gi[bad[0][0]].tolist(),
                                  gl[k][tuple(bad[0][:2])] if gl[k].ndim > 1 else gl[k][bad[0][0]], wl[k][tuple(bad[0][:2])] if wl[k].ndim > 1 else wl[k][bad[0][0]]))
    assert got == want, what


@functools.lru_cache(maxsize=None)
def expected(name):
    """the replica's result for a case, computed once: (stream, statistics)"""
    c = mc.BY_NAME[name]
    idx, layers, stats = mc.replica_of(c)
    return ck.pack(c["cfg"], idx, layers), stats


def merge_case(dst, src, c):
    return dst.merge_map(src, mode=c["mode"], voxel_offset=c["voxel_offset"], pose=c["pose"], min_weight=c["min_weight"])


@pytest.mark.parametrize("packed", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=lambda p: "rows%d%d" % p)
@pytest.mark.parametrize("name", [c["name"] for c in mc.CASES])
def test_cases(name, packed):
    c = mc.BY_NAME[name]
    want, want_stats = expected(name)
    dst = load(c["cfg"], *c["dst"], packed_likelihood_rows=packed[0])
    src = load(c["cfg"], *c["src"], packed_likelihood_rows=packed[1])
    src_before = src.map_digest()
    stats = merge_case(dst, src, c)
    print(name, stats)
    assert stats == want_stats
    assert_stream(dst.save_map(), want, name)
    assert digests_equal(src.map_digest(), src_before)  # (the source is only read)
    src.close()
    dst.close()


def test_empty_source_and_untouched_merge():
    c = mc.BY_NAME["zero_offset"]
    dst = load(c["cfg"], *c["dst"])
    before = dst.save_map()
    empty = load(c["cfg"], np.zeros((0, 3), np.int32), {})
    assert dst.merge_map(empty) == dict.fromkeys(mr.STATS, 0)
    zero = load(c["cfg"], *mc.rich_map(c["cfg"], [((0, 0, 0), "zero"), ((9, 9, 9), "zero")], 7))
    st = dst.merge_map(zero, min_weight=0.5)
    assert st == dict(dict.fromkeys(mr.STATS, 0), n_src_blocks=2, n_candidate_blocks=2)
    assert dst.save_map() == before
    for x in (dst, empty, zero):
        x.close()


@pytest.fixture(scope="module")
def fused():
    """a map fused from 3 frames at 64 x 48 / 10 cm with tracking (deferred stamps, VOX_OCC voxels), a small hand-built source over
    some of its blocks and a new one merged into it (ALIGNED), and the replica applied to the stream saved before"""
    from common import make_pair
    cfg, ctx, ora, s, sen, osen = make_pair(width=64, height=48, max_blocks=1024)
    ora.close()
    for i in range(3):
        fr = s.render(i)
        ctx.integrate(ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"]))
        ctx.update_tracking(fr["stamp"])
    before = ctx.save_map()
    h, idx, layers = ck.unpack(before)
    fields = {k: h[k] for k in ck.CONFIG_FIELDS}
    obs = np.flatnonzero((layers["weight"] > 0).sum(axis=1) > 200)
    assert len(obs) >= 4
    picks = [tuple(int(v) for v in idx[i]) for i in obs[:: max(1, len(obs) // 6)][:6]]
    far = (int(idx[:, 0].max()) + 3, 0, 0)
    stamp = int(layers["last_observed"].max())
    sidx, sl = mc.rich_map(fields, [(b, "rich") for b in picks] + [(far, "rich")], 11)
    sl["last_observed"] = (sl["last_observed"] // np.uint64(40) + np.uint64(stamp - 10_000_000)).astype(np.uint64)  # around the map's stamps
    sl["last_occupied"] = (sl["last_occupied"] // np.uint64(40) + np.uint64(stamp - 10_000_000)).astype(np.uint64)
    src = FusionContext(clone_cfg(cfg, max_blocks=64))
    assert src.load_map(ck.pack(fields, sidx, sl)) == len(sidx)
    stats = ctx.merge_map(src, min_weight=float(mc.MIN_WEIGHT))
    widx, wl, wstats = mr.merge(fields, idx, layers, sidx, sl, min_weight=float(mc.MIN_WEIGHT), max_weight=float(cfg.max_weight))
    yield dict(cfg=cfg, ctx=ctx, src=src, stream=s, sensor=sen, stats=stats, want_stats=wstats, want=ck.pack(fields, widx, wl), before=before,
               fields=fields)
    src.close()
    ctx.close()


def test_lazy_forms(fused):
    """the destination holds deferred last_observed stamps and VOX_OCC voxels: resolved for the touched blocks as a save resolves them"""
    f = fused
    print(f["stats"])
    assert f["stats"] == f["want_stats"] and f["stats"]["n_merged_voxels"] > 0 and f["stats"]["n_new_blocks"] == 1
    assert_stream(f["ctx"].save_map(), f["want"], "fused map")


def test_life_after_the_merge(fused):
    """the merged context and a fresh one that loads the replica's result take the same steps to the same map, removed list and mesh:
    the derived words of the touched blocks are consistent"""
    f = fused
    fresh = FusionContext(clone_cfg(f["cfg"]))
    assert fresh.load_map(f["want"]) > 0
    fr = f["stream"].render(3)
    out = []
    for c in (f["ctx"], fresh):
        c.integrate(c.upload_frame(f["sensor"], fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"]))
        c.update_tracking(fr["stamp"])
        c.generate_mesh(only_mesh_updated=False)
        removed = c.reset_inactive()
        mesh = c.fetch_mesh()
        out.append((c.map_digest(), sorted(map(tuple, removed.tolist())), {k: mesh[k].tobytes() for k in MESH_FIELDS}, c.save_map()))
    fresh.close()
    assert digests_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]
    assert len(out[0][2]["points"]) > 0 and out[0][2] == out[1][2]
    assert out[0][3] == out[1][3]


def test_partial_meshing_regenerates_the_touched_blocks():
    """generate_mesh(only_mesh_updated=True) directly after a merge: MESH_UPDATED sits on exactly the touched blocks, and the mesh
    equals the full meshing of the merged map (the untouched block (5, 5, 5) has no touched neighbour; its mesh is carried over)"""
    cfg = mc.CFG16
    didx, dl = mc.rich_map(cfg, [((0, 0, 0), "solid"), ((5, 5, 5), "solid")], 21)
    dl["block_flags"][:] = 0
    sidx, sl = mc.rich_map(cfg, [((0, 0, 0), "solid"), ((0, 0, 1), "solid")], 22)
    dst, src = load(cfg, didx, dl), load(cfg, sidx, sl)
    dst.generate_mesh(only_mesh_updated=False)
    assert all(dst.download_block(b)["block_flags"] & 2 == 0 for b in dst.block_indices())
    st = dst.merge_map(src, min_weight=0.5)
    assert st["n_touched_blocks"] == 2 and st["n_new_blocks"] == 1
    flagged = [tuple(b.tolist()) for b in dst.block_indices() if dst.download_block(b)["block_flags"] & 2]
    assert flagged == [(0, 0, 0), (0, 0, 1)]
    dst.generate_mesh(only_mesh_updated=True)
    part = dst.fetch_mesh()
    full_ctx = load(cfg, *ck.unpack(dst.save_map())[1:])
    full_ctx.generate_mesh(only_mesh_updated=False)
    full = full_ctx.fetch_mesh()
    assert len(part["points"]) > 100
    for k in MESH_FIELDS:
        assert part[k].tobytes() == full[k].tobytes(), k
    for x in (dst, src, full_ctx):
        x.close()


def _pose(**kw):
    T = np.eye(4)
    for k, v in kw.items():
        T[int(k[1]), int(k[2])] = v
    return T


BAD_REQUESTS = {
    "mode": (dict(mode=7), "mode"),
    "min_weight_negative": (dict(min_weight=-1.0), "min_weight"),
    "min_weight_nan": (dict(min_weight=float("nan")), "min_weight"),
    "min_weight_inf": (dict(min_weight=float("inf")), "min_weight"),
    "offset_high": (dict(voxel_offset=(0, 2 ** 30, 0)), "voxel_offset[1]"),
    "offset_low": (dict(voxel_offset=(0, 0, -(2 ** 30))), "voxel_offset[2]"),
    "pose_nan": (dict(mode=KHR_MERGE_RESAMPLE, pose=_pose(m03=float("nan"))), "finite"),
    "pose_last_row": (dict(mode=KHR_MERGE_RESAMPLE, pose=_pose(m33=2.0)), "last row"),
    "pose_scaled": (dict(mode=KHR_MERGE_RESAMPLE, pose=_pose(m00=1.001)), "rigid"),
    "pose_reflection": (dict(mode=KHR_MERGE_RESAMPLE, pose=_pose(m22=-1.0)), "reflection"),
    "key_range": (dict(voxel_offset=(2 ** 30 - 16, 0, 0), min_weight=0.5), "outside the block index range"),
}
CONFIG_DIFFS = {"voxel_size": 0.05, "voxels_per_side": 8, "truncation_distance": 0.25, "with_semantics": 0, "with_tracking": 0, "num_labels": 6,
                "semantic_mode": 1}


@pytest.fixture(scope="module")
def pair():
    c = mc.BY_NAME["zero_offset"]
    dst, src = load(c["cfg"], *c["dst"]), load(c["cfg"], *c["src"])
    yield dst, src, dst.map_digest()
    src.close()
    dst.close()


@pytest.mark.parametrize("what", sorted(BAD_REQUESTS))
def test_bad_requests(pair, what):
    dst, src, digest = pair
    kw, text = BAD_REQUESTS[what]
    rc, st = dst.merge_map_rc(src, dst.merge_request(kw.get("mode", KHR_MERGE_ALIGNED), kw.get("voxel_offset", (0, 0, 0)), kw.get("pose"), kw.get("min_weight", 0.0)))
    assert rc == KHR_EINVAL and text in last_error(dst), (rc, last_error(dst))
    assert digests_equal(dst.map_digest(), digest)


def test_null_arguments_and_self(pair):
    dst, src, digest = pair
    rq = dst.merge_request(KHR_MERGE_ALIGNED)
    for s, r in ((None, rq), (src, None), (dst, rq)):
        rc, _ = dst.merge_map_rc(s, r)
        assert rc == KHR_EINVAL and ("null" in last_error(dst) or "same context" in last_error(dst)), last_error(dst)
    assert dst.lib.khr_merge_map(None, src.h, C.byref(rq), None) == KHR_EINVAL
    assert digests_equal(dst.map_digest(), digest)


@pytest.mark.parametrize("field", sorted(CONFIG_DIFFS))
def test_configuration_differences_name_the_field(pair, field):
    dst, src, digest = pair
    kw = {field: CONFIG_DIFFS[field]}
    if field == "semantic_mode":
        kw["num_labels"] = 2
        other_dst = FusionContext(make_cfg(mc.CFG16, num_labels=2))  # (the binary integrator wants two labels: only the mode differs)
    else:
        other_dst = None
    other = FusionContext(make_cfg(mc.CFG16, **kw))
    d = other_dst or dst
    rc, _ = d.merge_map_rc(other, d.merge_request(KHR_MERGE_ALIGNED))
    assert rc == KHR_EINVAL and field in last_error(d), (rc, last_error(d))
    assert digests_equal(dst.map_digest(), digest)
    other.close()
    if other_dst:
        other_dst.close()


def test_sharded_contexts_are_refused(pair):
    dst, src, digest = pair
    sharded = FusionContext(make_cfg(mc.CFG16, rank=0, world_size=2))
    rq = dst.merge_request(KHR_MERGE_ALIGNED)
    rc, _ = dst.merge_map_rc(sharded, rq)
    assert rc == KHR_ESTATE and "world_size" in last_error(dst)
    rc, _ = sharded.merge_map_rc(src, rq)
    assert rc == KHR_ESTATE and "world_size" in last_error(sharded)
    assert digests_equal(dst.map_digest(), digest)
    sharded.close()


def test_pool_one_short_and_exactly_enough():
    c = mc.BY_NAME["zero_offset"]
    want, want_stats = expected("zero_offset")
    need = len(c["dst"][0]) + want_stats["n_new_blocks"]
    src = load(c["cfg"], *c["src"])
    short = load(c["cfg"], *c["dst"], max_blocks=need - 1)
    digest = short.map_digest()
    rc, _ = short.merge_map_rc(src, short.merge_request(KHR_MERGE_ALIGNED, min_weight=c["min_weight"]))
    assert rc == KHR_ENOMEM, (rc, last_error(short))
    assert "%d new blocks" % want_stats["n_new_blocks"] in last_error(short) and "%d free" % (want_stats["n_new_blocks"] - 1) in last_error(short)
    assert digests_equal(short.map_digest(), digest)
    exact = load(c["cfg"], *c["dst"], max_blocks=need)
    rc, _ = exact.merge_map_rc(src, exact.merge_request(KHR_MERGE_ALIGNED, voxel_offset=(0, 0, 2 ** 30)))  # a failed merge first ...
    assert rc == KHR_EINVAL
    assert merge_case(exact, src, c) == want_stats  # ... then the merge succeeds, with exactly enough blocks
    assert_stream(exact.save_map(), want, "exactly enough blocks")
    for x in (src, short, exact):
        x.close()


def test_resources():
    """the scratch belongs to the destination: a repeat merge of the same size allocates nothing, and nothing outlives the contexts"""
    import gc
    gc.collect()
    start = live_resources()
    c = mc.BY_NAME["block_offset"]
    dst, src = load(c["cfg"], *c["dst"]), load(c["cfg"], *c["src"])
    idle = live_resources()
    merge_case(dst, src, c)
    first = live_resources()
    assert first != idle
    merge_case(dst, src, c)
    assert live_resources() == first
    src.close()
    dst.close()
    assert live_resources() == start


def test_aw_demo_merge_mode_equals_its_host_merge_and_the_python_path(tmp_path):
    """aw_demo --merge: two ActiveWindows take half of the stream each, the second map is merged into the first through
    hydra::VolumetricMap::merge and, from block copies, on one host thread: equal layer for layer.  The same two half streams stepped
    through the C ABI as ActiveWindow::spinOnce steps them give the same statistics from FusionContext.merge_map."""
    from common import make_pair
    from test_gpu_render_view import YAML
    W, H, N = 320, 240, 14
    cfgp = tmp_path / "aw_merge.yaml"
    cfgp.write_text(YAML)
    demo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khronos_amd", "lib", "aw_demo")
    out = subprocess.run([demo, "--merge", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N and res["equal"] is True and res["first_mismatch"] == ""
    assert res["n_merged_voxels"] > 0 and res["n_new_blocks"] > 0
    ctxs = []
    for half in (range(0, N // 2), range(N // 2, N)):
        cfg, ctx, ora, s, sen, osen = make_pair(width=W, height=H, temporal_window=0.75, truncation_distance=0.3, exact_arithmetic=1,
                                                md_min_cluster_size=20, md_min_separation_distance=2.0, md_max_range=5.0)
        ora.close()
        last_full = 0
        for i in half:
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
        ctxs.append(ctx)
    assert ctxs[0].num_blocks() == res["n_dst_blocks"]
    mine = ctxs[0].merge_map(ctxs[1])
    for c in ctxs:
        c.close()
    assert mine == {k: res[k] for k in mine}
