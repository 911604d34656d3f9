"""khr_diff_map (FusionContext.diff_map; ASSUMPTIONS.md A.18): the voxels that appeared or vanished in the live map against another
context's map, found on the device.  The hand-built pairs of tests/diff_cases.py, a fused map with deferred stamps against an edited
copy of its own checkpoint, the two forms of khr_diff_map_into and the life of the result, errors (each leaves both digests as
they were) and resources -- every array and statistic byte for byte against the numpy replica (tests/diff_replica.py), which is
fed with the two contexts' own checkpoint streams."""
import ctypes as C
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import diff_cases as dc
import diff_replica as dr
import merge_cases as mc
from khronos_amd import FusionContext, checkpoint as ck
from khronos_amd.capi import KHR_EINVAL, KHR_ESTATE, KHR_MERGE_RESAMPLE, KHR_OK, live_resources
from test_gpu_merge_map import CONFIG_DIFFS, _pose, clone_cfg, digests_equal, last_error, load, make_cfg

pytestmark = pytest.mark.gpu
ARRAYS = dr.VOXEL_FIELDS + dr.BLOCK_FIELDS


def replica_from_streams(now, then, mesh_min_weight=1e-4, **kw):
    """the replica on what the two contexts save"""
    hn, ni, nl = ck.unpack(now.save_map())
    ht, ti, tl = ck.unpack(then.save_map())
    fields = {k: hn[k] for k in ck.CONFIG_FIELDS}
    return dr.diff(fields, ni, nl, ti, tl, mesh_min_weight=mesh_min_weight, **kw)


def assert_result(got, want, what):
    print(what, got["stats"])
    assert got["stats"] == want["stats"], (what, got["stats"], want["stats"])
    for name, dt, sh in ARRAYS:
        g, w = got[name], want[name]
        assert g.dtype == dt and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first rows", bad[:4].tolist(), g[bad[:4]].tolist(), w[bad[:4]].tolist()))


def diff_checked(now, then, what, mesh_min_weight=1e-4, **kw):
    """a diff with both digests checked; returns (result, replica's result)"""
    before = now.map_digest(), then.map_digest()
    got = now.diff_map(then, **kw)
    assert digests_equal(now.map_digest(), before[0]) and digests_equal(then.map_digest(), before[1]), what
    want = replica_from_streams(now, then, mesh_min_weight=mesh_min_weight, **kw)
    assert_result(got, want, what)
    return got, want


@pytest.mark.parametrize("name", [c["name"] for c in dc.CASES])
def test_cases(name):
    c = dc.BY_NAME[name]
    now, then = load(c["cfg"], *c["now"]), load(c["cfg"], *c["then"])
    got, _ = diff_checked(now, then, name, **dc.request_of(c))
    if name == "order":  # (the case is about five changed blocks whose sorted order is not the order of their keys)
        assert list(map(tuple, got["blocks"].tolist())) == sorted(dc.ORDER_BLOCKS)
    if name == "all_changed":
        assert got["stats"]["n_appeared"] == 4096 and got["block_first"].tolist() == [0]
    then.close()
    now.close()


def test_empty_ref_and_a_ref_of_zero_weights():
    c = dc.BY_NAME["zero_offset"]
    now = load(c["cfg"], *c["now"])
    empty = load(c["cfg"], np.zeros((0, 3), np.int32), {})
    r = now.diff_map(empty)
    assert r["stats"] == dict.fromkeys(dr.STATS, 0) and all(len(r[k]) == 0 for k, _, _ in ARRAYS)
    zero = load(c["cfg"], *mc.rich_map(c["cfg"], [((0, 0, 0), "zero"), ((9, 9, 9), "zero")], 7))
    got, _ = diff_checked(now, zero, "zero weights", min_weight=0.5)
    st = got["stats"]
    assert st["n_ref_blocks"] == st["n_candidate_blocks"] == 2 and st["n_present_blocks"] == 1 and st["n_compared_voxels"] == 0 and st["n_only_now"] > 0
    for x in (now, empty, zero):
        x.close()


@pytest.fixture(scope="module")
def fused():
    """a map fused from 3 frames at 64 x 48 / 10 cm with tracking (deferred stamps, VOX_OCC voxels) as `now`; `then` is a hand-edited
    copy of its own checkpoint: the distances of some blocks mirrored (what was occupied is free and the reverse), earlier stamps,
    other labels, one block's weights zeroed, one block dropped and a far one added"""
    from common import make_pair
    cfg, ctx, ora, s, sen, osen = make_pair(width=64, height=48, max_blocks=1024)
    ora.close()
    for i in range(3):
        fr = s.render(i)
        ctx.integrate(ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"]))
        ctx.update_tracking(fr["stamp"])
    h, idx, layers = ck.unpack(ctx.save_map())
    fields = {k: h[k] for k in ck.CONFIG_FIELDS}
    obs = np.flatnonzero((layers["weight"] > 0).sum(axis=1) > 200)
    assert len(obs) >= 4
    edited = {k: np.array(v) for k, v in layers.items()}
    for i in obs[::2]:
        edited["distance"][i] = -layers["distance"][i]
        edited["last_observed"][i] = layers["last_observed"][i] - np.minimum(layers["last_observed"][i], np.uint64(70_000_000))
        edited["sem_label"][i] = (layers["sem_label"][i] + 1) % np.uint32(max(1, fields["num_labels"]))
    edited["weight"][obs[3]] = 0  # (a block `then` holds but never observed: its voxels are ONLY_NOW)
    keep = np.ones(len(idx), bool)
    keep[obs[1]] = False
    tidx = idx[keep]
    tl = {k: v[keep] for k, v in edited.items()}
    far_i, far_l = mc.rich_map(fields, [((int(idx[:, 0].max()) + 3, 0, 0), "rich")], 11)
    tidx = np.concatenate([tidx, far_i])
    tl = {k: np.concatenate([tl[k], far_l[k].astype(tl[k].dtype)]) for k in tl}
    then = FusionContext(clone_cfg(cfg))
    assert then.load_map(ck.pack(fields, tidx, tl)) == len(tidx)
    yield dict(cfg=cfg, now=ctx, then=then, stream=s, sensor=sen, n_blocks=len(idx))
    then.close()
    ctx.close()


def test_fused_map_against_an_edited_copy(fused):
    f = fused
    got, _ = diff_checked(f["now"], f["then"], "fused", mesh_min_weight=float(f["cfg"].mesh_min_weight))
    st = got["stats"]
    assert st["n_appeared"] > 0 and st["n_disappeared"] > 0 and st["n_only_now"] > 0
    assert st["n_candidate_blocks"] == f["n_blocks"] and st["n_present_blocks"] == f["n_blocks"] - 1
    assert (got["stamp_now"] > 0).all() and (got["stamp_then"] <= got["stamp_now"]).all() and (got["stamp_then"] != got["stamp_now"]).any()


def test_into_forms_and_the_life_of_the_result(fused):
    f = fused
    now, then = f["now"], f["then"]
    ref = now.diff_map(then)
    n, m = len(ref["kind"]), len(ref["blocks"])
    assert n > 0 and m > 0

    def host_copy(names=None):
        out = {k: np.zeros((n if w == "v" else m,) + sh, dt) for k, dt, sh, w in now.DIFF_FIELDS}
        for a in out.values():
            a.view(np.uint8)[...] = 0xAB
        assert now.diff_map_into({k: v for k, v in out.items() if names is None or k in names}) == KHR_OK
        return out

    full = host_copy()
    for k, _, _ in ARRAYS:
        assert full[k].tobytes() == ref[k].tobytes(), k
    part = host_copy(names=("kind", "block_first"))  # NULL pointers are skipped; the call can be repeated
    for k, _, _ in ARRAYS:
        if k in ("kind", "block_first"):
            assert part[k].tobytes() == ref[k].tobytes(), k
        else:
            assert (part[k].view(np.uint8) == 0xAB).all(), k
    # the device form: device-to-device in stream order (device arrays through the runtime the library is linked against)
    from common import DeviceArray
    dev = {k: DeviceArray(np.zeros((n if w == "v" else m,) + sh, dt)) for k, dt, sh, w in now.DIFF_FIELDS}
    assert now.diff_map_into({k: d.data_ptr() for k, d in dev.items()}, on_device=True) == KHR_OK
    now.sync()
    for k, _, _ in ARRAYS:
        assert dev[k].read(0, ref[k].nbytes).tobytes() == ref[k].tobytes(), k
    for d in dev.values():
        d.free()
    # the result survives a frame and a meshing ...
    fr = f["stream"].render(3)
    now.integrate(now.upload_frame(f["sensor"], fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"]))
    now.update_tracking(fr["stamp"])
    now.generate_mesh(only_mesh_updated=False)
    later = host_copy()
    for k, _, _ in ARRAYS:
        assert later[k].tobytes() == ref[k].tobytes(), k
    # ... a failed diff discards it, a new diff brings one back
    rc, _ = now.diff_map_rc(then, now.diff_request(mode=7))
    assert rc == KHR_EINVAL
    assert now.diff_map_into({}) == KHR_ESTATE and "khr_diff_map" in last_error(now)
    diff_checked(now, then, "after a frame", mesh_min_weight=float(f["cfg"].mesh_min_weight))
    assert now.diff_map_into({}) == KHR_OK


def test_no_result_before_a_diff_and_after_a_reset():
    c = dc.BY_NAME["one_block"]
    now, then = load(c["cfg"], *c["now"]), load(c["cfg"], *c["then"])
    assert now.diff_map_into({}) == KHR_ESTATE
    assert now.diff_map(then, **dc.request_of(c))["stats"]["n_changed_blocks"] == 1
    assert now.diff_map_into({}) == KHR_OK
    now.reset_map(c["cfg"]["voxel_size"], c["cfg"]["truncation_distance"])
    assert now.diff_map_into({}) == KHR_ESTATE
    then.close()
    now.close()


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
    "occupied_nan": (dict(occupied_distance=float("nan")), "occupied_distance"),
    "free_inf": (dict(free_distance=float("inf")), "free_distance"),
    "occupied_equals_free": (dict(occupied_distance=0.05, free_distance=0.05), "occupied_distance"),
    "occupied_above_free": (dict(occupied_distance=0.06, free_distance=0.05), "free_distance"),
}


@pytest.fixture(scope="module")
def pair():
    c = dc.BY_NAME["zero_offset"]
    now, then = load(c["cfg"], *c["now"]), load(c["cfg"], *c["then"])
    yield now, then, now.map_digest(), then.map_digest()
    then.close()
    now.close()


def unchanged(pair):
    now, then, dn, dt = pair
    return digests_equal(now.map_digest(), dn) and digests_equal(then.map_digest(), dt)


@pytest.mark.parametrize("what", sorted(BAD_REQUESTS))
def test_bad_requests(pair, what):
    now, then = pair[:2]
    kw, text = BAD_REQUESTS[what]
    rc, st = now.diff_map_rc(then, now.diff_request(**kw))
    assert rc == KHR_EINVAL and "khr_diff_map" in last_error(now) and text in last_error(now), (rc, last_error(now))
    assert st == dict.fromkeys(dr.STATS, 0) and unchanged(pair)


def test_null_arguments_and_self(pair):
    now, then = pair[:2]
    rq = now.diff_request()
    for t, r in ((None, rq), (then, None), (now, rq)):
        rc, _ = now.diff_map_rc(t, r)
        assert rc == KHR_EINVAL and ("null" in last_error(now) or "same context" in last_error(now)), last_error(now)
    assert now.lib.khr_diff_map(None, then.h, C.byref(rq), None) == KHR_EINVAL
    assert now.lib.khr_diff_map_into(None, 0, *([None] * 11)) == KHR_EINVAL
    assert unchanged(pair)


@pytest.mark.parametrize("field", sorted(CONFIG_DIFFS))
def test_configuration_differences_name_the_field(pair, field):
    now, then = pair[:2]
    kw = {field: CONFIG_DIFFS[field]}
    other_now = None
    if field == "semantic_mode":
        kw["num_labels"] = 2
        other_now = FusionContext(make_cfg(mc.CFG16, num_labels=2))  # (the binary integrator wants two labels: only the mode differs)
    other = FusionContext(make_cfg(mc.CFG16, **kw))
    d = other_now or now
    rc, _ = d.diff_map_rc(other, d.diff_request())
    assert rc == KHR_EINVAL and field in last_error(d), (rc, last_error(d))
    assert unchanged(pair)
    other.close()
    if other_now:
        other_now.close()


def test_sharded_contexts_are_refused(pair):
    now, then = pair[:2]
    sharded = FusionContext(make_cfg(mc.CFG16, rank=0, world_size=2))
    rc, _ = now.diff_map_rc(sharded, now.diff_request())
    assert rc == KHR_ESTATE and "world_size" in last_error(now)
    rc, _ = sharded.diff_map_rc(then, sharded.diff_request())
    assert rc == KHR_ESTATE and "world_size" in last_error(sharded)
    assert unchanged(pair)
    sharded.close()


def test_resources():
    """the scratch and the result belong to `now`: a repeat diff of the same size allocates nothing, a merge after it shares the
    scratch, and nothing outlives the contexts"""
    gc.collect()
    start = live_resources()
    c = dc.BY_NAME["block_offset"]
    now, then = load(c["cfg"], *c["now"]), load(c["cfg"], *c["then"])
    idle = live_resources()
    first_result = now.diff_map(then, **dc.request_of(c))
    first = live_resources()
    assert first != idle
    again = now.diff_map(then, **dc.request_of(c))
    assert live_resources() == first
    for k, _, _ in ARRAYS:
        assert again[k].tobytes() == first_result[k].tobytes(), k
    now.merge_map(then, voxel_offset=c["voxel_offset"], min_weight=c["min_weight"])
    assert live_resources() == first
    then.close()
    now.close()
    assert live_resources() == start


def test_aw_demo_diff_mode_equals_its_host_diff(tmp_path):
    """aw_demo --diff: one ActiveWindow takes the stream, halfway its map is checkpointed into a side context, at the end the live
    map is diffed against it through hydra::VolumetricMap::diff and, from block copies, on one host thread: equal list for list"""
    from test_gpu_render_view import YAML
    W, H, N = 64, 48, 8
    cfgp = tmp_path / "aw_diff.yaml"
    cfgp.write_text(YAML)
    demo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khronos_amd", "lib", "aw_demo")
    out = subprocess.run([demo, "--diff", str(cfgp), str(W), str(H), str(N)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N and res["equal"] is True and res["first_mismatch"] == ""
    assert res["n_present_blocks"] > 0 and res["n_compared_voxels"] > 0
