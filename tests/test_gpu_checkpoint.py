"""khr_checkpoint_save / khr_checkpoint_load (FusionContext.save_map / load_map): the live map as one slot-independent byte stream
and back.  Every comparison is bit-exact (exact arithmetic mode): whole-map digests, block lists, meshes, and -- across the save
point -- the CPU oracle, which never stops."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from common import PinnedArray, make_pair, step_both
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ENOMEM, KHR_ESTATE, KhrConfig
from test_gpu_map_slice import run_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
MESH_FIELDS = ("points", "colors", "labels", "first_seen", "stamps")
PUBLIC_LAYERS = ("distance", "weight", "color", "last_observed", "last_occupied", "flags", "sem_label")


def clone_cfg(cfg, **kw):
    out = KhrConfig()
    C.memmove(C.byref(out), C.byref(cfg), C.sizeof(KhrConfig))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def digests_equal(a, b):
    return [hex(int(x)) for x in a] == [hex(int(x)) for x in b]


def last_error(ctx):
    return ctx.lib.khr_last_error().decode()


def mesh_bytes(m):
    return {k: m[k].tobytes() for k in MESH_FIELDS}


@pytest.fixture(scope="module")
def saved():
    """the 30-frame stream of tests/test_gpu_map_slice.py (archival every 5 frames, blocks archived), and its checkpoint"""
    cfg, ctx, ora, removed = run_stream(temporal_window=0.6)
    assert len(removed) > 0
    blob = ctx.save_map()
    return cfg, ctx, ora, blob


@pytest.mark.gpu
def test_round_trip(saved):
    cfg, ctx, ora, blob = saved
    nbytes, nblocks = ctx.checkpoint_size()
    assert nbytes == len(blob) and nblocks == ctx.num_blocks() > 0
    fresh = FusionContext(clone_cfg(cfg))
    assert fresh.load_map(blob) == nblocks
    assert digests_equal(fresh.map_digest(), ctx.map_digest())
    assert np.array_equal(fresh.block_indices(), ctx.block_indices())
    for c in (ctx, fresh):
        c.generate_mesh(only_mesh_updated=False, clear_flag=False)
    ma, mb = ctx.download_mesh(), fresh.download_mesh()
    assert len(ma["points"]) > 0
    assert mesh_bytes(ma) == mesh_bytes(mb)
    # the decoded stream, field by field, against the per-block downloads
    h, idx, layers = ck.unpack(blob)
    assert np.array_equal(idx, ctx.block_indices())
    for k in ("voxel_size", "truncation_distance"):
        assert np.float32(h[k]) == np.float32(getattr(cfg, k))
    for k in ("voxels_per_side", "with_semantics", "with_tracking", "num_labels", "semantic_mode"):
        assert h[k] == getattr(cfg, k), k
    for i, b in enumerate(idx):
        want, got = ctx.download_block(b), ck.block_view(layers, i)
        for k in PUBLIC_LAYERS + ("likelihoods",):
            assert got[k].tobytes() == want[k].tobytes(), (k, b)
        assert got["block_flags"] == want["block_flags"]
    assert not (layers["flags"] & 0xF0).any(), "internal voxel flag bits in the stream"
    # saving the restored map gives the same bytes; so does a save into page-locked memory, and a load out of it
    assert fresh.save_map() == blob
    pin = PinnedArray(np.zeros(len(blob), np.uint8))
    try:
        view = np.ctypeslib.as_array(C.cast(pin.ptr, C.POINTER(C.c_uint8)), shape=(len(blob),))
        assert ctx.save_map(out=view) == len(blob)
        assert view.tobytes() == blob
        third = FusionContext(clone_cfg(cfg))
        rc, kept = third.load_map_rc(None, ptr=pin.data_ptr(), nbytes=len(blob))
        assert rc == 0 and kept == nblocks
        assert digests_equal(third.map_digest(), ctx.map_digest())
        third.close()
    finally:
        pin.free()
    fresh.close()


@pytest.mark.gpu
def test_import_from_the_oracle(saved):
    """the restore path without the save path: the stream is built by the codec from the oracle's blocks"""
    cfg, ctx, ora, blob = saved
    built = ck.pack_blocks(cfg, ora.block_indices(), ora.get_block)
    fresh = FusionContext(clone_cfg(cfg))
    assert fresh.load_map(built) == ora.num_blocks()
    assert digests_equal(fresh.map_digest(), ora.map_digest())
    assert np.array_equal(fresh.block_indices(), ora.block_indices())
    assert built == blob, "the device-written stream and the codec's stream of the oracle's blocks differ"
    fresh.close()


CONT = dict(voxel_size=0.05, truncation_distance=0.15, temporal_window=0.6, stream_kw=dict(period=5.0))


@pytest.mark.gpu
def test_continuation_against_the_oracle():
    """Save after 30 frames, load into a fresh context, feed frames 30..59 to it and to the oracle, which never stopped.  The
    stream (5 cm voxels, a 5 s camera circle) was checked with the oracle on the CPU to meet the conditions asserted below."""
    cfg, ctx, ora, s, sen, osen = make_pair(**CONT)
    for i in range(30):
        step_both(ctx, ora, sen, osen, s.render(i), motion=True, track=True)
        if i % 5 == 4:
            assert np.array_equal(np.asarray(ctx.reset_inactive()), np.asarray(ora.reset_inactive()))
    blob = ctx.save_map()
    h, idx, layers = ck.unpack(blob)
    assert len(idx) > 100, "the saved map must hold more than 100 blocks"
    assert (layers["flags"] & 2).any() and (layers["flags"] & 1).any() and (layers["distance"] < 0).any()
    res = FusionContext(clone_cfg(cfg))
    assert res.load_map(blob) == len(idx)
    assert digests_equal(res.map_digest(), ora.map_digest())
    ctx.close()
    archived_after, seed_frames = 0, 0
    for i in range(30, 60):
        out = step_both(res, ora, sen, osen, s.render(i), motion=True, track=True)
        assert digests_equal(res.map_digest(), ora.map_digest()), ("digest", i)
        st = res.stats()
        assert st["n_updated_voxels"] == out["ostats"]["n_updated_voxels"], ("n_updated_voxels", i)
        assert st["n_band_voxels"] == out["ostats"]["n_band_voxels"], ("n_band_voxels", i)
        assert st["n_allocated_blocks"] == ora.num_blocks(), ("n_allocated_blocks", i)
        assert out["n_gpu"] == out["n_ora"], ("clusters", i)
        assert np.array_equal(out["dyn_gpu"], out["dyn_ora"]), ("dynamic image", i)
        seed_frames += 1 if out["seeds_ora"] > 0 else 0
        if i % 5 == 4:
            res.generate_mesh(only_mesh_updated=False, clear_flag=True)
            ora.generate_mesh(False, True)
            gm, om = res.download_mesh(), ora.mesh()
            for k in ("points", "colors", "labels", "stamps"):
                print("mesh", i, k, gm[k].shape, om[k].shape, "equal" if gm[k].tobytes() == om[k].tobytes() else "DIFFERENT")
            for k in ("points", "colors", "labels", "stamps"):
                assert gm[k].shape == om[k].shape and gm[k].tobytes() == om[k].tobytes(), ("mesh", i, k)
            rg, ro = np.asarray(res.reset_inactive()), np.asarray(ora.reset_inactive())
            assert np.array_equal(rg, ro), ("archived blocks", i)
            archived_after += len(rg)
            assert digests_equal(res.map_digest(), ora.map_digest()), ("digest after archival", i)
    assert archived_after > 0, "no block was archived after the restore"
    assert seed_frames > 0, "no frame after the restore had motion seeds"
    res.close()


@pytest.mark.gpu
def test_different_layout(saved):
    cfg, ctx, ora, blob = saved
    want = ctx.map_digest()
    n = ctx.num_blocks()
    # another pool size (>= the block count), and the other likelihood row form
    for kw in (dict(max_blocks=n), dict(max_blocks=1500), dict(packed_likelihood_rows=1)):
        c = FusionContext(clone_cfg(cfg, **kw))
        assert c.load_map(blob) == n
        assert digests_equal(c.map_digest(), want), kw
        if kw.get("packed_likelihood_rows"):
            # ... and the reverse: saved with packed rows, loaded with padded ones
            again = c.save_map()
            assert again == blob
            d = FusionContext(clone_cfg(cfg, packed_likelihood_rows=0))
            assert d.load_map(again) == n and digests_equal(d.map_digest(), want)
            d.close()
        c.close()


@pytest.mark.gpu
def test_8vps_round_trip():
    cfg, ctx, ora, removed = run_stream(n_frames=12, archive_every=0, voxels_per_side=8, voxel_size=0.05, truncation_distance=0.15,
                                        max_blocks=16384)
    blob = ctx.save_map()
    assert ck.unpack(blob)[0]["voxels_per_side"] == 8
    c = FusionContext(clone_cfg(cfg, max_blocks=8192))
    assert c.load_map(blob) == ctx.num_blocks() > 0
    assert digests_equal(c.map_digest(), ctx.map_digest()) and digests_equal(c.map_digest(), ora.map_digest())
    assert c.save_map() == blob
    c.close()
    ctx.close()


def owner_of(idx, world):
    """khr_device.h: ownerOf"""
    def mix(h):
        h = h & 0xFFFFFFFF
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    x, y, z = (int(v) & 0xFFFFFFFF for v in idx)
    h = mix(((x * 73856093) & 0xFFFFFFFF) ^ mix(((y * 19349663) & 0xFFFFFFFF) ^ mix((z * 83492791) & 0xFFFFFFFF)))
    return (h * world) >> 32


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_reshard(saved, world):
    cfg, ctx, ora, blob = saved
    want = ctx.map_digest()
    total = np.zeros(12, np.uint64)
    kept_sum = 0
    for rank in range(world):
        c = FusionContext(clone_cfg(cfg, rank=rank, world_size=world))
        kept = c.load_map(blob)
        idx = c.block_indices()
        assert len(idx) == kept == c.checkpoint_size()[1]
        assert all(owner_of(b, world) == rank for b in idx)
        with np.errstate(over="ignore"):
            total += c.map_digest()
        kept_sum += kept
        c.close()
    assert kept_sum == ctx.num_blocks()
    assert digests_equal(total, want), "the shards' digests must add up (mod 2^64) to the saved map's"


@pytest.mark.gpu
def test_errors(saved):
    cfg, ctx, ora, blob = saved
    want = ctx.map_digest()
    n = ctx.num_blocks()
    # a non-empty map refuses a load and keeps its contents
    rc, kept = ctx.load_map_rc(blob)
    assert rc == KHR_ESTATE and "empty" in last_error(ctx)
    assert digests_equal(ctx.map_digest(), want)
    # a buffer that is too small: KHR_ENOMEM, nothing written, the length reported
    small = np.full(len(blob) - 1, 0xAB, np.uint8)
    rc, need = ctx.save_map_into(small)
    assert rc == KHR_ENOMEM and need == len(blob) and (small == 0xAB).all()

    def check_recovers(c, expect_blocks=n):
        assert c.num_blocks() == 0 and int(c.map_digest()[10]) == 0
        if expect_blocks is not None:
            assert c.load_map(blob) == expect_blocks and digests_equal(c.map_digest(), want)

    # configuration mismatches: the text names the field
    for kw, field in ((dict(voxel_size=0.2), "voxel_size"), (dict(truncation_distance=0.4), "truncation_distance"),
                      (dict(with_tracking=0), "with_tracking"), (dict(num_labels=19), "num_labels"),
                      (dict(voxels_per_side=8), "voxels_per_side"), (dict(with_semantics=0), "with_semantics")):
        c = FusionContext(clone_cfg(cfg, **kw))
        rc, kept = c.load_map_rc(blob)
        assert rc == KHR_EINVAL and field in last_error(c), (kw, last_error(c))
        assert c.num_blocks() == 0
        c.close()
    c = FusionContext(clone_cfg(cfg))
    # more blocks than the pool holds
    tiny = FusionContext(clone_cfg(cfg, max_blocks=n - 1))
    rc, kept = tiny.load_map_rc(blob)
    assert rc == KHR_ENOMEM and "max_blocks" in last_error(tiny)
    check_recovers(tiny, expect_blocks=None)
    tiny.close()
    # the same block index twice, built with the codec
    h, idx, layers = ck.unpack(blob)
    dup_idx = idx.copy()
    dup_idx[len(idx) // 2] = dup_idx[len(idx) // 2 - 1]
    dup = ck.pack(h, dup_idx, layers, sort=False)
    rc, kept = c.load_map_rc(dup)
    assert rc == KHR_EINVAL and "duplicate" in last_error(c), last_error(c)
    check_recovers(c)
    # truncated buffer, bad magic, unknown version: refused before any device work
    c.reset_map(cfg.voxel_size, cfg.truncation_distance)
    for bad, word in ((blob[:-1], "truncated"), (blob[:200], "truncated"), (b"\x00" + blob[1:], "magic"),
                      (blob[:4] + b"\x09" + blob[5:], "version")):
        rc, kept = c.load_map_rc(bad)
        assert rc == KHR_EINVAL and word in last_error(c), (word, last_error(c))
    check_recovers(c)
    c.close()


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
def test_aw_demo_checkpoint(tmp_path):
    """hydra::VolumetricMap::save / load around the two calls, through a file"""
    cfgp = tmp_path / "aw_ckpt.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--checkpoint", str(cfgp), "320", "240", "16", str(tmp_path / "map.khrm")], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["blocks_saved"] == r["blocks_loaded"] > 0, r
    assert r["digest_saved"] == r["digest_loaded"] and len(r["digest_saved"]) == 12, r
    assert r["file_bytes"] == os.path.getsize(tmp_path / "map.khrm"), r
    assert r["save_ms"] > 0 and r["load_ms"] > 0, r
