"""Marching cubes on the hand-built maps of tests/mesh_cases.py: the device (k_mesh_prepare, k_marching_cubes count / emit, the copy
of the kept blocks, both mesh halos, k_mesh_gather) against the CPU oracle on the same voxel content, which reaches the device
through a checkpoint stream (FusionContext.load_map) and the oracle through OracleMap.put_blocks.  Every comparison is bit for bit.
tests/test_cpu_mesh_cases.py shows on the CPU that the maps reach what they are built to reach."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases as mc
from common import compact_mesh_halo_exchange, record_mesh_halo_exchange, tri_soup
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_ENOMEM
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
MESH_FIELDS = ("points", "colors", "labels", "stamps", "first_seen")


def make_cfg(vps, **kw):
    return default_config(voxels_per_side=vps, max_blocks=4096, max_frame_pixels=320 * 240, exact_arithmetic=1, **dict(mc.CONFIG, **kw))


def load_pair(vps, indices, layers, **kw):
    """the same blocks in a fresh context (through a checkpoint stream) and a fresh oracle (block by block)"""
    cfg = make_cfg(vps, **kw)
    ctx = FusionContext(cfg)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    ora = po.OracleMap(po.config_from(cfg, 0))
    ora.put_blocks(indices, layers)
    assert [hex(int(x)) for x in ctx.map_digest()] == [hex(int(x)) for x in ora.map_digest()]
    return cfg, ctx, ora


def assert_same_mesh(ctx, ora, what=""):
    """download_mesh == fetch_mesh == the oracle's mesh, array for array, byte for byte; the statistics agree"""
    gm, om, fm = ctx.download_mesh(), ora.mesh(), ctx.fetch_mesh()
    for k in MESH_FIELDS:
        assert gm[k].shape == om[k].shape, (what, k, gm[k].shape, om[k].shape)
        if gm[k].tobytes() != om[k].tobytes():
            bad = np.flatnonzero((gm[k] != om[k]).reshape(len(gm[k]), -1).any(axis=1))
            raise AssertionError((what, k, len(bad), "of", len(gm[k]), "first", bad[:4], gm[k][bad[:4]], om[k][bad[:4]]))
        assert fm[k].tobytes() == gm[k].tobytes(), (what, "fetch_mesh", k)
    assert ctx.stats()["n_mesh_vertices"] == len(om["points"]), what
    return om


def run_map(vps, indices, layers, **kw):
    cfg, ctx, ora = load_pair(vps, indices, layers, **kw)
    ctx.generate_mesh(False, False)
    ora.generate_mesh(False, False)
    m = assert_same_mesh(ctx, ora, kw)
    ctx.close()
    ora.close()
    return m


@pytest.mark.parametrize("vps", [16, 8])
def test_all_cases(vps):
    m = run_map(vps, *mc.all_cases(vps))
    assert len(m["points"]) > 0


@pytest.mark.parametrize("eps", [0.0, 1e-3])
@pytest.mark.parametrize("attr", [0, 1])
@pytest.mark.parametrize("vps", [16, 8])
def test_edges(vps, attr, eps):
    m = run_map(vps, *mc.edges(vps), mesh_attr_source=attr, mesh_degenerate_eps=eps)
    assert len(m["points"]) > 0


def test_relations():
    run_map(16, *mc.relations())


def test_shortcut():
    idx, layers, plan = mc.shortcut(with_plan=True)
    m = run_map(16, idx, layers)
    # (the per-block expectations -- zero vertices, single cubes -- are asserted on the oracle's mesh in test_cpu_mesh_cases.py)
    assert len(m["points"]) > 6


@pytest.mark.parametrize("vps", [16, 8])
def test_dense(vps):
    m = run_map(vps, *mc.dense(vps))
    assert len(m["points"]) == mc.dense_vertices(vps)


def test_partial():
    idx, layers, flagged = mc.partial(with_plan=True)
    cfg, ctx, ora = load_pair(16, idx, layers)
    ctx.generate_mesh(True, False)          # the flagged half alone, one of its blocks without a triangle
    ora.generate_mesh(True, False)
    part = assert_same_mesh(ctx, ora, "flagged half")
    ctx.generate_mesh(False, False)
    ora.generate_mesh(False, False)
    full = assert_same_mesh(ctx, ora, "all blocks")
    assert 0 < len(part["points"]) < len(full["points"])
    ctx.generate_mesh(True, True)           # the flagged half again, the other blocks' vertices carried over
    ora.generate_mesh(True, True)
    again = assert_same_mesh(ctx, ora, "flagged half regenerated, the rest kept")
    for k in MESH_FIELDS:
        assert again[k].tobytes() == full[k].tobytes(), k
    assert sorted(tuple(b) for b in ctx.block_indices().tolist()) == sorted(tuple(b) for b in idx.tolist())
    for b in idx:
        assert (ctx.download_block(b)["block_flags"] & mc.BLK_MESH_UPDATED) == 0
    ctx.generate_mesh(True, True)           # nothing is flagged now: every block's vertices are carried over
    assert_same_mesh(ctx, ora, "nothing to regenerate")
    ctx.close()
    ora.close()


def sharded(world, vps, indices, layers):
    cfg = make_cfg(vps)
    blob = ck.pack(cfg, indices, layers)
    shards = [FusionContext(make_cfg(vps, rank=r, world_size=world)) for r in range(world)]
    kept = [c.load_map(blob) for c in shards]
    assert sum(kept) == len(indices)
    ora = po.OracleMap(po.config_from(cfg, 0))
    ora.put_blocks(indices, layers)
    ora.generate_mesh(False, False)
    return shards, ora.mesh()


def assert_shards_equal_full(shards, full):
    parts = [c.download_mesh() for c in shards]
    uni = tri_soup({k: np.concatenate([p[k] for p in parts]) for k in parts[0]})
    want = tri_soup(full)
    assert uni[0].shape == want[0].shape and want[0].shape[0] > 100
    for a, b in zip(want, uni):
        assert a.tobytes() == b.tobytes()


def emitting_blocks(full, indices, vps):
    """blocks with a vertex strictly inside their own cubes' lattice: a vertex no other block's cube can have produced"""
    p = full["points"].astype(np.float64) / mc.VOXEL_SIZE - 0.5
    out = set()
    for b in indices.tolist():
        lo = np.array(b, np.float64) * vps + 0.01
        if ((p > lo) & (p < lo + vps - 1.02)).all(axis=1).any():
            out.add(tuple(b))
    return out


def assert_every_relation_remote(shards, full, indices, vps):
    have = {tuple(b) for b in indices.tolist()}
    emit = emitting_blocks(full, indices, vps)
    seen = set()
    for c in shards:
        own = {tuple(b) for b in c.block_indices().tolist()}
        for b in own & emit:
            for k in range(1, 8):
                nb = tuple(b[i] + mc.OFFSETS[k][i] for i in range(3))
                if nb in have and nb not in own:
                    seen.add(k)
    assert seen == set(range(1, 8)), seen


MAPS = {"relations": lambda: (16,) + mc.relations(), "all_cases16": lambda: (16,) + mc.all_cases(16), "all_cases8": lambda: (8,) + mc.all_cases(8)}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(MAPS))
def test_whole_record_halo(name, world):
    vps, idx, layers = MAPS[name]()
    shards, full = sharded(world, vps, idx, layers)
    assert record_mesh_halo_exchange(shards, only_mesh_updated=False) > 0
    for c in shards:
        c.generate_mesh(False, False)
    assert_shards_equal_full(shards, full)
    if name == "relations":
        assert_every_relation_remote(shards, full, idx, vps)
    # without the halo a shard drops every cube that touches a remote neighbour
    n_with = [len(c.download_mesh()["points"]) for c in shards]
    for c in shards:
        c.mesh_halo_import(None)
        c.generate_mesh(False, False)
    assert sum(len(c.download_mesh()["points"]) for c in shards) < sum(n_with)
    for c in shards:
        c.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(MAPS))
def test_compact_halo(name, world):
    vps, idx, layers = MAPS[name]()
    shards, full = sharded(world, vps, idx, layers)
    headers, bufs = compact_mesh_halo_exchange(shards, only_mesh_updated=False)
    assert int(headers[:, 0].sum()) > 0
    if name == "relations":  # requests of every relation went out: header word 8 * peer + k counts those of relation k to that peer
        assert all(int(headers[:, k::8].sum()) > 0 for k in range(1, 8)), headers
    for c in shards:
        c.generate_mesh(False, False)
    assert_shards_equal_full(shards, full)
    if name == "relations":
        assert_every_relation_remote(shards, full, idx, vps)
    for c in shards:
        c.close()
    for d in [bufs[0]] + bufs[1] + bufs[2]:
        d.free()


def test_overflow_is_not_sticky():
    """a mesh that does not fit fails with KHR_ENOMEM and both numbers; the same context then meshes what fits, and the blocks it
    does not regenerate keep the vertices they had before the failed call"""
    vps = 8
    need = mc.dense_vertices(vps)
    idx, layers = mc.dense(vps, flagged=mc.DENSE_HALF)
    cfg, ctx, ora = load_pair(vps, idx, layers, max_mesh_vertices=need - 1)

    def digests():
        return [hex(int(x)) for x in ctx.map_digest()], [hex(int(x)) for x in ora.map_digest()]

    def assert_overflow():
        # the map -- block flags included, which only a successful clear_flag call changes, on both sides alike -- is the
        # oracle's before the failed call and after it
        before, want = digests()
        assert before == want
        ctx.generate_mesh(False, False)
        view = C.c_int64(0)
        for call in (lambda: ctx.lib.khr_mesh_num_vertices(ctx.h), lambda: ctx.lib.khr_fetch_mesh(ctx.h, C.byref(view))):
            assert call() == KHR_ENOMEM
            msg = ctx.lib.khr_last_error().decode()
            assert str(need) in msg and str(need - 1) in msg, msg
        assert digests() == (before, want)

    assert_overflow()                       # on the fresh context
    ctx.generate_mesh(True, True)           # the flagged half fits
    ora.generate_mesh(True, True)
    half = assert_same_mesh(ctx, ora, "flagged half after an overflow")
    assert len(half["points"]) == mc.dense_vertices(vps, mc.DENSE_HALF)
    assert_overflow()                       # again, now with a mesh to lose
    ctx.generate_mesh(True, False)          # no block is flagged any more: every vertex is carried over from before the failed call
    ora.generate_mesh(True, False)
    assert_same_mesh(ctx, ora, "kept blocks after an overflow")
    assert [hex(int(x)) for x in ctx.map_digest()] == [hex(int(x)) for x in ora.map_digest()]
    ctx.close()
    ora.close()
    # exactly enough room succeeds
    cfg, ctx, ora = load_pair(vps, idx, layers, max_mesh_vertices=need)
    ctx.generate_mesh(False, False)
    ora.generate_mesh(False, False)
    assert len(assert_same_mesh(ctx, ora, "max_mesh_vertices == need")["points"]) == need
    ctx.close()
    ora.close()
