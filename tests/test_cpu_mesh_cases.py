"""-m "not gpu": the hand-built marching-cubes maps of tests/mesh_cases.py, with the CPU oracle alone.  Checks that OracleMap.put_block
hands back exactly what went in, and that every map meets the conditions tests/test_gpu_mesh_cases.py relies on: the maps must not
be vacuous (every configuration, every planted kind and every block relation is really reached)."""
import numpy as np
import pytest

import mesh_cases as mc
from common import np_map_digest
from khronos_amd import checkpoint as ck, default_config
from oracle import pyoracle as po

LAYERS = ("distance", "weight", "color", "last_observed", "last_occupied", "flags", "sem_label", "block_flags", "likelihoods")


def make_oracle(vps, **kw):
    cfg = default_config(voxels_per_side=vps, max_blocks=256, exact_arithmetic=1, **dict(mc.CONFIG, **kw))
    return cfg, po.OracleMap(po.config_from(cfg, 0))


def oracle_mesh(vps, indices, layers, only_updated=False, **kw):
    cfg, ora = make_oracle(vps, **kw)
    ora.put_blocks(indices, layers)
    ora.generate_mesh(only_updated, False)
    m = ora.mesh()
    ora.close()
    return m


def lattice(g, points):
    """world positions -> the box's voxel-centre coordinates (voxel (x, y, z)'s centre = (x, y, z))"""
    return np.asarray(points, np.float64) / mc.VOXEL_SIZE - 0.5 - np.asarray(g.origin, np.float64) * g.vps


def near(points_lattice, site, tol=1e-3):
    return int((np.abs(points_lattice - np.asarray(site, np.float64)).max(axis=1) <= tol).sum())


@pytest.mark.parametrize("vps", [16, 8])
def test_put_block_round_trip(vps):
    """put_block -> get_block -> pack_blocks -> unpack gives back every layer byte for byte, and the oracle's map digest equals the
    numpy restatement over the same blocks"""
    idx, layers = mc.edges(vps)
    rng = np.random.default_rng(5)
    layers = dict(layers)  # every flag combination and non-zero likelihoods, which the meshing maps do not need
    layers["flags"] = rng.integers(0, 16, layers["flags"].shape).astype(np.uint8)
    layers["block_flags"] = rng.integers(0, 16, len(idx)).astype(np.uint8)
    lik = rng.standard_normal(layers["likelihoods"].shape).astype(np.float32)
    layers["likelihoods"] = np.where((layers["flags"] & 8)[..., None] != 0, lik, np.float32(0))  # (the format: zeros without SEM_VALID)
    cfg, ora = make_oracle(vps)
    order = rng.permutation(len(idx))
    for i in order:                       # any order; blocks are allocated as they come
        ora.put_block(idx[i], ck.block_view(layers, i))
    assert ora.num_blocks() == len(idx)
    blob = ck.pack_blocks(cfg, ora.block_indices(), ora.get_block)
    assert blob == ck.pack(cfg, idx, layers)
    h, idx2, layers2 = ck.unpack(blob)
    srt = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    assert np.array_equal(idx2, idx[srt])
    for k in LAYERS:
        assert layers2[k].tobytes() == np.ascontiguousarray(layers[k][srt]).tobytes(), k
    want = np_map_digest((b, ora.get_block(b)) for b in ora.block_indices())
    assert [hex(int(x)) for x in ora.map_digest()] == [hex(int(x)) for x in want]
    # a second put overwrites in place
    ora.put_block(idx[0], ck.block_view(layers, 1))
    assert ora.num_blocks() == len(idx) and ora.get_block(idx[0])["distance"].tobytes() == layers["distance"][1].tobytes()
    ora.close()


@pytest.mark.parametrize("vps", [16, 8])
def test_all_cases_reaches_every_configuration(vps):
    idx, layers = mc.all_cases(vps)
    assert len(idx) == 8 and idx.min(axis=0).tolist() == list(mc.ORIGIN)
    c, v = mc.cube_configs(idx, layers, vps)
    assert int(v.sum()) == (2 * vps - 1) ** 3
    hist = np.bincount(c[v], minlength=256)
    print("all_cases vps %d: %d valid cubes, per configuration %d .. %d (mean %.1f)" % (vps, v.sum(), hist.min(), hist.max(), hist.mean()))
    assert (hist > 0).all(), np.flatnonzero(hist == 0)
    mag = np.abs(layers["distance"])
    assert mag.min() >= np.float32(0.05 * mc.TRUNCATION) * np.float32(0.999) and mag.max() <= np.float32(mc.TRUNCATION)
    assert len(oracle_mesh(vps, idx, layers)["points"]) > 0


@pytest.mark.parametrize("vps", [16, 8])
def test_dense_has_the_analytic_count(vps):
    idx, layers = mc.dense(vps)
    c, v = mc.cube_configs(idx, layers, vps)
    assert set(np.unique(c[v]).tolist()) == {0x5A, 0xA5}
    assert mc.dense_vertices(vps) == 12 * int(v.sum()) == 12 * (2 * vps - 1) ** 3
    m = oracle_mesh(vps, idx, layers)
    assert len(m["points"]) == mc.dense_vertices(vps), "the triangle table gives another count for configurations 0x5A / 0xA5"
    # the flagged half alone: the cubes of those four blocks
    idx, layers = mc.dense(vps, flagged=mc.DENSE_HALF)
    m = oracle_mesh(vps, idx, layers, only_updated=True)
    assert 0 < len(m["points"]) == mc.dense_vertices(vps, mc.DENSE_HALF) < mc.dense_vertices(vps) - 1


@pytest.mark.parametrize("vps", [16, 8])
def test_edges_kinds_are_reached(vps):
    idx, layers, plan, g = mc.edges(vps, with_plan=True)
    for kind, sites in plan.items():   # inside blocks and across each of the three faces
        if kind.startswith("eps"):
            continue
        cells = [s if np.ndim(s[0]) == 0 else s[0] for s in sites]
        for axis in range(3):
            on_face = [s for s in cells if s[axis] in (vps - 1, vps)]
            assert len(on_face) >= 6, (kind, axis)
        assert any(all(c not in (vps - 1, vps) for c in s) for s in cells), kind
    base = oracle_mesh(vps, idx, layers)
    p = lattice(g, base["points"])
    # zeros of either sign: a vertex exactly on the voxel centre (t = 0, or 1 from the other end)
    for kind in ("zero", "neg_zero"):
        hits = sum(1 for s in plan[kind] if near(p, s, 1e-2) > 0)
        print(vps, kind, "sites with a vertex on the voxel centre:", hits, "of", len(plan[kind]))
        assert hits >= len(plan[kind]) // 2, (kind, hits)
    assert np.signbit(layers["distance"][layers["distance"] == 0]).sum() == len(plan["neg_zero"])
    # degenerate pairs (|d0 - d1| < 1e-6, natural t = 3 / 7 or 4 / 7): the vertex sits half way
    mid = lambda s: (np.asarray(s[0], np.float64) + np.asarray(s[1], np.float64)) / 2
    hits = sum(1 for s in plan["tiny"] if near(p, mid(s), 1e-2) > 0)
    print(vps, "tiny pairs with a vertex half way:", hits, "of", len(plan["tiny"]))
    assert hits >= len(plan["tiny"]) // 2
    # t == 0.5 exactly: the two attribute rules pick different voxels there (and at the degenerate pairs), and nowhere else
    hits = sum(1 for s in plan["half"] if near(p, mid(s), 1e-2) > 0)
    assert hits >= len(plan["half"]) // 2
    other = oracle_mesh(vps, idx, layers, mesh_attr_source=1)
    assert other["points"].tobytes() == base["points"].tobytes()
    diff = np.flatnonzero((other["colors"] != base["colors"]).any(axis=1))
    assert len(diff) > 0 and (other["labels"][diff] != base["labels"][diff]).all() and (other["stamps"][diff] != base["stamps"][diff]).all()
    # ... from the lower voxel of the edge (rule 0, where it is the table edge's first endpoint) to the upper one (rule 1), with the
    # negative distance at either end; every such vertex sits on an edge whose t is 0.5 (planted, or two planted sites side by side)
    signs, f32 = set(), np.float32
    for i in diff:
        lo, up = np.array(_voxel_of(g, base["labels"][i])), np.array(_voxel_of(g, other["labels"][i]))
        assert sorted((up - lo).tolist()) == [0, 0, 1], (lo, up)
        d0, d1 = g.d[tuple(lo)], g.d[tuple(up)]
        assert (d0 < 0) != (d1 < 0)
        assert abs(f32(d0 - d1)) < f32(1e-6) or f32(d0 / f32(d0 - d1)) == f32(0.5) or f32(d1 / f32(d1 - d0)) == f32(0.5), (d0, d1)
        signs.add(bool(d0 < 0))
    assert signs == {True, False}
    # mesh_degenerate_eps = 1e-3: the pairs below it move half way, the pairs at and above it stay
    wide = oracle_mesh(vps, idx, layers, mesh_degenerate_eps=1e-3)
    assert wide["points"].shape == base["points"].shape and wide["points"].tobytes() != base["points"].tobytes()
    pw = lattice(g, wide["points"])
    moved = np.flatnonzero((wide["points"] != base["points"]).any(axis=1))
    assert len(moved) > 0
    hits = sum(1 for s in plan["eps_below"] if near(pw, mid(s), 1e-2) > 0 and near(p, mid(s), 1e-2) == 0)
    assert hits >= len(plan["eps_below"]) // 2, hits
    kept = 0
    for s in plan["eps_above"] + plan["eps_equal"]:
        d0, d1 = np.float64(g.d[s[0]]), np.float64(g.d[s[1]])
        at = np.asarray(s[0], np.float64) + d0 / (d0 - d1) * (np.asarray(s[1], np.float64) - np.asarray(s[0], np.float64))
        assert near(pw, at, 1e-2) == near(p, at, 1e-2)
        kept += near(pw, at, 1e-2) > 0
    assert kept >= len(plan["eps_above"]) // 2
    # weights: a corner at exactly mesh_min_weight is observed, the float below it is not
    n_base = len(base["points"])
    for kind, to, grows in (("w_min", np.nextafter(mc.MESH_MIN_WEIGHT, np.float32(0)), False), ("w_below", mc.MESH_MIN_WEIGHT, True),
                            ("w_zero", mc.MESH_MIN_WEIGHT, True)):
        w = layers["weight"].copy()
        frm = {"w_min": mc.MESH_MIN_WEIGHT, "w_below": np.nextafter(mc.MESH_MIN_WEIGHT, np.float32(0)), "w_zero": np.float32(0)}[kind]
        assert int((w == frm).sum()) == len(plan[kind])
        w[w == frm] = to
        n = len(oracle_mesh(vps, idx, dict(layers, weight=w))["points"])
        print(vps, kind, "vertices", n_base, "->", n)
        assert (n > n_base) if grows else (n < n_base), (kind, n, n_base)


def _voxel_of(g, label):
    """the box voxel whose label this is (labels are 1 + the voxel's running number in [x, y, z] order)"""
    return np.unravel_index(int(label) - 1, g.d.shape)


def test_relations_every_copy_and_every_owner():
    idx, layers, plan = mc.relations(with_plan=True)
    assert len(idx) == 7 * 7 + 8 <= 64
    have = {tuple(b) for b in idx.tolist()}
    origins = [g.origin for g, _ in plan]
    for a in range(8):
        for b in range(a + 1, 8):
            assert max(abs(origins[a][i] - origins[b][i]) for i in range(3)) > 3, "copies must not touch"
    m = oracle_mesh(16, idx, layers)
    for k, (g, missing) in enumerate(plan):
        p = lattice(g, m["points"])
        mine = ((p >= -0.5) & (p <= 2 * g.vps - 0.5)).all(axis=1)
        assert mine.sum() > 0
        if missing is None:
            continue
        assert tuple(g.origin[i] + missing[i] for i in range(3)) not in have
        # every cube that holds a lattice edge strictly inside this box touches the missing block (mesh_cases.py: relations)
        # (0.01 of a voxel inside it: float32 positions this far from the origin resolve 0.003 of a voxel)
        lo = np.array([c * g.vps - 1 for c in missing], np.float64) + 0.01
        hi = np.array([(c + 1) * g.vps for c in missing], np.float64) - 0.01
        inside = ((p > lo) & (p < hi)).all(axis=1)
        assert inside.sum() == 0, (k, int(inside.sum()))
        assert (mine & ~inside).sum() > 0
        # ... and the same box of the complete copy is not empty: the absence above is the missing block's doing
        pc = lattice(plan[0][0], m["points"])
        assert ((pc > lo) & (pc < hi)).all(axis=1).sum() > 0
    # the complete copy: every relation is remote for some block, for two and for three ranks
    g = plan[0][0]
    blocks = [tuple(g.origin[i] + o[i] for i in range(3)) for o in mc.OFFSETS]
    for world in (2, 3):
        for k in range(1, 8):
            remote = [b for b in blocks if tuple(b[i] + mc.OFFSETS[k][i] for i in range(3)) in blocks
                      and mc.owner_of(tuple(b[i] + mc.OFFSETS[k][i] for i in range(3)), world) != mc.owner_of(b, world)]
            assert remote, (world, k)


def test_shortcut_blocks():
    idx, layers, plan = mc.shortcut(with_plan=True)
    m = oracle_mesh(16, idx, layers)
    total = 0
    for name, (g, expect) in plan.items():
        p = lattice(g, m["points"])
        mine = ((p >= -0.5) & (p <= np.array(g.d.shape) - 0.5)).all(axis=1)
        print("shortcut", name, int(mine.sum()))
        total += int(mine.sum())
        if expect is not None:
            assert mine.sum() == expect, name
    assert total == len(m["points"])
    v = 16
    # the all-positive first block: its own distances hold no negative, and every vertex comes from its outermost cubes
    g = plan["positive_first"][0]
    assert (g.d[g.block_slices((0, 0, 0))] > 0).all()
    p = lattice(g, m["points"])
    p = p[((p >= -0.5) & (p <= 2 * v - 0.5)).all(axis=1)]
    assert len(p) > 0 and ((p >= v - 1) & (p <= v)).any(axis=1).all() and (p <= v).all()
    # the mirror image: the cubes that cross belong to the seven negative blocks and read the positive one
    g = plan["positive_last"][0]
    p = lattice(g, m["points"])
    p = p[((p >= -0.5) & (p <= 2 * v - 0.5)).all(axis=1)]
    assert len(p) > 0 and (p >= v - 1).all()
    assert (layers["distance"][[tuple(b) == (100, 100, 100) for b in idx.tolist()]][0] < 0).nonzero()[0].tolist() == [0]
    assert (layers["distance"][[tuple(b) == (-100, -100, -100) for b in idx.tolist()]][0] < 0).nonzero()[0].tolist() == [v ** 3 - 1]


def test_partial_flags_half_and_an_empty_block():
    idx, layers, flagged = mc.partial(with_plan=True)
    full, _ = mc.all_cases(16)
    assert len(idx) == 9 and len(flagged) == 5
    fl = {tuple(b): int(f) for b, f in zip(idx.tolist(), layers["block_flags"])}
    assert sorted(b for b, f in fl.items() if f & mc.BLK_MESH_UPDATED) == sorted(flagged)
    part = oracle_mesh(16, idx, layers, only_updated=True)
    whole = oracle_mesh(16, idx, layers)
    assert 0 < len(part["points"]) < len(whole["points"])
    # the ninth block adds nothing: the whole mesh is all_cases' mesh
    assert whole["points"].tobytes() == oracle_mesh(16, full, mc.all_cases(16)[1])["points"].tobytes()
