"""-m "not gpu": the definition of khr_query_points (ASSUMPTIONS.md A.13) as tests/query_replica.py restates it, run over the CPU
oracle's blocks after the 320x240, 10 cm, 30-frame stream with archival every 5 frames.  Fixes the point sets the GPU test uses
(tests/query_cases.py) and proves on the replica alone that they are not vacuous; checks two properties of the replica itself."""
import os

import numpy as np
import pytest

import query_cases as qc
import query_replica as qr
import render_replica as rr
from khronos_amd import capi, default_config
from khronos_amd.synth import SyntheticStream
from oracle import pyoracle as po

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N_FRAMES = 320, 240, 30


@pytest.fixture(scope="module")
def world():
    """the oracle half of common.make_pair / step_both: motion detection, masked integration, tracking, archival every 5 frames"""
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, with_semantics=1, with_tracking=1, max_blocks=4096, max_frame_pixels=W * H,
                         md_min_cluster_size=20, md_min_separation_distance=2.0, md_max_range=5.0, temporal_window=0.6, exact_arithmetic=1)
    ora = po.OracleMap(po.config_from(cfg, 0))
    s = SyntheticStream(W, H, seed=1234)
    osen = ora.make_sensor(W, H, s.fx, s.fy, s.cx, s.cy)
    fr = dyn = None
    for i in range(N_FRAMES):
        fr = s.render(i)
        _, dyn, _ = ora.detect_motion(osen, fr["stamp"], fr["pose"], fr["depth"])
        ora.integrate(osen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"], mask=dyn)
        ora.update_tracking(fr["stamp"])
        if i % 5 == 4:
            ora.reset_inactive()
    blocks = qr.QueryBlocks(ora.block_indices(), ora.get_block, cfg.voxels_per_side)
    sets = qc.all_sets(blocks, fr, osen, cfg.voxel_size, cfg.truncation_distance, cfg.mesh_min_weight)
    res = {k: qr.query(blocks, p, cfg.voxel_size, cfg.mesh_min_weight) for k, p in sets.items()}
    return dict(cfg=cfg, blocks=blocks, frame=fr, dyn=np.asarray(dyn), sensor=osen, sets=sets, res=res)


def test_every_status_occurs_and_the_sets_are_not_vacuous(world):
    res, sets = world["res"], world["sets"]
    union = np.concatenate([res[k]["status"] for k in ("surface", "box", "lattice", "bad")])
    seen = sorted(set(int(v) for v in union))
    print("status values:", {v: int((union == v).sum()) for v in seen})
    # VALUE needs the voxel of tap 0 or of tap 7 allocated, and the point lies in one of the eight: VALUE implies VOXEL; GRADIENT
    # implies VALUE.  So A.13 can produce exactly these four
    assert seen == [0, qr.QP_VOXEL, qr.QP_VALUE | qr.QP_VOXEL, qr.QP_VALUE | qr.QP_GRADIENT | qr.QP_VOXEL], seen
    n = len(sets["surface"]) // 3
    at = res["surface"]["status"][:n]
    print("surface at offset 0: %d of %d with VALUE" % ((at & qr.QP_VALUE != 0).sum(), n))
    assert 2 * (at & qr.QP_VALUE != 0).sum() >= n
    assert len(sets["bad"]) >= 5 and not res["bad"]["status"].any()
    for k in qr.FIELDS:
        assert not res["bad"][k].any(), k
    assert np.array_equal(np.sort(sets["mixed"], axis=0), np.sort(np.concatenate([sets[k] for k in ("surface", "box", "lattice", "bad")]), axis=0),
                          equal_nan=True)


def test_outputs_of_a_clear_bit_are_zero(world):
    for name, r in world["res"].items():
        st = r["status"]
        assert not r["distance"][(st & qr.QP_VALUE) == 0].any(), name
        assert not r["gradient"][(st & qr.QP_GRADIENT) == 0].any(), name
        off = (st & qr.QP_VOXEL) == 0
        for k in ("weight", "color", "label", "flags", "last_observed"):
            assert not r[k][off].any(), (name, k)
        assert (r["n_value"], r["n_gradient"], r["n_voxel"]) == tuple(int(((st & b) != 0).sum()) for b in (1, 2, 4))
    r = world["res"]["surface"]
    assert r["label"].any() and r["last_observed"].any() and r["color"].any() and r["flags"].any()


def test_lattice_holds_each_named_case(world):
    cfg, blocks = world["cfg"], world["blocks"]
    v = cfg.voxels_per_side
    mw = f32(cfg.mesh_min_weight)
    vs_inv = f32(1) / f32(cfg.voxel_size)
    lat = qc.lattice_points(blocks, cfg.voxel_size, cfg.mesh_min_weight)
    a, b = qc.pick_blocks(blocks, cfg.mesh_min_weight)
    assert (a < 0).sum() >= 2 and (b >= 0).all()
    edge = (0, 1, v - 2, v - 1)

    def indices(p):
        ok, i0, f = qr.index_and_fraction(p, vs_inv)
        assert ok.all()
        return np.stack(i0, axis=1), np.stack(f, axis=1)

    def n_blocks(i0, lo, hi):
        """distinct blocks under the taps i0 + [lo, hi] per axis"""
        return np.prod([((i0[:, a] + hi) // v) - ((i0[:, a] + lo) // v) + 1 for a in range(3)], axis=0)

    # exact voxel centres
    i0, f = indices(lat["centres"])
    assert len(i0) >= 40 and not f.any()
    assert np.isin(i0 % v, edge).any(axis=1).sum() >= 12
    # local index 0, 1, vps-2, vps-1 on one, two, three axes; the eight taps of the distance straddle 2, 4, 8 blocks, the gradient
    # reaches into the previous block
    for name, axes in (("edge1", 1), ("edge2", 2), ("edge3", 3)):
        i0, f = indices(lat[name])
        on_edge = np.isin(i0 % v, edge)
        assert (on_edge.sum(axis=1) == axes).all(), name
        for l in edge:
            assert ((i0 % v == l).sum(axis=1) == axes).any(), (name, l)  # all `axes` edge axes at l
        assert (n_blocks(i0, 0, 1) == 2 ** axes).any(), name
        assert (((i0 % v == 0).sum(axis=1) == axes) & (n_blocks(i0, -1, 2) == 2 ** axes) & (n_blocks(i0, 0, 1) == 1)).any(), name
        assert (f > 0).all()
        for blk in (a, b):
            assert ((i0 // v == blk).all(axis=1)).any(), (name, blk)
    # the distance valid, a shifted sample in a block that is not allocated
    i0, f = indices(lat["cut"])
    assert len(i0) >= 1
    for k in range(len(i0)):
        taps = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)]) + i0[k]
        row, found, lin = blocks.lookup(taps[:, 0], taps[:, 1], taps[:, 2])
        assert found.all() and (blocks.weight[row, lin] >= mw).all()
        around = np.array([[(k2 if ax == a else o[ax - (ax > a)]) for ax in range(3)] for a in range(3) for k2 in (-1, 2)
                           for o in ((0, 0), (1, 0), (0, 1), (1, 1))]) + i0[k]
        assert len(set(map(tuple, around))) == 24
        assert not blocks.lookup(around[:, 0], around[:, 1], around[:, 2])[1].all()
    # inside an allocated block, an unobserved voxel among the taps
    i0, f = indices(lat["hole"])
    assert len(i0) >= 1
    for k in range(len(i0)):
        taps = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)]) + i0[k]
        assert len(set(map(tuple, taps // v))) == 1
        row, found, lin = blocks.lookup(taps[:, 0], taps[:, 1], taps[:, 2])
        assert found.all() and (blocks.weight[row, lin] < mw).any()
    r = qr.query(blocks, lat["cut"], cfg.voxel_size, cfg.mesh_min_weight)
    assert (r["status"] == (qr.QP_VALUE | qr.QP_VOXEL)).all()
    r = qr.query(blocks, lat["hole"], cfg.voxel_size, cfg.mesh_min_weight)
    assert (r["status"] == qr.QP_VOXEL).all()


def test_distance_at_a_voxel_centre_is_the_stored_distance(world):
    cfg, blocks = world["cfg"], world["blocks"]
    p = qc.lattice_points(blocks, cfg.voxel_size, cfg.mesh_min_weight)["centres"]
    r = qr.query(blocks, p, cfg.voxel_size, cfg.mesh_min_weight)
    full = r["status"] == (qr.QP_VALUE | qr.QP_GRADIENT | qr.QP_VOXEL)
    assert full.sum() >= 20, full.sum()
    _, i0, f = qr.index_and_fraction(p, f32(1) / f32(cfg.voxel_size))
    row, found, lin = blocks.lookup(*i0)
    stored = blocks.distance[row, lin]
    assert found[full].all() and stored[full].any()
    assert r["distance"][full].tobytes() == stored[full].tobytes()
    # the attribute voxel of a voxel centre is that voxel: observed, since it is tap 0
    assert r["weight"][full].tobytes() == blocks.weight[row, lin][full].tobytes()


def test_gradient_is_the_difference_of_two_distances_one_voxel_apart(world):
    """index-space definition against render_replica.sample: points whose g is exact (g = p * vs_inv - 0.5 without rounding, found
    by exact_point) and their partners at g - 1 and g + 1 on one axis have the same fractions, so
    gradient_a = (sample(g + e_a) - sample(g - e_a)) * (0.5 * vs_inv) bit for bit"""
    cfg, blocks = world["cfg"], world["blocks"]
    vs_inv = f32(1) / f32(cfg.voxel_size)
    mw = f32(cfg.mesh_min_weight)
    v = cfg.voxels_per_side
    rng = np.random.default_rng(11)
    a_blk, b_blk = qc.pick_blocks(blocks, cfg.mesh_min_weight)
    checked = 0
    for axis in range(3):
        trip = []
        for blk in (a_blk, b_blk):
            for _ in range(200):
                j = blk.astype(np.int64) * v + rng.integers(0, v, 3)
                g = [f32(float(j[a]) + float(rng.integers(0, 256)) / 256.0) for a in range(3)]
                mid = [qc.exact_point(ga, vs_inv) for ga in g]
                lo, hi = qc.exact_point(g[axis] - f32(1), vs_inv), qc.exact_point(g[axis] + f32(1), vs_inv)
                if lo is None or hi is None or any(m is None for m in mid):
                    continue
                pm, pp = list(mid), list(mid)
                pm[axis], pp[axis] = lo, hi
                trip.append((mid, pm, pp))
        assert len(trip) >= 50, (axis, len(trip))
        mid, pm, pp = (np.array([t[k] for t in trip], f32) for k in range(3))
        r = qr.query(blocks, mid, cfg.voxel_size, cfg.mesh_min_weight)
        vm, dm = rr.sample(blocks, [pm[:, a] for a in range(3)], vs_inv, mw)
        vp, dp = rr.sample(blocks, [pp[:, a] for a in range(3)], vs_inv, mw)
        has = (r["status"] & qr.QP_GRADIENT) != 0
        assert has.sum() >= 20 and (vm & vp)[has].all(), (axis, has.sum())
        want = ((dp - dm) * (f32(0.5) * vs_inv)).astype(f32)
        assert r["gradient"][has, axis].tobytes() == want[has].tobytes(), axis
        assert r["gradient"][has, axis].any()
        # and the distance itself is render_replica's sample at the point
        v0, d0 = rr.sample(blocks, [mid[:, a] for a in range(3)], vs_inv, mw)
        val = (r["status"] & qr.QP_VALUE) != 0
        assert np.array_equal(v0, val) and r["distance"][val].tobytes() == d0[val].tobytes()
        checked += int(has.sum())
    print("gradient cross-check on %d points" % checked)


def test_surface_medians_on_the_oracle(world):
    """the oracle-side form of the GPU test's replica-independent check: over the last frame's non-dynamic pixels the median
    distance is positive in front of the surface, negative behind it and below one voxel in magnitude on it"""
    cfg, res = world["cfg"], world["res"]["surface"]
    depth = world["frame"]["depth"]
    sel = np.flatnonzero((depth > 0).ravel())
    n = len(sel)
    static = world["dyn"].ravel()[sel] == 0
    med = []
    for k in range(3):
        st, d = res["status"][k * n:(k + 1) * n], res["distance"][k * n:(k + 1) * n]
        use = static & ((st & qr.QP_VALUE) != 0)
        assert use.sum() > 1000
        med.append(float(np.median(d[use])))
    print("median distance on / in front of / behind the surface: %.4f %.4f %.4f m (voxel %.2f m)" % (med[0], med[1], med[2], cfg.voxel_size))
    assert abs(med[0]) < cfg.voxel_size and med[1] > 0 and med[2] < 0


def test_binding_and_header():
    assert "khr_query_points" in capi.EXPORTS
    lib = capi.load_library()
    assert len(lib.khr_query_points.argtypes) == 14
    assert (capi.KHR_QP_VALUE, capi.KHR_QP_GRADIENT, capi.KHR_QP_VOXEL) == (qr.QP_VALUE, qr.QP_GRADIENT, qr.QP_VOXEL)
    assert [n for n, _, _ in capi.FusionContext.QUERY_FIELDS] == list(qr.FIELDS)
    text = open(os.path.join(ROOT, "include", "khronos_amd.h")).read()
    for word in ("khr_query_stats", "#define KHR_QP_VALUE 1", "#define KHR_QP_GRADIENT 2", "#define KHR_QP_VOXEL 4",
                 "int khr_query_points(khr_ctx* ctx, int64_t n, const float* points, float min_weight, int on_device"):
        assert word in text, word
