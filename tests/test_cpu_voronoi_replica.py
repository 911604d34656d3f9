"""-m "not gpu": the definition of khr_voronoi_field (ASSUMPTIONS.md A.20) as tests/voronoi_replica.py restates it.  The windowed
key passes are held to brute force, sites included; the stop rule of the line walk, the separation predicate and the basis rule are
checked on hand-picked inputs and on the corridors and posts of tests/voronoi_cases.py; the box the GPU test puts around the last
pose of the 30-frame stream is fixed here and proven not to be vacuous on the CPU oracle's map; hydra::VoronoiConfig reads the
reference's values."""
import os
import subprocess

import numpy as np
import pytest

import distance_cases as dc
import distance_replica as dr
import mesh_cases as mc
import query_replica as qr
import voronoi_cases as vc
import voronoi_replica as vr
from khronos_amd import capi, default_config
from khronos_amd.synth import SyntheticStream
from oracle import pyoracle as po

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "khronos_amd", "lib", "host_selftest")
W, H, N_FRAMES = 320, 240, 30
MODES = [(vr.L1, 4, 0.0), (vr.ANGLE, 1, 0.2), (vr.L1_THEN_ANGLE, 20, 0.2)]


def blocks_of(indices, layers, vps):
    n = {tuple(int(v) for v in b): i for i, b in enumerate(indices)}
    get = lambda idx: {k: layers[k][n[tuple(int(v) for v in idx)]] for k in ("distance", "weight", "color", "sem_label", "flags", "last_observed")}
    return qr.QueryBlocks(indices, get, vps)


def test_the_symbol_is_declared_and_bound():
    assert "khr_voronoi_field" in capi.EXPORTS and "khr_voronoi_field_into" in capi.EXPORTS
    lib = capi.load_library()
    assert len(lib.khr_voronoi_field.argtypes) == 3 and len(lib.khr_voronoi_field_into.argtypes) == 11
    assert [k for k, _, _, _ in capi.FusionContext.VOR_FIELDS] == list(vr.DENSE + vr.LIST)
    assert [k for k, _ in capi.KhrVoronoiStats._fields_] == list(vr.STATS)
    hdr = open(os.path.join(ROOT, "include", "khronos_amd.h")).read()
    for text in ("typedef struct khr_voronoi_request", "typedef struct khr_voronoi_stats", "#define KHR_VOR_L1 0", "#define KHR_VOR_ANGLE 1",
                 "#define KHR_VOR_L1_THEN_ANGLE 2", "#define KHR_VOR_MAX_BASIS 4",
                 "int khr_voronoi_field(khr_ctx* ctx, const khr_voronoi_request* request, khr_voronoi_stats* stats);",
                 "int khr_voronoi_field_into(khr_ctx* ctx, int on_device, float* distance, int32_t* d2, uint8_t* status, int32_t* site, uint8_t* basis,"):
        assert text in hdr, text
    assert (capi.KHR_VOR_L1, capi.KHR_VOR_ANGLE, capi.KHR_VOR_L1_THEN_ANGLE, capi.KHR_VOR_MAX_BASIS) == (vr.L1, vr.ANGLE, vr.L1_THEN_ANGLE, vr.MAX_BASIS)
    rq = capi.FusionContext.voronoi_request((0, 0, 0), (1, 1, 1))
    assert (rq.min_distance, rq.mode, rq.parent_l1_separation, rq.min_basis) == (0.0, vr.L1_THEN_ANGLE, 20, 2)
    assert f32(rq.parent_cos_angle_separation) == f32(0.2)


@pytest.mark.parametrize("shape,R,density", [((20, 20, 20), 3, 0.002), ((20, 20, 20), 40, 0.002), ((7, 19, 13), 2, 0.01), ((19, 5, 16), 6, 0.004),
                                             ((1, 18, 1), 4, 0.1), ((12, 12, 12), 5, 0.0), ((9, 7, 5), 3, 0.03), ((9, 7, 5), 40, 0.03)])
def test_the_windowed_keys_equal_brute_force_value_and_site(shape, R, density):
    ties = 0
    for seed in range(3):
        rng = np.random.default_rng((hash((shape, R)) & 0xFFFF) + seed)
        sites = rng.random(shape) < density
        if density > 0 and not sites.any():
            sites[tuple(s // 3 for s in shape)] = True
        (bv, bs), (wv, ws) = vr.brute(sites), vr.windowed(sites, R)
        near = bv <= R * R
        assert np.array_equal(bv, dr.brute(sites)) and np.array_equal(np.minimum(wv, dr.FAR), dr.windowed(sites, R))   # A.15's value
        assert np.array_equal(wv[near], bv[near]) and np.array_equal(ws[near], bs[near]), (shape, R, seed)
        assert (wv[~near] > R * R).all() and (wv <= vr.FAR).all()
        if density == 0:
            assert (wv == vr.FAR).all() and (ws == vr.NO_SITE).all()
            continue
        # the cells in range with more than one minimiser: the tie-break is exercised
        s, c = np.argwhere(sites), np.argwhere(np.ones(shape, bool))
        d = ((c[:, None, :] - s[None, :, :]) ** 2).sum(axis=2)
        ties += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1)[near.ravel()].sum())
        # every site is a cell of the set, at the stated distance
        z, y, x = np.nonzero(near)
        l = bs[near]
        sx, sy, sz = l % shape[2], (l // shape[2]) % shape[1], l // (shape[2] * shape[1])
        assert sites[sz, sy, sx].all() and np.array_equal((x - sx) ** 2 + (y - sy) ** 2 + (z - sz) ** 2, bv[near])
    print("shape %s R %d: %d tied cells in range" % (shape, R, ties))
    if density > 0:
        assert ties > 0


def test_the_line_walk_stops_only_beyond_the_best_value():
    """the pitfall of dfWindowMin's stop rule: on this line cell 4 first finds (3 + 1, site 50) at k = 1; the site at k = 2 has
    k^2 == 4, ties the value and carries the smaller index"""
    keys = [vr.FAR_KEY] * 9
    keys[5] = (3 << 32) | 50
    keys[2] = (0 << 32) | 2
    strict, loose = vr.line_walk(keys, 8, True), vr.line_walk(keys, 8, False)
    assert (strict[4] >> 32, strict[4] & vr.NO_SITE) == (4, 2)
    assert (loose[4] >> 32, loose[4] & vr.NO_SITE) == (4, 50)
    exhaustive = [min(keys[j] + (((i - j) ** 2) << 32) for j in range(9)) for i in range(9)]
    assert strict == [vr.FAR_KEY if (k >> 32) >= vr.FAR else k for k in exhaustive]
    assert [k >> 32 for k in loose] == [k >> 32 for k in strict]   # the values agree: only the site is at stake
    # and on random lines the strict walk is the exhaustive window
    rng = np.random.default_rng(5)
    for _ in range(20):
        n, R = int(rng.integers(1, 24)), int(rng.integers(0, 9))
        line = [int(rng.integers(0, 12)) << 32 | int(rng.integers(0, 99)) if rng.random() < 0.4 else vr.FAR_KEY for _ in range(n)]
        want = [min(line[j] + (((i - j) ** 2) << 32) for j in range(n) if abs(i - j) <= R) for i in range(n)]
        assert vr.line_walk(line, R, True) == [vr.FAR_KEY if (k >> 32) >= vr.FAR else k for k in want]


def test_the_separation_predicate_on_hand_picked_triples():
    c = (0, 0, 0)
    for mode in (vr.L1, vr.ANGLE, vr.L1_THEN_ANGLE):
        assert not vr.separated(c, (3, 4, 5), (3, 4, 5), mode, 1, 1.0)   # p == q: never, though cos = 1 admits the angle 0
    assert vr.separated(c, (3, 4, 5), (6, 8, 10), vr.ANGLE, 1, 1.0)     # the same direction, cos = 1: a.b == |a| |b|
    # a right angle: a.b = 0 <= 0 * |a| |b| counts as separated
    assert vr.separated(c, (1, 0, 0), (0, 1, 0), vr.ANGLE, 1, 0.0)
    assert not vr.separated(c, (2, 1, 0), (1, 2, 0), vr.ANGLE, 1, 0.0) and vr.separated(c, (2, -1, 0), (1, 2, 0), vr.ANGLE, 1, 0.0)
    assert not vr.separated(c, (1, 0, 0), (0, 1, 0), vr.L1, 3, 0.0) and vr.separated(c, (1, 0, 0), (0, 1, 0), vr.L1_THEN_ANGLE, 3, 0.0)
    # the L1 boundary: exactly parent_l1_separation is separated, one less is not
    assert vr.separated(c, (5, 1, 1), (1, 1, 1), vr.L1, 4, 0.0) and not vr.separated(c, (5, 1, 1), (1, 1, 1), vr.L1, 5, 0.0)
    assert vr.separated(c, (5, 1, 1), (2, 0, 1), vr.L1, 4, 0.0) and not vr.separated(c, (4, 1, 1), (2, 0, 1), vr.L1, 4, 0.0)
    # seen from elsewhere the same two sites subtend another angle
    assert vr.separated((3, 3, 0), (5, 3, 0), (1, 3, 0), vr.ANGLE, 1, 0.2) and not vr.separated((9, 3, 0), (5, 3, 0), (1, 3, 0), vr.ANGLE, 1, 0.2)


def field_of_case(case, mode, l1, cs, **kw):
    indices, layers, origin, dims, in_set = case
    blocks = blocks_of(indices, layers, vc.VPS)
    observed, obstacle = dr.classify(blocks, origin, dims, 1, mc.MESH_MIN_WEIGHT, 0.0)
    assert np.array_equal(obstacle, in_set) and observed.all()   # the map says what the construction means
    cell = f32(mc.VOXEL_SIZE)
    return vr.voronoi_field(blocks, mc.VOXEL_SIZE, origin, dims, 1, 100.0, mc.MESH_MIN_WEIGHT, min_distance=vc.MIN_DISTANCE_CELLS * float(cell), mode=mode,
                            parent_l1_separation=l1, parent_cos_angle_separation=cs, **kw)


@pytest.mark.parametrize("mode,l1,cs", MODES)
def test_corridors_list_their_middle_columns(mode, l1, cs):
    case = vc.corridor(vc.CORRIDOR_EVEN)
    out = field_of_case(case, mode, l1, cs)
    origin, dims = case[2], case[3]
    assert sorted(set((out["cells"][:, 0] - origin[0]).tolist())) == [6, 7] and len(out["cells"]) == 2 * dims[1] * dims[2]
    assert (out["basis"][:, :, [6, 7]] >= 2).all() and (np.delete(out["basis"], [6, 7], axis=2) <= 1).all()
    # (with an L1 separation of 4 two cells of the SAME wall two rows and two layers apart count as separated: basis 3 inside)
    assert (out["basis"][:, :, [6, 7]] == 2).all() or mode == vr.L1
    # the walls themselves and the columns beside them (nearer than min_distance) are not eligible, the others have their own site
    assert not out["basis"][:, :, [1, 2, 3, 10, 11, 12]].any() and (out["basis"][:, :, [0, 4, 5, 8, 9, 13]] == 1).all()
    # an even gap: column 6 is nearer to the wall at 2, column 7 to the wall at 11
    assert (out["site"][:, :, 6] % dims[0] == 2).all() and (out["site"][:, :, 7] % dims[0] == 11).all()
    case = vc.corridor(vc.CORRIDOR_ODD)
    out = field_of_case(case, mode, l1, cs)
    origin, dims = case[2], case[3]
    # an odd gap: column 7 is equidistant, its site is the wall at x = 2 (the least index); the diagram is two cells thick
    assert sorted(set((out["cells"][:, 0] - origin[0]).tolist())) == [7, 8]
    assert (out["site"][:, :, 7] % dims[0] == 2).all() and (out["d2"][:, :, 7] == 25).all() and (out["site"][:, :, 8] % dims[0] == 12).all()
    # the list is the ascending run of the cells with basis >= 2, with their sites on the two walls
    lin = np.flatnonzero(out["basis"].ravel() >= 2)
    local = out["cells"] - np.asarray(origin)
    assert np.array_equal(local[:, 0] + dims[0] * (local[:, 1] + dims[1] * local[:, 2]), lin)
    assert np.array_equal(out["cell_basis"], out["basis"].ravel()[lin]) and set((out["cell_sites"][:, :2, 0] - origin[0]).ravel().tolist()) == {2, 12}
    if mode != vr.L1:
        assert (out["cell_basis"] == 2).all() and not out["cell_sites"][:, 2:].any()


@pytest.mark.parametrize("mode,l1,cs", MODES)
def test_the_centre_of_four_posts_has_a_full_basis(mode, l1, cs):
    case = vc.posts()
    out = field_of_case(case, mode, l1, cs)
    x, y, z = vc.POSTS_CENTRE
    assert out["basis"][z, y, x] == 4 and out["d2"][z, y, x] == 32
    row = np.flatnonzero((out["cells"] - np.asarray(case[2]) == np.asarray(vc.POSTS_CENTRE)).all(axis=1))
    assert len(row) == 1
    got = {tuple(int(v) for v in s - np.asarray(case[2])) for s in out["cell_sites"][row[0]]}
    assert got == {(px, py, 3) for px, py in vc.POSTS}
    assert out["stats"]["n_basis4"] >= 1 and out["stats"]["n_basis2"] > 0
    # min_basis selects from the same field
    for mb in (3, 4):
        sel = field_of_case(case, mode, l1, cs, min_basis=mb)
        assert sel["basis"].tobytes() == out["basis"].tobytes() and sel["stats"]["n_listed"] == int((out["basis"] >= mb).sum()) > 0


@pytest.mark.parametrize("name,unk", [("wall", True), ("random", False)])
def test_the_two_forms_give_the_same_field_on_the_hand_built_maps(name, unk):
    """windowed and brute agree on every output where the range covers the box, and the field is not vacuous"""
    indices, layers = dc.CASES[name](8)
    blocks = blocks_of(indices, layers, 8)
    origin, _ = dc.box_of(name, 8, 2)
    cell = f32(mc.VOXEL_SIZE) * f32(2)
    a, b = (vr.voronoi_field(blocks, mc.VOXEL_SIZE, origin, (15, 9, 11), 2, 100.0, mc.MESH_MIN_WEIGHT, unknown_is_obstacle=unk, form=form,
                             min_distance=2 * float(cell), mode=vr.L1, parent_l1_separation=4) for form in ("windowed", "brute"))
    for k in vr.DENSE + vr.LIST:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"] == b["stats"] and a["stats"]["n_listed"] > 0, a["stats"]


@pytest.fixture(scope="module")
def world():
    """the oracle's map of the stream of tests/test_cpu_distance_field.py"""
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, with_semantics=1, with_tracking=1, max_blocks=4096, max_frame_pixels=W * H,
                         md_min_cluster_size=20, md_min_separation_distance=2.0, md_max_range=5.0, temporal_window=0.6, exact_arithmetic=1)
    ora = po.OracleMap(po.config_from(cfg, 0))
    s = SyntheticStream(W, H, seed=1234)
    osen = ora.make_sensor(W, H, s.fx, s.fy, s.cx, s.cy)
    fr = None
    for i in range(N_FRAMES):
        fr = s.render(i)
        _, dyn, _ = ora.detect_motion(osen, fr["stamp"], fr["pose"], fr["depth"])
        ora.integrate(osen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"], mask=dyn)
        ora.update_tracking(fr["stamp"])
        if i % 5 == 4:
            ora.reset_inactive()
    return dict(cfg=cfg, blocks=qr.QueryBlocks(ora.block_indices(), ora.get_block, cfg.voxels_per_side), frame=fr)


def test_the_stream_box_holds_voronoi_cells_of_every_basis(world):
    cfg = world["cfg"]
    origin, dims = dc.stream_box(world["frame"]["pose"], cfg.voxel_size)
    kw = dict(vc.STREAM)
    cell = f32(cfg.voxel_size) * f32(kw["ratio"])
    out = vr.voronoi_field(world["blocks"], cfg.voxel_size, origin, dims, kw.pop("ratio"), kw.pop("max_distance"), cfg.mesh_min_weight,
                           min_distance=vc.MIN_DISTANCE_CELLS * float(cell), **kw)
    st = out["stats"]
    print("stream box origin %s dims %s: %s" % (origin, dims, st))
    assert st["n_basis2"] > 0 and st["n_basis3"] + st["n_basis4"] > 0 and st["n_listed"] > 0
    assert st["n_listed"] == st["n_basis2"] + st["n_basis3"] + st["n_basis4"] <= st["n_eligible"] < st["n_in_range"]


def test_voronoi_config_reads_the_reference_values():
    out = subprocess.run([SELFTEST, "--voronoi-config"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(kv.split("=") for kv in out.stdout.split())
    assert got["mode"] == str(vr.L1_THEN_ANGLE) and f32(float(got["min_distance_m"])) == f32(0.30), got
    assert got["parent_l1_separation"] == "20" and f32(float(got["parent_cos_angle_separation"])) == f32(0.2), got
    assert got["min_basis"] == str(min(4, max(2, int(got["min_basis_for_extraction"]) + 1))), got
    assert got["modes"] == "0,1,2" and got["clamped"] == "2,4", got
