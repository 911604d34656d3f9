"""-m "not gpu": the definition of khr_distance_field (ASSUMPTIONS.md A.15) as tests/distance_replica.py restates it.  The windowed
separable form is held to brute force; the hand-built maps of tests/distance_cases.py are checked against what their construction
says; the box the GPU test puts around the last pose of the 30-frame stream is fixed here and proven not to be vacuous on the CPU
oracle's map; hydra::DistanceFieldConfig reads the reference's mapper file."""
import os
import subprocess

import numpy as np
import pytest

import distance_cases as dc
import distance_replica as dr
import mesh_cases as mc
import query_replica as qr
from khronos_amd import capi, default_config
from khronos_amd.synth import SyntheticStream
from oracle import pyoracle as po

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "khronos_amd", "lib", "host_selftest")
W, H, N_FRAMES = 320, 240, 30
@pytest.fixture(autouse=True)
def the_feature_exists():
    """the replica restates a call of the library: without the call there is nothing it defines"""
    assert "khr_distance_field" in capi.EXPORTS and hasattr(capi.FusionContext, "distance_field")


def blocks_of(indices, layers, vps):
    n = {tuple(int(v) for v in b): i for i, b in enumerate(indices)}
    get = lambda idx: {k: layers[k][n[tuple(int(v) for v in idx)]] for k in ("distance", "weight", "color", "sem_label", "flags", "last_observed")}
    return qr.QueryBlocks(indices, get, vps)


def test_the_symbol_is_declared_and_bound():
    assert "khr_distance_field" in capi.EXPORTS
    lib = capi.load_library()
    assert len(lib.khr_distance_field.argtypes) == 7
    assert [k for k, _ in capi.FusionContext.DF_FIELDS] == list(dr.FIELDS)
    hdr = open(os.path.join(ROOT, "include", "khronos_amd.h")).read()
    for text in ("typedef struct khr_df_request", "typedef struct khr_df_stats", "#define KHR_DF_MAX_DIM 512", "#define KHR_DF_FAR (1 << 30)",
                 "int khr_distance_field(khr_ctx* ctx, const khr_df_request* request, int on_device, float* distance, int32_t* d2, uint8_t* status"):
        assert text in hdr, text
    assert capi.KHR_DF_FAR == dr.FAR and (capi.KHR_DF_OBSERVED, capi.KHR_DF_OBSTACLE, capi.KHR_DF_IN_RANGE) == (1, 2, 4)


@pytest.mark.parametrize("shape,R,density", [((20, 20, 20), 3, 0.002), ((20, 20, 20), 40, 0.002), ((7, 19, 13), 2, 0.01), ((19, 5, 16), 6, 0.004),
                                             ((1, 18, 1), 4, 0.1), ((12, 12, 12), 5, 0.0)])
def test_the_windowed_form_equals_brute_force(shape, R, density):
    rng = np.random.default_rng(hash((shape, R)) & 0xFFFF)
    sites = rng.random(shape) < density
    if density > 0 and not sites.any():
        sites[tuple(s // 3 for s in shape)] = True
    b, w = dr.brute(sites), dr.windowed(sites, R)
    near = b <= R * R
    print("shape %s R %d: %d sites, %d of %d cells in range" % (shape, R, sites.sum(), near.sum(), sites.size))
    assert np.array_equal(w[near], b[near])
    assert (w[~near] > R * R).all() and (w <= dr.FAR).all()
    if density > 0 and R < 10:
        assert near.any() and not near.all()   # R small enough that some cells are out of range, large enough that some are in
    if density == 0:
        assert (w == dr.FAR).all()


@pytest.mark.parametrize("vps", [16, 8])
def test_wall_matches_its_construction(vps):
    indices, layers, g = dc.wall(vps, with_group=True)
    blocks = blocks_of(indices, layers, vps)
    first = dc.group_first_cell(dc.WALL_ORIGIN, vps, 1)
    s, t = dc.wall_start(vps), dc.WALL_THICKNESS
    # a box inside the group's y and z extent that spans it along x, range beyond the box
    origin, dims = (first[0], first[1] + 2, first[2] + 1), (3 * vps, 2 * vps, vps)
    out = dr.distance_field(blocks, mc.VOXEL_SIZE, origin, dims, 1, max_distance=100.0, min_weight=mc.MESH_MIN_WEIGHT)
    cell = f32(mc.VOXEL_SIZE)
    col = np.arange(3 * vps)
    want = np.where(col < s, cell * (s - col).astype(f32), np.where(col < s + t, -cell * (col - (s - 1)).astype(f32), cell * (col - (s + t - 1)).astype(f32)))
    assert (out["distance"] == want.astype(f32)[None, None, :]).all()
    assert (out["d2"][0, 0, :s] == (s - col[:s]) ** 2).all() and (out["d2"][0, 0, s:s + t] == -((col[s:s + t] - s + 1) ** 2)).all()
    st = out["status"][0, 0]
    assert (st[:s] == 5).all() and (st[s:s + t] == 7).all() and (st[s + t:] == 4).all()   # free / obstacle / unknown, all in range
    n = dims[1] * dims[2]
    assert out["stats"] == {"n_observed": n * (s + t), "n_obstacle": n * t, "n_free": n * s, "n_in_range": n * 3 * vps}
    # behind the slab nothing is observed: with unknown_is_obstacle those cells join O (distance to free space through the slab) and
    # their status stays unobserved; with positive_only every cell of O is 0
    unk = dr.distance_field(blocks, mc.VOXEL_SIZE, origin, dims, 1, max_distance=100.0, min_weight=mc.MESH_MIN_WEIGHT, unknown_is_obstacle=True)
    assert (unk["d2"][0, 0, s:] == -((col[s:] - s + 1) ** 2)).all() and (unk["status"][0, 0, s + t:] == 4).all()
    assert np.array_equal(unk["d2"][:, :, :s], out["d2"][:, :, :s])
    pos = dr.distance_field(blocks, mc.VOXEL_SIZE, origin, dims, 1, max_distance=100.0, min_weight=mc.MESH_MIN_WEIGHT, unknown_is_obstacle=True,
                            positive_only=True)
    assert not pos["d2"][:, :, s:].any() and not pos["distance"][:, :, s:].any() and not np.signbit(pos["distance"]).any()
    assert np.array_equal(pos["d2"][:, :, :s], out["d2"][:, :, :s]) and (pos["status"] & 4 != 0).all()
    # a short range: the free columns further than 5 cells from the slab are out of range
    short = dr.distance_field(blocks, mc.VOXEL_SIZE, origin, dims, 1, max_distance=0.55, min_weight=mc.MESH_MIN_WEIGHT)
    far = col < s - 5
    assert (short["d2"][0, 0, far] == dr.FAR).all() and (short["distance"][0, 0, far] == f32(0.55)).all() and (short["status"][0, 0, far] == 1).all()
    assert np.array_equal(short["d2"][0, 0, s - 5:s + t], out["d2"][0, 0, s - 5:s + t])
    # the windowed and the brute form agree on the whole box, at the short range too
    for kw in (dict(max_distance=0.55), dict(max_distance=100.0, unknown_is_obstacle=True)):
        small = (origin, (3 * vps, 5, 4))
        a = dr.distance_field(blocks, mc.VOXEL_SIZE, *small, 1, min_weight=mc.MESH_MIN_WEIGHT, form="windowed", **kw)
        b = dr.distance_field(blocks, mc.VOXEL_SIZE, *small, 1, min_weight=mc.MESH_MIN_WEIGHT, form="brute", **kw)
        for k in dr.FIELDS:
            assert a[k].tobytes() == b[k].tobytes(), (kw, k)


@pytest.mark.parametrize("vps,ratio", [(16, 2), (16, 4), (8, 2), (8, 4)])
def test_a_cell_takes_the_least_observed_distance_of_its_voxels(vps, ratio):
    indices, layers, g = dc.wall(vps, with_group=True)
    blocks = blocks_of(indices, layers, vps)
    first = dc.group_first_cell(dc.WALL_ORIGIN, vps, ratio)
    dims = tuple(d * vps // ratio for d in dc.WALL_DIMS)
    observed, obstacle = dr.classify(blocks, first, dims, ratio, mc.MESH_MIN_WEIGHT, 0.0)
    s, t = dc.wall_start(vps), dc.WALL_THICKNESS
    col = np.arange(dims[0])
    # a cell is an obstacle iff one of its columns lies in the slab -- the slab starts inside a cell: S is no multiple of the ratio --
    # and observed iff one of its columns is (the last slab column shares a cell with unobserved ones or not, either way)
    assert s % ratio != 0
    want_obst = (col * ratio < s + t) & ((col + 1) * ratio > s)
    want_obs = col * ratio < s + t
    assert (obstacle == want_obst[None, None, :]).all() and (observed == want_obs[None, None, :]).all()
    # the same from the voxel arrays directly, on the random map: least distance over the voxels with weight >= min_weight
    indices, layers, g = dc.random(vps, with_group=True)
    blocks = blocks_of(indices, layers, vps)
    first = dc.group_first_cell(mc.ORIGIN, vps, ratio)
    dims = tuple(d * vps // ratio for d in dc.RANDOM_DIMS)
    mw, sd = f32(1.5), f32(0.4 * mc.TRUNCATION)
    observed, obstacle = dr.classify(blocks, first, dims, ratio, mw, sd)
    present = np.zeros(g.w.shape, bool)
    for p in g.present:
        present[g.block_slices(p)] = True
    ok = present & (g.w >= mw)
    dd = np.where(ok, g.d, np.inf).reshape(dims[0], ratio, dims[1], ratio, dims[2], ratio).min(axis=(1, 3, 5))
    assert np.array_equal(observed.transpose(2, 1, 0), np.isfinite(dd)) and np.array_equal(obstacle.transpose(2, 1, 0), dd <= sd)
    # the explicit min_weight matters: voxel by voxel (ratio 1) fewer are observed than with the default
    vdims = tuple(d * vps for d in dc.RANDOM_DIMS)
    vfirst = dc.group_first_cell(mc.ORIGIN, vps, 1)
    heavy, light = (dr.classify(blocks, vfirst, vdims, 1, m, sd)[0].sum() for m in (mw, mc.MESH_MIN_WEIGHT))
    assert heavy == ok.sum() and 0 < heavy < light == (present & (g.w >= mc.MESH_MIN_WEIGHT)).sum()
    assert 0 < obstacle.sum() <= observed.sum() < observed.size


def test_an_empty_obstacle_set_leaves_everything_out_of_range():
    indices, layers = dc.wall(16)
    blocks = blocks_of(indices, layers, 16)
    first = dc.group_first_cell(dc.WALL_ORIGIN, 16, 1)
    out = dr.distance_field(blocks, mc.VOXEL_SIZE, first, (dc.wall_start(16) - 1, 9, 7), 1, max_distance=50.0, min_weight=mc.MESH_MIN_WEIGHT)
    assert (out["d2"] == dr.FAR).all() and (out["distance"] == f32(50.0)).all() and (out["status"] == 1).all()
    assert out["stats"]["n_in_range"] == 0 and out["stats"]["n_free"] == out["d2"].size
    # nothing at all: a box far from every block, unknown cells as obstacles -- no free cell to measure against
    out = dr.distance_field(blocks, mc.VOXEL_SIZE, (5000, 5000, 5000), (4, 5, 6), 1, max_distance=50.0, unknown_is_obstacle=True)
    assert (out["d2"] == -dr.FAR).all() and (out["distance"] == f32(-50.0)).all() and not out["status"].any()


@pytest.fixture(scope="module")
def world():
    """the oracle half of common.make_pair / step_both: the stream of tests/test_cpu_query_points.py"""
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
    return dict(cfg=cfg, blocks=blocks, frame=fr, dyn=np.asarray(dyn), sensor=osen)


def test_the_stream_box_holds_every_class_and_both_ranges(world):
    cfg = world["cfg"]
    origin, dims = dc.stream_box(world["frame"]["pose"], cfg.voxel_size)
    out = dr.distance_field(world["blocks"], cfg.voxel_size, origin, dims, dc.STREAM_RATIO, dc.STREAM_MAX_DISTANCE, cfg.mesh_min_weight)
    n = out["d2"].size
    st = out["stats"]
    shares = {"obstacle": st["n_obstacle"] / n, "free": st["n_free"] / n, "unknown": (n - st["n_observed"]) / n, "in_range": st["n_in_range"] / n}
    print("stream box origin %s dims %s: %s" % (origin, dims, {k: round(v, 4) for k, v in shares.items()}))
    assert min(shares["obstacle"], shares["free"], shares["unknown"]) >= 0.01
    assert 0 < st["n_in_range"] < n
    # what the GPU test asserts independently of the replica, on the oracle's map first
    status, dist = out["status"], out["distance"]
    free = (status & 3) == 1
    obst = (status & 2) != 0
    nb = np.zeros_like(obst)
    for axis in range(3):
        for sh in (1, -1):
            r = np.roll(obst, sh, axis=axis)
            edge = [slice(None)] * 3
            edge[axis] = 0 if sh == 1 else -1
            r[tuple(edge)] = False
            nb |= r
    med = float(np.median(dist[free & nb]))
    print("median distance of the %d free cells beside an obstacle cell: %.4f (cell size %.4f)" % ((free & nb).sum(), med, out["cell_size"]))
    assert med == out["cell_size"]
    c = dc.surface_cells(world["frame"], world["sensor"], world["dyn"], out["cell_size"], origin, dims)
    seen = (status[c[:, 2], c[:, 1], c[:, 0]] & 1) != 0
    near = np.abs(dist[c[:, 2], c[:, 1], c[:, 0]][seen]) <= f32(2) * f32(out["cell_size"])
    print("surface pixels in the box: %d, observed cell: %d, within two cells: %.4f" % (len(c), seen.sum(), near.mean()))
    assert seen.sum() > 1000 and near.mean() >= 0.95


def test_distance_field_config_reads_the_reference_mapper_file():
    out = subprocess.run([SELFTEST, "--distance-config", os.path.join(ROOT, "tests", "golden", "uHumans2.yaml")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(kv.split("=") for kv in out.stdout.split())
    assert f32(float(got["max_distance_m"])) == f32(4.5) and f32(float(got["min_weight"])) == f32(1.0e-6), got
    assert got["positive_distance_only"] == "1" and got["ratio"] == "2", got
