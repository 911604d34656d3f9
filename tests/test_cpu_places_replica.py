"""-m "not gpu": tests/places_replica.py, the plain restatement of khr_places_graph (ASSUMPTIONS.md A.21), held to the hand counts of
tests/places_cases.py, to a second closure (min-propagation), to the properties the definition promises -- every member in exactly
one place inside one bucket, shift invariance, refinement under compression, components independent of compression -- and to its own
lists.  The stream box of tests/voronoi_cases.py is proven not to be vacuous on the CPU oracle's map; hydra::PlacesConfig reads the
reference's values."""
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as dc
import places_cases as pc
import places_replica as pr
import voronoi_cases as vc
import voronoi_replica as vr
from khronos_amd import capi
from test_cpu_voronoi_replica import world  # noqa: F401  (the oracle's 30-frame map, a module-scoped fixture)

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "khronos_amd", "lib", "host_selftest")
_fields = {}


def voronoi(key):
    if key not in _fields:
        case = pc.voronoi_case(key)
        _fields[key] = (case, pc.voronoi_field_of_case(case))
    return _fields[key]


def random_field():
    if "random" not in _fields:
        _fields["random"] = pc.random_field()
    return _fields["random"]


def graph(build):
    origin, dims, f, kw, exp = build()
    return origin, dims, f, kw, exp, pr.places_graph(origin, dims, f["distance"], f["d2"], f["basis"], f["site"], **kw)


def test_the_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "khronos_amd.h")).read()
    for name, n_args in (("khr_places_graph", 3), ("khr_places_graph_from", 10), ("khr_places_graph_into", 16), ("khr_places_graph_box", 3)):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTS
        assert len(getattr(capi.load_library(), name).argtypes) == n_args
    assert "khr_places_request" in header and "khr_places_stats" in header
    assert [k for k, _ in capi.KhrPlacesStats._fields_] == list(pr.STATS)
    assert [k for k, _, _, _ in capi.FusionContext.PL_FIELDS] == ["place"] + list(pr.PLACE_FIELDS) + list(pr.EDGE_FIELDS)


@pytest.mark.parametrize("key,compression,min_size", sorted(pc.VORONOI_COUNTS))
def test_the_hand_counts_of_corridors_and_posts(key, compression, min_size):
    case, f = voronoi(key)
    assert f["stats"]["n_listed"] == (336 if key == "posts" else 72)
    if key != "posts":   # the listed cells are two columns: global -9, -8 (even) or -8, -7 (odd)
        assert sorted(set(f["cells"][:, 0].tolist())) == ([-9, -8] if key == "even" else [-8, -7])
    g = pr.of_voronoi(f, case[2], compression=compression, min_component_size=min_size)
    places, sizes, edges = pc.VORONOI_COUNTS[(key, compression, min_size)]
    assert g["stats"]["n_places"] == places == len(g["n_cells"]) and g["stats"]["n_edges"] == edges == len(g["edge_a"])
    if sizes is not None:
        assert sorted(g["n_cells"].tolist()) == sizes
    assert g["stats"]["n_members"] == f["stats"]["n_listed"]


def test_buckets_round_towards_minus_infinity():
    """the even corridor at compression 8: columns -9 and -8 lie in buckets -2 and -1 -- 4 places; division that truncates towards zero
    puts both into bucket -1 and gives 2"""
    case, f = voronoi("even")
    assert pr.bucket_of(-9, 8) == -2 and pr.bucket_of(-8, 8) == -1 and pr.bucket_of(-9, 8, floor=False) == -1
    assert pr.of_voronoi(f, case[2], compression=8)["stats"]["n_places"] == 4
    assert pr.of_voronoi(f, case[2], compression=8, floor=False)["stats"]["n_places"] == pc.CORRIDOR_TRUNCATED_8 == 2


@pytest.mark.parametrize("name,build", pc.SYNTHETIC, ids=[n for n, _ in pc.SYNTHETIC])
def test_synthetic_member_sets(name, build):
    origin, dims, f, kw, exp, g = graph(build)
    st = g["stats"]
    nx, ny, nz = dims
    if "places" in exp:
        assert st["n_places"] == st["n_places_all"] == exp["places"] and st["n_edges"] == exp["edges"], st
    if "sizes" in exp:
        assert sorted(g["n_cells"].tolist()) == exp["sizes"]
    if "components" in exp:
        assert st["n_components"] == exp["components"]
    if "first" in exp:   # the representative: place 0 starts at the snake's first cell, which is the least lin
        x, y, z = exp["first"]
        assert g["place"][z, y, x] == 0 and np.flatnonzero(g["place"].ravel() == 0)[0] == x + nx * (y + ny * z)
    if "sites" in exp:   # a site outside [0, nx ny nz) gives zeros, like -1
        assert [tuple(int(v) for v in row) for row in g["site"]] == exp["sites"]
    if "centre" in exp:
        assert tuple(g["centre"][0]) == exp["centre"] and g["centre_d2"][0] == exp["centre_d2"]
    if "chain" in exp:
        ids = [int(g["place"][z, y, x]) for x, y, z in exp["chain"]]
        deg = g["degree"][ids]
        assert deg[0] == deg[-1] == 1 and (deg[1:-1] == 2).all() and (g["edge_n_contacts"] == 1).all()
    if name == "no_site":
        assert (g["site"][0] == 0).all() and tuple(g["site"][1]) == (origin[0] + 1, origin[1] + 0, origin[2] + 1)   # site 9 = (1, 0, 1)
    # the flood fill against the min-propagation closure
    member = pr.members_of(f["distance"], f["d2"], f["basis"])
    lab = pr.labels_minprop(member, origin, kw["compression"])
    place_of, places = pr.labels_flood(member, origin, kw["compression"])
    assert len(place_of) == int(member.sum()) == st["n_members"]
    for found in places:
        rep = min(c[0] + nx * (c[1] + ny * c[2]) for c in found)
        assert all(lab[c[2], c[1], c[0]] == rep for c in found)
        assert len({tuple((origin[a] + c[a]) // kw["compression"] for a in range(3)) for c in found}) == 1   # inside one bucket
    assert len(np.unique(lab[member])) == len(places)
    check_lists(origin, dims, f, g)


def check_lists(origin, dims, f, g):
    """sum, n_cells, degree, n_contacts, clearance and the orders against the dense output and the input arrays"""
    nx, ny, nz = dims
    place = g["place"]
    z, y, x = np.nonzero(place >= 0)
    ids = place[z, y, x]
    n = len(g["n_cells"])
    assert np.array_equal(np.bincount(ids, minlength=n), g["n_cells"])
    for a, v in enumerate((x, y, z)):
        assert np.array_equal(np.bincount(ids, weights=(v + origin[a]).astype(np.float64), minlength=n).astype(np.int64), g["sum"][:, a])
    first = np.full(n, place.size, np.int64)
    np.minimum.at(first, ids, x + nx * (y + ny * z))
    assert (np.diff(first) > 0).all()   # ascending representatives
    keys = g["edge_a"].astype(np.int64) << 32 | g["edge_b"].astype(np.int64)
    assert (g["edge_a"] < g["edge_b"]).all() and (np.diff(keys) > 0).all()
    assert np.array_equal(np.bincount(np.concatenate([g["edge_a"], g["edge_b"]]).astype(np.int64), minlength=n), g["degree"])
    pairs = {}
    for dx, dy, dz in pr.FORWARD:
        X, Y, Z = x + dx, y + dy, z + dz
        ok = (X >= 0) & (X < nx) & (Y >= 0) & (Y < ny) & (Z >= 0) & (Z < nz)
        q = np.where(ok, place[np.where(ok, Z, 0), np.where(ok, Y, 0), np.where(ok, X, 0)], -1)
        for i in np.flatnonzero((q >= 0) & (q != ids)):
            k = (min(ids[i], q[i]), max(ids[i], q[i]))
            v = min(int(f["d2"][z[i], y[i], x[i]]), int(f["d2"][Z[i], Y[i], X[i]]))
            e = pairs.setdefault(k, [0, 0])
            e[0], e[1] = max(e[0], v), e[1] + 1
    if g["stats"]["n_places"] == g["stats"]["n_places_all"]:   # (with a filter the dropped places' pairs are not in `place`)
        assert len(pairs) == len(g["edge_a"])
    for a, b, v, c in zip(g["edge_a"], g["edge_b"], g["edge_clearance_d2"], g["edge_n_contacts"]):
        assert pairs[(a, b)] == [v, c]
    assert (g["centre_d2"] == [f["d2"].ravel()[np.flatnonzero(place.ravel() == p)].max() for p in range(n)]).all()
    assert len(np.unique(g["component"])) == g["stats"]["n_components"] and (g["component"] < max(g["stats"]["n_components"], 1)).all()
    assert (g["component"][g["edge_a"].astype(np.int64)] == g["component"][g["edge_b"].astype(np.int64)]).all()


def test_shift_invariance():
    """the same field cut by a box shifted by (5, -7, 3), members away from both borders: the same places up to the offset"""
    f, o = random_field(), pc.RANDOM_ORIGIN
    nx, ny, nz = pc.RANDOM_DIMS
    sx, sy, sz = 5, -7, 3   # the second box's local cell c is the first box's c + shift
    a_part = (slice(max(sz, 0), nz + min(sz, 0)), slice(max(sy, 0), ny + min(sy, 0)), slice(max(sx, 0), nx + min(sx, 0)))
    b_part = (slice(max(-sz, 0), nz + min(-sz, 0)), slice(max(-sy, 0), ny + min(-sy, 0)), slice(max(-sx, 0), nx + min(-sx, 0)))
    keep = np.zeros((nz, ny, nx), bool)
    keep[a_part] = True
    basis = np.where(keep, f["basis"], 0).astype(np.uint8)
    kw = dict(compression=5, min_node_distance=pc.RANDOM_MIN_NODE_DISTANCE)
    a = pr.places_graph(o, pc.RANDOM_DIMS, f["distance"], f["d2"], basis, f["site"], **kw)
    shifted = {k: np.zeros_like(f[k]) for k in ("distance", "d2", "basis")}
    for k in shifted:
        shifted[k][b_part] = (basis if k == "basis" else f[k])[a_part]
    site = np.full((nz, ny, nx), -1, np.int32)   # (site indices are box-local: left out of the comparison)
    b = pr.places_graph((o[0] + sx, o[1] + sy, o[2] + sz), pc.RANDOM_DIMS, shifted["distance"], shifted["d2"], shifted["basis"], site, **kw)
    assert a["stats"] == b["stats"] and a["stats"]["n_places"] > 20 and a["stats"]["n_edges"] > 20
    assert np.array_equal(a["place"][a_part], b["place"][b_part])
    for k in ("centre", "centre_d2", "radius", "basis", "n_cells", "sum", "degree", "component") + pr.EDGE_FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_refinement_and_components_do_not_depend_on_compression():
    f, o = random_field(), pc.RANDOM_ORIGIN
    kw = dict(min_node_distance=pc.RANDOM_MIN_NODE_DISTANCE)
    fine = pr.of_voronoi(f, o, compression=1, **kw)
    assert fine["stats"]["n_places"] == fine["stats"]["n_members"] and (fine["n_cells"] == 1).all()
    member = fine["place"] >= 0
    comp_fine = fine["component"][fine["place"][member]]
    for c in pc.RANDOM_COMPRESSIONS[1:]:
        g = pr.of_voronoi(f, o, compression=c, **kw)
        assert np.array_equal(g["place"] >= 0, member)   # a place at compression c is a union of places at compression 1
        assert g["stats"]["n_components_all"] == fine["stats"]["n_components_all"] == pc.RANDOM_COMPONENTS
        assert np.array_equal(g["component"][g["place"][member]], comp_fine)


@pytest.mark.parametrize("compression", pc.RANDOM_COMPRESSIONS)
def test_the_random_field_makes_the_filter_work(compression):
    f, o = random_field(), pc.RANDOM_ORIGIN
    kw = dict(min_node_distance=pc.RANDOM_MIN_NODE_DISTANCE, compression=compression)
    everything, kept = pr.of_voronoi(f, o, **kw), pr.of_voronoi(f, o, min_component_size=3, **kw)
    print(compression, everything["stats"], kept["stats"])
    assert everything["stats"]["n_components"] == pc.RANDOM_COMPONENTS and kept["stats"]["n_components"] == pc.RANDOM_KEPT[compression]
    assert 0 < kept["stats"]["n_places"] < everything["stats"]["n_places"] and 0 < kept["stats"]["n_edges"] < everything["stats"]["n_edges"]
    check_lists(o, pc.RANDOM_DIMS, f, kept)
    # the kept places are the others' renumbered monotonically
    old = everything["place"][kept["place"] >= 0]
    new = kept["place"][kept["place"] >= 0]
    order = np.argsort(old, kind="stable")
    assert (np.diff(new[order]) >= 0).all() and ((np.diff(new[order]) > 0) == (np.diff(old[order]) > 0)).all()


def test_the_stream_box_holds_places_and_links(world):  # noqa: F811
    """the CPU oracle's 30-frame map, voronoi_cases.STREAM box: compression 4 is not vacuous"""
    cfg = world["cfg"]
    origin, dims = dc.stream_box(world["frame"]["pose"], cfg.voxel_size)
    kw = dict(vc.STREAM)
    cell = f32(cfg.voxel_size) * f32(kw["ratio"])
    f = vr.voronoi_field(world["blocks"], cfg.voxel_size, origin, dims, kw.pop("ratio"), kw.pop("max_distance"), cfg.mesh_min_weight,
                         min_distance=vc.MIN_DISTANCE_CELLS * float(cell), **kw)
    g = pr.of_voronoi(f, origin, compression=4)
    print("stream box: %s" % g["stats"])
    assert g["stats"]["n_places"] >= 2 and g["stats"]["n_edges"] >= 1
    check_lists(origin, dims, f, g)


def test_places_config_reads_the_reference_values():
    out = subprocess.run([SELFTEST, "--places-config"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict(kv.split("=") for kv in out.stdout.split())
    # graph.compression_distance_m 1.5 over cells of 0.2 m (voxels of 0.1 m, ratio 2) gives 7; filter_places with components of 3
    assert int(got["compression"]) == 7 and abs(float(got["min_node_distance"]) - 0.4) < 1e-6 and int(got["min_component_size"]) == 3
    assert int(got["compression_small_cells"]) == 16 and int(got["compression_large_cells"]) == 1 and int(got["unfiltered_min_component_size"]) == 1
