"""Hand-built inputs for khr_places_graph / khr_places_graph_from (tests/test_cpu_places_replica.py, tests/test_gpu_places_graph.py),
with the counts the constructions give written by hand.

The Voronoi cases are voronoi_cases.corridor / posts under (L1, separation 4, range 100 m, min_distance 2 cells): VORONOI_COUNTS maps
(case, compression, min_component_size) to (places, sorted place sizes or None, edges).

The synthetic member sets are fields built in numpy, no map needed: `field(dims, cells)` makes the four arrays [z, y, x] with the listed
cells as members (basis 2, d2 from `d2_of`), every other cell basis 0, d2 = 2^30, site -1.  SYNTHETIC lists (name, builder); a builder
returns (origin, dims, field, request keywords, expected) where `expected` holds the hand counts that are asserted on top of the
comparison with tests/places_replica.py."""
import numpy as np

import voronoi_cases as vc
import voronoi_replica as vr

f32 = np.float32
CELL = f32(0.1)
FAR = 1 << 30

# (L1, 4, range 100 m), min_distance MIN_DISTANCE_CELLS cells
VORONOI_KW = dict(mode=vr.L1, parent_l1_separation=4, parent_cos_angle_separation=0.0)
# the corridor's 72 listed cells are the columns x = 6, 7 = global -9, -8: floor division puts -9 into bucket -2 and -8 into bucket
# -1 at compression 8, and the rows y = 35 .. 40 split 5 + 1 -- 4 places; division that truncates towards zero would put both
# columns into bucket -1 and give 2 places (CORRIDOR_TRUNCATED_8)
VORONOI_COUNTS = {
    ("even", 16, 1): (1, [72], 0), ("even", 16, 3): (0, [], 0),
    ("even", 8, 1): (4, [6, 6, 30, 30], 6),
    ("even", 1, 1): (72, [1] * 72, 476), ("even", 2, 1): (24, None, 128),
    ("odd", 8, 1): (2, [12, 60], 1), ("odd", 8, 3): (0, [], 0),
    ("posts", 16, 1): (1, [336], 0),
    ("posts", 8, 1): (8, [5, 5, 18, 20, 30, 30, 108, 120], 28),
    ("posts", 4, 1): (30, None, 146),
}
CORRIDOR_TRUNCATED_8 = 2


def voronoi_case(key):
    return {"even": lambda: vc.corridor(vc.CORRIDOR_EVEN), "odd": lambda: vc.corridor(vc.CORRIDOR_ODD), "posts": vc.posts}[key]()


def voronoi_field_of_case(case):
    """the Voronoi field of a voronoi_cases case from its construction (everything observed, the obstacle set as built)"""
    _, _, origin, dims, in_set = case
    return vr.field_of(in_set, np.ones_like(in_set), in_set, origin, f32(0.1), 1000, 100.0, min_distance=vc.MIN_DISTANCE_CELLS * float(f32(0.1)), **VORONOI_KW)


def field(dims, cells, d2_of=None, basis=2, site_of=None):
    nx, ny, nz = dims
    d2 = np.full((nz, ny, nx), FAR, np.int32)
    b = np.zeros((nz, ny, nx), np.uint8)
    site = np.full((nz, ny, nx), -1, np.int32)
    for i, (x, y, z) in enumerate(cells):
        d2[z, y, x] = 4 + (i * 7) % 23 if d2_of is None else d2_of(i, x, y, z)
        b[z, y, x] = basis
        site[z, y, x] = (i * 31) % (nx * ny * nz) if site_of is None else site_of(i, x, y, z)
    dist = np.where(d2 < FAR, CELL * np.sqrt(np.clip(np.where(d2 < FAR, d2, 0), 0, None).astype(f32)), f32(100.0)).astype(f32)
    return dict(distance=dist, d2=d2, basis=b, site=site)


def plane_snake(z=0):
    """135 cells in one 16 x 16 plane: the rows y = 0, 2, .. 14 in full, joined at alternating ends by one cell in the rows between"""
    cells = []
    for r in range(8):
        xs = range(16) if r % 2 == 0 else range(15, -1, -1)
        cells += [(x, 2 * r, z) for x in xs]
        if r < 7:
            cells.append((15 if r % 2 == 0 else 0, 2 * r + 1, z))
    return cells


def snake_in_a_plane():
    cells = plane_snake(5)
    assert len(cells) == 135
    return (32, -16, 0), (16, 16, 16), field((16, 16, 16), cells), dict(compression=16), dict(places=1, edges=0, sizes=[135], first=(0, 0, 5))


def snake_through_a_bucket():
    """the plane snake in the planes z = 0, 2, .. 14, one cell between two planes at alternating ends of the snake"""
    cells = []
    for k in range(8):
        cells += plane_snake(2 * k)
        if k < 7:
            cells.append((0, 14 if k % 2 == 0 else 0, 2 * k + 1))
    # an odd plane's snake is walked from its end: the same cells
    assert len(set(cells)) == len(cells) == 8 * 135 + 7
    return (-16, -32, 16), (16, 16, 16), field((16, 16, 16), cells), dict(compression=16), dict(places=1, edges=0, sizes=[1087], first=(0, 0, 0))


def two_combs():
    """two interleaved combs in the plane z = 3 that never touch: teeth two cells apart, each ending five cells from the other's back"""
    a = [(x, 0, 3) for x in range(16)] + [(x, y, 3) for x in (0, 4, 8, 12) for y in range(1, 11)]
    b = [(x, 15, 3) for x in range(16)] + [(x, y, 3) for x in (2, 6, 10, 14) for y in range(5, 15)]
    return (0, 0, 0), (16, 16, 16), field((16, 16, 16), a + b), dict(compression=16), dict(places=2, edges=0, sizes=[56, 56], components=2)


def checkerboard():
    cells = [(x, y, z) for z in range(16) for y in range(16) for x in range(16) if (x + y + z) % 2 == 0]
    return (16, 16, -16), (16, 16, 16), field((16, 16, 16), cells), dict(compression=16), dict(places=1, edges=0, sizes=[2048])


def long_chain():
    """600 cells that form a PATH under 26-adjacency: rows x = 1 .. 14 at y = 0, 2, .., the turn between two rows one diagonal cell
    at x = 15 or x = 0 (a square turn would make a triangle); at compression 1 every cell is a place"""
    cells = []
    for r in range(40):
        xs = range(1, 15) if r % 2 == 0 else range(14, 0, -1)
        cells += [(x, 2 * r, 0) for x in xs]
        cells.append((15 if r % 2 == 0 else 0, 2 * r + 1, 0))
    assert len(cells) == 600
    return (-3, 7, 11), (16, 80, 1), field((16, 80, 1), cells), dict(compression=1), dict(places=600, edges=599, components=1, chain=cells)


def one_cell_member():
    return (-5, 0, 9), (1, 1, 1), field((1, 1, 1), [(0, 0, 0)]), dict(compression=4), dict(places=1, edges=0, sizes=[1])


def one_cell_empty():
    return (-5, 0, 9), (1, 1, 1), field((1, 1, 1), []), dict(compression=4), dict(places=0, edges=0, sizes=[])


def small_unaligned():
    """5 x 4 x 3 cells, all members, at (-21, -5, -9): inside the 16-bucket (-2, -1, -1)"""
    dims = (5, 4, 3)
    cells = [(x, y, z) for z in range(3) for y in range(4) for x in range(5)]
    return (-21, -5, -9), dims, field(dims, cells), dict(compression=16), dict(places=1, edges=0, sizes=[60])


def small_unaligned_4():
    """the same at compression 4: x = -21 | -20 .. -17, y = -5 | -4 .. -2, z = -9 | -8, -7: eight places, all touching"""
    o, dims, f, _, _ = small_unaligned()
    return o, dims, f, dict(compression=4), dict(places=8, edges=28, sizes=sorted([1 * 1 * 1, 4, 3, 12, 2, 8, 6, 24]), components=1)


def single_member():
    return (3, -9, 4), (7, 5, 6), field((7, 5, 6), [(4, 2, 3)], site_of=lambda i, x, y, z: 1), dict(compression=5), dict(places=1, edges=0, sizes=[1])


def full(compression):
    """12^3 cells, all members, across bucket borders on every axis"""
    def build():
        dims = (12, 12, 12)
        cells = [(x, y, z) for z in range(12) for y in range(12) for x in range(12)]
        pairs = sum((12 - abs(dx)) * (12 - abs(dy)) * (12 - abs(dz)) for dx, dy, dz in FORWARD)   # 13 n minus the boundary terms
        exp = dict(places=1728, edges=pairs, components=1) if compression == 1 else dict(places=8, edges=28, components=1)
        return (-6, 10, 26), dims, field(dims, cells), dict(compression=compression), exp
    return build


FORWARD = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) > (0, 0, 0)]


def centre_ties():
    """a 3 x 3 x 1 place whose greatest d2 (9) occurs at (2, 0), (0, 1) and (1, 2): the centre is (2, 0), the least lin"""
    cells = [(x, y, 0) for y in range(3) for x in range(3)]
    top = {(2, 0), (0, 1), (1, 2)}
    f = field((3, 3, 1), cells, d2_of=lambda i, x, y, z: 9 if (x, y) in top else 5)
    return (8, 8, 8), (3, 3, 1), f, dict(compression=8), dict(places=1, edges=0, sizes=[9], centre=(10, 8, 8), centre_d2=9)


def d2_out_of_range():
    """a row of five cells with basis 2; the second has d2 = -1 and the fourth d2 = 2^30: no members, so three places in a row's stead"""
    cells = [(x, 0, 0) for x in range(5)]
    f = field((5, 1, 1), cells, d2_of=lambda i, x, y, z: {1: -1, 3: FAR}.get(x, 6))
    f["distance"][0, 0, :] = CELL * f32(2)
    return (0, 0, 0), (5, 1, 1), f, dict(compression=16), dict(places=3, edges=0, sizes=[1, 1, 1], components=3)


def no_site():
    cells = [(0, 0, 0), (1, 0, 0), (3, 1, 1)]
    f = field((4, 2, 2), cells, site_of=lambda i, x, y, z: -1 if x < 2 else 9, d2_of=lambda i, x, y, z: 7)
    return (-2, -2, -2), (4, 2, 2), f, dict(compression=16), dict(places=2, edges=0, sizes=[1, 2])   # (x = -2, -1 | 1: buckets -1 and 0, two cells apart)


def sites_out_of_range():
    """three lone cells of a 5-cell row at (1, 2, 3): the first's site is 5 = nx ny nz (one past the box), the second's -7 (below -1),
    the third's 4: zeros, zeros, the global cell (5, 2, 3)"""
    cells = [(0, 0, 0), (2, 0, 0), (4, 0, 0)]
    f = field((5, 1, 1), cells, site_of=lambda i, x, y, z: {0: 5, 2: -7, 4: 4}[x], d2_of=lambda i, x, y, z: 3)
    return (1, 2, 3), (5, 1, 1), f, dict(compression=16), dict(places=3, edges=0, sizes=[1, 1, 1], sites=[(0, 0, 0), (0, 0, 0), (5, 2, 3)])


def random_members(dims, seed, density=0.3):
    def build():
        rng = np.random.default_rng(seed)
        nx, ny, nz = dims
        m = rng.random((nz, ny, nx)) < density
        cells = [(int(x), int(y), int(z)) for z, y, x in np.argwhere(m)]
        vals = rng.integers(1, 40, len(cells))
        return (-7, 13, -30), dims, field(dims, cells, d2_of=lambda i, x, y, z: int(vals[i])), dict(compression=3 + seed % 4), dict()
    return build


SYNTHETIC = [("plane_snake", snake_in_a_plane), ("bucket_snake", snake_through_a_bucket), ("combs", two_combs), ("checkerboard", checkerboard),
             ("chain", long_chain), ("one_cell_member", one_cell_member), ("one_cell_empty", one_cell_empty), ("small_unaligned", small_unaligned),
             ("small_unaligned_4", small_unaligned_4), ("single", single_member), ("full_16", full(16)), ("full_1", full(1)),
             ("centre_ties", centre_ties), ("d2_range", d2_out_of_range), ("no_site", no_site), ("bad_sites", sites_out_of_range),
             ("65x3x2", random_members((65, 3, 2), 1)),
             ("2x2x257", random_members((2, 2, 257), 2)), ("37x21x45", random_members((37, 21, 45), 3, 0.12))]

# the random member field: 3 % obstacles on 37 x 21 x 45 cells at (-40, 5, -77), range 8 cells, cells of 0.1 m, (L1, 4), min_distance 0
# so that min_node_distance = 0.25 m does the selecting
RANDOM_ORIGIN, RANDOM_DIMS, RANDOM_R, RANDOM_MIN_NODE_DISTANCE = (-40, 5, -77), (37, 21, 45), 8, 0.25
RANDOM_COMPRESSIONS, RANDOM_SIZES = (1, 3, 5, 16), (1, 3)
# With the generator below: 4173 members in 58 components, whatever the compression; kept at min_component_size 3.  (The issue
# quotes 67 components with 28 / 21 / 16 / 4 kept from a prototype whose random seed it does not state, so those figures cannot be
# reproduced; these are the counts of THIS field, from tests/places_replica.py, and they serve the same end: at every compression
# some components are dropped and some kept, so the filter, the renumbering and the edge compaction all do work.)
RANDOM_COMPONENTS, RANDOM_KEPT = 58, {1: 34, 3: 24, 5: 17, 16: 5}


def random_field(seed=2021):
    nx, ny, nz = RANDOM_DIMS
    in_set = np.random.default_rng(seed).random((nz, ny, nx)) < 0.03
    return vr.field_of(in_set, np.ones_like(in_set), in_set, RANDOM_ORIGIN, CELL, RANDOM_R, float(CELL) * RANDOM_R + 0.05, min_distance=0.0, **VORONOI_KW)
