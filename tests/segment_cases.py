"""Hand-built maps for khr_segment_map (ASSUMPTIONS.md A.19), on merge_cases.rich_map / diff_cases.solid_map: (indices, layers)
pairs in the form of khronos_amd.checkpoint, fixed seeds, at most a few tens of blocks.  Each case is named for the way the
kernels can go wrong and carries its `runs`: request keywords plus, under "expect", the component count written by hand (None where
only the replica says).  Needs no device."""
import functools
import itertools

import numpy as np

import diff_cases as dc
import merge_cases as mc
from khronos_amd import checkpoint as ck

f32 = np.float32
CFG16, CFG8 = mc.CFG16, mc.CFG8
INF = f32(np.inf)
MESH_MIN_WEIGHT = 1e-4  # khr_default_config's mesh_min_weight: what min_weight = 0 stands for in the contexts of the tests
OCC, FREE = f32(-0.1), f32(0.1)  # a member's distance and a non-member's at surface_distance = 0


def block_of(v, vps):
    return tuple(int(c) // vps for c in v)  # (Python's floor division: negative indices too)


def sparse_map(cfg, members, extra_blocks=(), seed=1, label=1, kind="solid"):
    """every voxel of `members` (global voxel indices; a dict gives each its label) observed and occupied, every other voxel of the
    blocks they lie in and of `extra_blocks` observed and free; the other layers rich"""
    vps = ck.config_fields(cfg)["voxels_per_side"]
    labels = members if isinstance(members, dict) else {tuple(v): label for v in members}
    blocks = sorted({block_of(v, vps) for v in labels} | {tuple(b) for b in extra_blocks})
    idx, L = mc.rich_map(cfg, [(b, kind) for b in blocks], seed)
    L["distance"][:] = FREE
    row = {b: i for i, b in enumerate(blocks)}
    for v, lab in labels.items():
        b = block_of(v, vps)
        lin = (v[0] - b[0] * vps) + vps * ((v[1] - b[1] * vps) + vps * (v[2] - b[2] * vps))
        L["distance"][row[b], lin] = OCC
        L["sem_label"][row[b], lin] = lab
    return idx, L


def case(name, cfg, now, runs, **extra):
    return dict(name=name, cfg=cfg, now=now, runs=runs, **extra)


def by_connectivity(e6, e18, e26, **kw):
    return [dict(connectivity=c, expect=e, **kw) for c, e in ((6, e6), (18, e18), (26, e26))]


def _pairs(cfg, tag):
    """two members differing by a face, an edge and a corner offset: inside a block, across a block face, a block edge and a block
    corner; around the edge and the corner the other blocks once absent and once present without members.  Every placement has a
    neighbourhood of blocks of its own, around negative block indices."""
    vps = ck.config_fields(cfg)["voxels_per_side"]
    e = vps - 1
    face, edge, corner = (1, 0, 0), (1, 1, 0), (1, 1, 1)
    # (kind, offset, the first voxel inside its block: which axes of the offset leave the block, the other blocks present?)
    layout = [("face", face, (3, 4, 5), False), ("face", face, (e, 4, 5), False),
              ("edge", edge, (3, 4, 5), False), ("edge", edge, (e, 4, 5), False), ("edge", edge, (e, e, 5), False), ("edge", edge, (e, e, 5), True),
              ("corner", corner, (3, 4, 5), False), ("corner", corner, (e, 4, 5), False), ("corner", corner, (e, e, 5), False),
              ("corner", corner, (e, e, e), False), ("corner", corner, (e, e, e), True)]
    members, extra, pairs = [], [], []
    for i, (kind, off, v, fill) in enumerate(layout):
        base = (-9 + 4 * (i % 4), -7 + 4 * (i // 4), -2)  # the block of the first voxel
        a = tuple(base[k] * vps + v[k] for k in range(3))
        b = tuple(a[k] + off[k] for k in range(3))
        members += [a, b]
        pairs.append((kind, a, b))
        if fill:  # every block around the edge or the corner
            span = [(0, 1) if v[k] == e and off[k] else (0,) for k in range(3)]
            extra += [tuple(base[k] + d[k] for k in range(3)) for d in itertools.product(*span)]
    n = len(layout)
    n_face, n_edge = sum(k == "face" for k, *_ in layout), sum(k == "edge" for k, *_ in layout)
    # by hand: 11 pairs; at 6 the two face pairs join (20 components), at 18 also the four edge pairs (16), at 26 all (11)
    assert (n, n_face, n_edge) == (11, 2, 4)
    return case("pairs" + tag, cfg, sparse_map(cfg, members, extra, seed=11), by_connectivity(20, 16, 11), pairs=pairs)


def _snake(cfg, tag, expect_len):
    """a one-voxel-wide 6-connected serpentine through one block: full rows along x on even y and even z, joined at alternating
    ends; one component at 6, as long as a block allows"""
    vps = ck.config_fields(cfg)["voxels_per_side"]
    path, at_end = [], False
    for z in range(0, vps, 2):
        ys = list(range(0, vps, 2))
        if (z // 2) % 2:
            ys.reverse()
        for j, y in enumerate(ys):
            path += [(x, y, z) for x in range(vps)]
            at_end = not at_end
            x_turn = vps - 1 if at_end else 0
            if j + 1 < len(ys):
                path.append((x_turn, (y + ys[j + 1]) // 2, z))
            elif z + 2 < vps:
                path.append((x_turn, y, z + 1))
    assert len(set(path)) == len(path) == expect_len
    b = (-1, 0, -2)
    members = [tuple(b[k] * vps + v[k] for k in range(3)) for v in path]
    return case("snake" + tag, cfg, sparse_map(cfg, members, seed=21), [dict(connectivity=6, expect=1), dict(connectivity=26, expect=1)], n_voxels=expect_len)


def _zigzag():
    """a path that crosses one block face eight times, the connecting voxels alternately on either side: each block holds pieces
    that only the other block joins.  The same across a block edge at 18 (the two other blocks around the edge absent)."""
    vps, e = 16, 15
    a, b = (-1, 0, 0), (0, 0, 0)
    m = []
    for y in range(0, 16, 2):  # crossings at y = 0, 2, .., 14
        m += [(a[0] * vps + e, y, 5), (b[0] * vps, y, 5)]
        if y + 1 < 15:
            m.append(((b[0] * vps) if (y // 2) % 2 == 0 else (a[0] * vps + e), y + 1, 5))
    face = case("zigzag_face", CFG16, sparse_map(CFG16, m, seed=31), by_connectivity(1, 1, 1))
    m = []
    for z in range(0, 16, 2):  # A = (0, 0, 0) voxel (15, 15, z), D = (1, 1, 0) voxel (0, 0, z): an edge offset apart
        m += [(e, e, z), (16, 16, z)]
        if z + 1 < 15:
            m.append((16, 16, z + 1) if (z // 2) % 2 == 0 else (e, e, z + 1))
    # by hand at 6: A holds {0}, {2,3,4}, {6,7,8}, {10,11,12}, {14}, D holds {0,1,2}, {4,5,6}, {8,9,10}, {12,13,14}: 9 pieces
    edge = case("zigzag_edge", CFG16, sparse_map(CFG16, m, seed=32), by_connectivity(9, 1, 1))
    return [face, edge]


def _rings():
    """a closed loop through 2 x 2 blocks, and one around a block corner through all 8 blocks (a Hamiltonian cycle along the edges
    of the cube [14, 17]^3)"""
    sq = [(x, y, 3) for x in range(13, 19) for y in range(13, 19) if x in (13, 18) or y in (13, 18)]
    sq = [(x - 16, y - 16, z) for x, y, z in sq]  # around the block edge at x = y = 0: blocks (-1..0, -1..0, 0)
    flat = case("ring_2x2", CFG16, sparse_map(CFG16, sq, seed=41), by_connectivity(1, 1, 1), n_voxels=20)
    gray = [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1), (1, 0, 0)]
    cube = set()
    for p, q in zip(gray, gray[1:] + gray[:1]):
        for t in range(4):
            cube.add(tuple(14 + (3 * p[k] if p[k] == q[k] else (t if q[k] > p[k] else 3 - t)) for k in range(3)))
    cube = [(x - 32, y - 16, z) for x, y, z in cube]  # the corner at (-16, 0, 16): blocks (-2..-1, -1..0, 0..1)
    assert len({block_of(v, 16) for v in cube}) == 8
    corner = case("ring_corner", CFG16, sparse_map(CFG16, cube, seed=42), by_connectivity(1, 1, 1), n_voxels=24)
    return [flat, corner]


def _checker(cfg, tag, labels):
    """a solid block whose labels alternate in a 3D checkerboard: vps^3 one-voxel components with by_label at 6 (the most a block
    can hold), two at 18 and 26 (each colour hangs together through the edge offsets), one without by_label"""
    vps = ck.config_fields(cfg)["voxels_per_side"]
    idx, L = dc.solid_map(cfg, [(2, -1, 0)], 51, OCC)
    lin = np.arange(vps ** 3)
    L["sem_label"][0] = np.where((lin % vps + (lin // vps) % vps + lin // (vps * vps)) % 2 == 0, labels[0], labels[1]).astype(np.uint32)
    return case("checker" + tag, cfg, (idx, L), by_connectivity(vps ** 3, 2, 2, by_label=True) + by_connectivity(1, 1, 1, by_label=False))


def _big():
    """2 x 2 x 2 solid blocks at the top corner of the block index range and again at the bottom corner: two components of
    8 * 16^3 voxels (a neighbour lookup that wraps around the key range would join them), coordinate sums beyond 2^32"""
    top, bot = (1 << 20) - 2, -(1 << 20)
    blocks = [tuple(o + d for d in dd) for o in (top, bot) for dd in itertools.product((0, 1), repeat=3)]
    return case("big", CFG16, dc.solid_map(CFG16, blocks, 61, OCC), [dict(connectivity=26, by_label=False, expect=2), dict(connectivity=6, by_label=False, expect=2)],
                n_voxels=2 * 8 * 16 ** 3)


def _filter():
    """straight runs of 2, 3, 4, 6 and 7 voxels with min_voxels = 3 and max_voxels = 6: one too small, one too large, three kept
    and renumbered 1, 2, 3"""
    m = []
    for row, n in enumerate((7, 2, 4, 3, 6)):  # (not in order of size: the ids follow the representatives)
        m += [(x, 2 * row, 9) for x in range(12, 12 + n)]  # (from x = 12: the longer runs cross into the next block)
    runs = [dict(connectivity=6, min_voxels=3, max_voxels=6, expect=3, sizes=[4, 3, 6], small=1, large=1),
            dict(connectivity=6, min_voxels=0, max_voxels=0, expect=5, sizes=[7, 2, 4, 3, 6], small=0, large=0),
            dict(connectivity=6, min_voxels=7, max_voxels=7, expect=1, sizes=[7], small=4, large=0),
            dict(connectivity=6, min_voxels=8, max_voxels=-3, expect=0, sizes=[], small=5, large=0)]
    return case("filter", CFG16, sparse_map(CFG16, m, seed=71), runs)


def _thresholds():
    """isolated voxels at the thresholds: weight at min_weight and the float below it, distance at surface_distance and the float
    above it, weight at the context's mesh_min_weight and the float below it"""
    sd, mw, mmw = f32(0.02), mc.MIN_WEIGHT, f32(MESH_MIN_WEIGHT)
    idx, L = mc.rich_map(CFG16, [((0, -1, 0), "zero")], 81)
    L["distance"][:] = FREE
    spots = [(mw, sd), (np.nextafter(mw, f32(0)), sd), (mw, np.nextafter(sd, INF)), (f32(2.5), OCC), (mmw, OCC), (np.nextafter(mmw, f32(0)), OCC)]
    for i, (w, d) in enumerate(spots):
        L["weight"][0, 3 * i], L["distance"][0, 3 * i] = w, d
    # by hand: at min_weight = 0.5 the first and the fourth; at 0 (= 1e-4) also the second and the fifth
    return case("thresholds", CFG16, (idx, L), [dict(min_weight=float(mw), surface_distance=float(sd), expect=2),
                                                dict(min_weight=0.0, surface_distance=float(sd), expect=4)])


def _labels_flags():
    """twenty isolated voxels, voxel i with label i % 5 and flags i % 4 (| SEM_VALID on every other one)"""
    idx, L = mc.rich_map(CFG16, [((1, 1, -1), "solid")], 91)
    L["distance"][:] = FREE
    for i in range(20):
        lin = 2 * i + 64 * (i % 3)
        L["distance"][0, lin], L["sem_label"][0, lin], L["flags"][0, lin] = OCC, i % 5, (i % 4) | (8 if i % 2 else 0)
    many = list(range(100, 163)) + [4]
    assert len(many) == 64
    runs = [dict(labels=[2], expect=4), dict(labels=[1, 3], expect=8), dict(labels=many, expect=4), dict(labels=[7], expect=0),
            dict(flags_require=1, expect=10), dict(flags_exclude=2, expect=10), dict(flags_require=1, flags_exclude=2, expect=5),
            dict(flags_require=3, labels=[3, 0], expect=2)]  # (i % 4 == 3 and i % 5 in (0, 3): i = 3, 15)
    return case("labels_flags", CFG16, (idx, L), runs)


def _order():
    """diff_cases.ORDER_BLOCKS: five blocks whose (x, y, z) order is neither the order of their keys nor the order given; a run of
    two voxels in each"""
    m = []
    for i, b in enumerate(dc.ORDER_BLOCKS):
        m += [(b[0] * 16 + 3 + i, b[1] * 16 + 7, b[2] * 16 + 2 * i), (b[0] * 16 + 4 + i, b[1] * 16 + 7, b[2] * 16 + 2 * i)]
    idx, L = sparse_map(CFG16, m, seed=101)
    perm = [dc.ORDER_BLOCKS.index(tuple(b)) for b in idx.tolist()]  # sparse_map sorts: hand the blocks over in the order given
    inv = np.argsort(perm)
    return case("order", CFG16, (idx[inv], {k: v[inv] for k, v in L.items()}), by_connectivity(5, 5, 5), blocks=sorted(dc.ORDER_BLOCKS))


def _rich(cfg, tag, seed):
    """random members (about three voxels in ten: near the percolation threshold at 6) over touching blocks, next to absent blocks,
    a block of zero weights and a far block"""
    blocks = [((0, 0, 0), "rich"), ((1, 0, 0), "rich"), ((0, 1, 0), "rich"), ((1, 1, 0), "rich"), ((0, 0, 1), "rich"), ((1, 1, 1), "rich"),
              ((-1, 0, 0), "rich"), ((-1, -1, -1), "rich"), ((0, 1, 1), "zero"), ((3, 3, 3), "rich")]
    idx, L = mc.rich_map(cfg, blocks, seed)
    rng = np.random.default_rng(seed + 7000)
    L["distance"][:] = rng.choice(np.array([-0.1, 0.1, 0.0, np.nextafter(f32(0), INF), -0.03, 0.07], f32), L["distance"].shape)
    runs = [dict(connectivity=c, by_label=b, min_weight=float(mc.MIN_WEIGHT), expect=None) for c in (6, 18, 26) for b in (False, True)]
    return case("rich" + tag, cfg, (idx, L), runs)


def _empty():
    none = (np.zeros((0, 3), np.int32), mc.empty_layers(CFG16))
    zero = mc.rich_map(CFG16, [((0, 0, 0), "zero"), ((1, 0, 0), "zero")], 111)
    return [case("empty_map", CFG16, none, by_connectivity(0, 0, 0)), case("empty_no_members", CFG16, zero, by_connectivity(0, 0, 0, min_weight=0.5))]


CASES = [_pairs(CFG16, ""), _pairs(CFG8, "_vps8"), _snake(CFG16, "", 8 * (8 * 16 + 7) + 7), _snake(CFG8, "_vps8", 4 * (4 * 8 + 3) + 3), *_zigzag(), *_rings(),
         _checker(CFG16, "", (1, 2)), _checker(CFG8, "_vps8", (0, 1)), _big(), _filter(), _thresholds(), _labels_flags(), _order(),
         _rich(CFG16, "", 121), _rich(CFG8, "_vps8", 122), *_empty()]
BY_NAME = {c["name"]: c for c in CASES}
REQUEST_KEYS = ("min_weight", "surface_distance", "connectivity", "by_label", "labels", "flags_require", "flags_exclude", "min_voxels", "max_voxels")


def request_of(run):
    return {k: run[k] for k in REQUEST_KEYS if k in run}


@functools.lru_cache(maxsize=None)
def _replica(name, i, want_voxels):
    import segment_replica as sr
    c = BY_NAME[name]
    return sr.segment(ck.config_fields(c["cfg"]), c["now"][0], c["now"][1], want_voxels=want_voxels, mesh_min_weight=MESH_MIN_WEIGHT,
                      **request_of(c["runs"][i]))


def replica_of(case_, i, want_voxels=True):
    """the replica's result for run i of a case (computed once, shared by the tests: treat it as read-only)"""
    return _replica(case_["name"], i, want_voxels)
