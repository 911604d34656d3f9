"""Hand-built maps for marching cubes (tests/test_cpu_mesh_cases.py, tests/test_gpu_mesh_cases.py): voxel content chosen by the
test instead of left behind by a stream.  Seeded, pure numpy.  Every builder returns (indices (n, 3) int32, layers) as
khronos_amd.checkpoint.pack takes them -- FusionContext.load_map(pack(...)) on the device side, OracleMap.put_blocks(indices,
layers) on the oracle side.

Content common to all maps: every voxel of a map has its own colour, label and last_observed (a vertex that takes its attributes
from the wrong voxel shows), distances are finite with magnitudes in [0.05, 1] * truncation unless a case plants something else,
weights are valid (1 .. 2) unless planted, voxel flags are ACTIVE | SEM_VALID, likelihoods zero, block flags UPDATED |
MESH_UPDATED | HAS_ACTIVE_DATA unless a case says otherwise.

Measured with the oracle on the CPU (tests/test_cpu_mesh_cases.py prints these; only what that module asserts is asserted):
  * all_cases, seed 7: all 256 cube configurations occur among the cubes with eight valid corners;
      vps 16: 29791 such cubes, 91 .. 158 per configuration (mean 116.4);  vps 8: 3375 cubes, 3 .. 25 per configuration (mean 13.2).
  * the 12-frame 320 x 240 stream of test_mesh_and_archival (10 cm voxels, seed 1234), classified before each of its three
      meshings: 75 of the 256 configurations (0 and 255 among them) over 104921 cubes with eight valid corners, 11045 of them
      with a sign change; not one observed voxel with a distance of exactly 0 and none with a weight equal to mesh_min_weight.
      Not asserted anywhere: it is the reason these maps exist.
"""
import numpy as np

VOXEL_SIZE, TRUNCATION, NUM_LABELS = 0.1, 0.3, 3
MESH_MIN_WEIGHT = np.float32(1e-4)            # khr_default_config
CONFIG = dict(voxel_size=VOXEL_SIZE, truncation_distance=TRUNCATION, with_semantics=1, with_tracking=1, num_labels=NUM_LABELS,
              semantic_mode=0)
BLK_UPDATED, BLK_MESH_UPDATED, BLK_HAS_ACTIVE_DATA = 1, 2, 8
ALL_CASES_SEED = 7
ORIGIN = (-2001, 37, -5)
OFFSETS = [(k & 1, (k >> 1) & 1, (k >> 2) & 1) for k in range(8)]   # relation k: bit 0 = +x, bit 1 = +y, bit 2 = +z


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


class Group:
    """a box of blocks as dense voxel arrays indexed [x, y, z] (global voxel coordinates minus the box's first voxel)"""

    def __init__(self, rng, vps, origin, dims=(2, 2, 2), present=None, first_id=0, signs="random"):
        self.vps, self.origin, self.dims = vps, tuple(int(v) for v in origin), dims
        self.present = [o for o in np.ndindex(*dims)] if present is None else [tuple(p) for p in present]
        shape = tuple(d * vps for d in dims)
        n = int(np.prod(shape))
        mag = (rng.uniform(0.05, 1.0, shape) * TRUNCATION).astype(np.float32)
        if signs == "random":
            sgn = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
        elif signs == "parity":
            gx, gy, gz = np.meshgrid(*[np.arange(s) + o * vps for s, o in zip(shape, self.origin)], indexing="ij")
            sgn = np.where(((gx + gy + gz) & 1) == 1, -1.0, 1.0)
        else:
            sgn = np.full(shape, float(signs))
        self.d = (mag * sgn).astype(np.float32)
        self.w = rng.uniform(1.0, 2.0, shape).astype(np.float32)
        ids = (np.arange(n, dtype=np.uint64) + np.uint64(first_id)).reshape(shape)
        self.col = ((ids * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)   # odd multiplier: a bijection mod 2^32
        self.lab = (ids + np.uint64(1)).astype(np.uint32)
        self.obs = np.uint64(1_000_000_000) + ids * np.uint64(1000) + np.uint64(7)
        self.block_flags = {p: BLK_UPDATED | BLK_MESH_UPDATED | BLK_HAS_ACTIVE_DATA for p in self.present}
        self.n_ids = n

    def block_slices(self, p):
        v = self.vps
        return tuple(slice(c * v, (c + 1) * v) for c in p)

    def centre(self, voxel):
        """world position of the centre of the box's voxel (x, y, z), as float64"""
        return (np.asarray(voxel, np.float64) + np.asarray(self.origin, np.float64) * self.vps + 0.5) * VOXEL_SIZE


def to_map(groups):
    """(indices, layers) of the present blocks of `groups`; voxels in linear order x + vps * (y + vps * z)"""
    vps = groups[0].vps
    nv = vps ** 3
    idx, d, w, col, lab, obs, bfl = [], [], [], [], [], [], []
    for g in groups:
        for p in g.present:
            s = g.block_slices(p)
            lin = lambda a: np.ascontiguousarray(a[s].transpose(2, 1, 0)).reshape(nv)
            idx.append([g.origin[i] + p[i] for i in range(3)])
            d.append(lin(g.d)); w.append(lin(g.w)); col.append(lin(g.col)); lab.append(lin(g.lab)); obs.append(lin(g.obs))
            bfl.append(g.block_flags[p])
    n = len(idx)
    assert len({tuple(i) for i in idx}) == n, "groups overlap"
    obs = np.stack(obs).astype(np.uint64)
    layers = {"distance": np.stack(d), "weight": np.stack(w), "color": np.stack(col).view(np.uint8).reshape(n, nv, 4),
              "last_observed": obs, "last_occupied": obs - np.uint64(3), "flags": np.full((n, nv), 9, np.uint8),
              "sem_label": np.stack(lab), "block_flags": np.array(bfl, np.uint8),
              "likelihoods": np.zeros((n, nv, NUM_LABELS), np.float32)}
    assert np.isfinite(layers["distance"]).all()
    for k in ("color", "sem_label", "last_observed"):
        flat = layers[k].reshape(n * nv, -1) if k == "color" else layers[k].reshape(n * nv, 1)
        assert len(np.unique(flat, axis=0)) == n * nv, "attribute %s is not distinct per voxel" % k
    return np.array(idx, np.int32), layers


def config(vps):
    return dict(CONFIG, voxels_per_side=vps)


def all_cases(vps, seed=ALL_CASES_SEED):
    """a 2 x 2 x 2 group far from the origin at a negative index, every voxel's sign independent and uniform"""
    return to_map([Group(np.random.default_rng(seed), vps, ORIGIN)])


def _edge_sites(rng, g, used, n, axis, crossing):
    """n lattice edges (voxel p, p + e_axis) of the box whose two voxels are unused: inside a block, or across the block face"""
    v, out = g.vps, []
    while len(out) < n:
        p = [int(rng.integers(0, s)) for s in g.d.shape]
        p[axis] = v - 1 if crossing else int(rng.choice([c for c in range(2 * v - 1) if c != v - 1]))
        q = list(p)
        q[axis] += 1
        p, q = tuple(p), tuple(q)
        if used[p] or used[q]:
            continue
        used[p] = used[q] = True
        out.append((p, q))
    return out


def edges(vps, seed=ALL_CASES_SEED, eps_pairs=True, with_plan=False):
    """all_cases with special values planted, each kind at least 32 times, inside blocks and on lattice edges across each of the
    three block faces.  plan (with_plan=True): kind -> list of planted sites (box voxel coordinates), and the Group."""
    rng = np.random.default_rng(seed)
    g = Group(rng, vps, ORIGIN)
    prng = np.random.default_rng(seed + 1000)
    used = np.zeros(g.d.shape, bool)
    plan = {k: [] for k in ("zero", "neg_zero", "half", "tiny", "eps_below", "eps_above", "eps_equal", "w_min", "w_below", "w_zero")}
    f32 = np.float32
    per = 6   # per (axis, inside / crossing): 6 x 3 x 2 = 36 >= 32 of each kind

    def sites(n):
        for axis in range(3):
            for crossing in (False, True):
                for i, (p, q) in enumerate(_edge_sites(prng, g, used, n, axis, crossing)):
                    yield axis, crossing, i, p, q

    # d = 0.0 and d = -0.0 at one end of an edge whose other end is negative (neither zero is < 0: the edge is a sign change
    # with t exactly 0 or 1); the zero sits on either side of the face
    for kind, val in (("zero", f32(0.0)), ("neg_zero", f32(-0.0))):
        for axis, crossing, i, p, q in sites(per):
            a, b = (p, q) if i % 2 == 0 else (q, p)
            g.d[a] = val
            g.d[b] = -abs(g.d[b])
            plan[kind].append(a)
    # d1 = -d0: t exactly 0.5, both orientations
    for axis, crossing, i, p, q in sites(per):
        m = abs(g.d[p])
        g.d[p], g.d[q] = (m, -m) if i % 2 == 0 else (-m, m)
        plan["half"].append((p, q))
    # 0 < |d0 - d1| < 1e-6 (the default mesh_degenerate_eps) at a sign change: the natural t would be 3 / 7 or 4 / 7
    for axis, crossing, i, p, q in sites(per):
        g.d[p], g.d[q] = (f32(3e-7), f32(-4e-7)) if i % 2 == 0 else (f32(-4e-7), f32(3e-7))
        plan["tiny"].append((p, q))
    if eps_pairs:  # pairs that straddle mesh_degenerate_eps = 1e-3: |d0 - d1| = 0.9e-3, 1.1e-3 and (where float32 allows) 1e-3 itself
        e = f32(1e-3)
        for axis, crossing, i, p, q in sites(2):
            g.d[p], g.d[q] = f32(4e-4), f32(-5e-4)
            plan["eps_below"].append((p, q))
        for axis, crossing, i, p, q in sites(2):
            g.d[p], g.d[q] = f32(6e-4), f32(-5e-4)
            plan["eps_above"].append((p, q))
        d0 = f32(e * f32(0.75))
        d1 = f32(d0 - e)
        if f32(d0 - d1) == e and d1 < 0:
            for axis, crossing, i, p, q in sites(1):
                g.d[p], g.d[q] = d0, d1
                plan["eps_equal"].append((p, q))
    # corner weights: exactly mesh_min_weight (observed), the float below it and 0 -- the pool's initial value -- (unobserved);
    # on either side of the faces as well
    for kind, val in (("w_min", MESH_MIN_WEIGHT), ("w_below", np.nextafter(MESH_MIN_WEIGHT, f32(0))), ("w_zero", f32(0))):
        for axis, crossing, i, p, q in sites(per):
            a = p if i % 2 == 0 else q
            g.w[a] = val
            plan[kind].append(a)
    for k in ("zero", "neg_zero", "half", "tiny", "w_min", "w_below", "w_zero"):
        assert len(plan[k]) >= 32, (k, len(plan[k]))
    out = to_map([g])
    return out + (plan, g) if with_plan else out


def _relation_ok(origin, world):
    """every relation 1..7 is remote for some block of the complete 2 x 2 x 2 group at `origin`"""
    blocks = {tuple(origin[i] + o[i] for i in range(3)) for o in OFFSETS}
    for k in range(1, 8):
        hit = False
        for b in blocks:
            nb = tuple(b[i] + OFFSETS[k][i] for i in range(3))
            hit = hit or (nb in blocks and owner_of(nb, world) != owner_of(b, world))
        if not hit:
            return False
    return True


def relations_origins():
    """origins of the eight copies: copy k = 1..7 at a fixed, well separated place; the complete copy (index 0 of the result)
    at the first place of a fixed scan where every relation 1..7 is remote for some block for world = 2 and world = 3"""
    origins = [None] + [(-2001 + 10 * k, 37 - 7 * k, -5 + 5 * k) for k in range(1, 8)]
    for t in range(1, 4000):
        o = (300 + 3 * t, -40 - 5 * (t % 17), 11 + 4 * (t % 29))
        if all(_relation_ok(o, w) for w in (2, 3)):
            origins[0] = o
            return origins
    raise AssertionError("no origin makes every relation remote")


def relations(seed=11, with_plan=False):
    """seven copies of the 2 x 2 x 2 group, copy k without the block at relation k of the group's first block, and a complete
    eighth.  vps 16.  plan: list of (Group, missing offset or None)."""
    rng = np.random.default_rng(seed)
    origins = relations_origins()
    groups, first = [], 0
    for k in range(8):
        present = [o for o in OFFSETS if k == 0 or o != OFFSETS[k]]
        g = Group(rng, 16, origins[k], present=present, first_id=first)
        first += g.n_ids
        groups.append(g)
    out = to_map(groups)
    return out + ([(g, None if k == 0 else OFFSETS[k]) for k, g in enumerate(groups)],) if with_plan else out


def shortcut(vps=16, seed=13, with_plan=False):
    """blocks that never hold a negative distance beside blocks that do, and blocks with exactly one negative voxel.
    plan: name -> (Group, expected vertex count or None)"""
    rng = np.random.default_rng(seed)
    first, groups, plan = 0, [], {}

    def add(name, origin, expect=None, **kw):
        nonlocal first
        g = Group(rng, vps, origin, first_id=first, **kw)
        first += g.n_ids
        groups.append(g)
        plan[name] = (g, expect)
        return g

    # the first block all positive, its +x, +y, +z, edge and corner neighbours all negative: only the first block's outermost
    # cubes cross a sign change, and that block has no negative distance of its own
    g = add("positive_first", (40, -3, 9), signs=-1.0)
    g.d[g.block_slices((0, 0, 0))] = np.abs(g.d[g.block_slices((0, 0, 0))])
    # the mirror image: the last block all positive; the other blocks' outermost cubes read it
    g = add("positive_last", (-60, 5, 2), signs=-1.0)
    g.d[g.block_slices((1, 1, 1))] = np.abs(g.d[g.block_slices((1, 1, 1))])
    add("lonely_positive", (7, 70, -30), expect=0, dims=(1, 1, 1), signs=1.0)
    add("all_negative", (-9, -80, 14), expect=0, signs=-1.0)
    # one negative voxel at linear index 0 / NV - 1: one cube of configuration 1 / 64 each (the cubes beyond need absent blocks)
    g = add("first_voxel", (100, 100, 100), expect=3, dims=(1, 1, 1), signs=1.0)
    g.d[0, 0, 0] = -g.d[0, 0, 0]
    g = add("last_voxel", (-100, -100, -100), expect=3, dims=(1, 1, 1), signs=1.0)
    g.d[vps - 1, vps - 1, vps - 1] = -g.d[vps - 1, vps - 1, vps - 1]
    out = to_map(groups)
    return out + (plan,) if with_plan else out


def dense(vps, seed=17, flagged=None):
    """sign of (x + y + z) & 1 over global voxel coordinates, all weights valid: every cube with eight corners present is
    configuration 0x5A or 0xA5 (four isolated corners, four triangles).  flagged: block offsets that keep MESH_UPDATED (default all)"""
    g = Group(np.random.default_rng(seed), vps, ORIGIN, signs="parity")
    if flagged is not None:
        for p in g.present:
            if p not in [tuple(f) for f in flagged]:
                g.block_flags[p] &= ~BLK_MESH_UPDATED
    return to_map([g])


def dense_vertices(vps, blocks=None):
    """12 x (number of cubes with all eight corners present), counted from the block set alone; blocks: offsets whose cubes count"""
    blocks = OFFSETS if blocks is None else [tuple(b) for b in blocks]
    # a cube of block b along one axis: vps - 1 cubes inside, one more if the + neighbour exists (b = 0 in a group of 2)
    return 12 * sum(int(np.prod([vps if c == 0 else vps - 1 for c in b])) for b in blocks)


DENSE_HALF = [(0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)]


def partial(vps=16, seed=ALL_CASES_SEED, with_plan=False):
    """all_cases with MESH_UPDATED on a seeded half of its blocks only, and a ninth, isolated all-positive block that is flagged too
    and ends up with zero triangles.  plan: the flagged block indices"""
    rng = np.random.default_rng(seed)
    g = Group(rng, vps, ORIGIN)
    pick = np.random.default_rng(seed + 1).permutation(8)[:4]
    flagged = [OFFSETS[k] for k in pick]
    for p in g.present:
        if p not in flagged:
            g.block_flags[p] &= ~BLK_MESH_UPDATED
    lone = Group(rng, vps, (ORIGIN[0] + 50, ORIGIN[1], ORIGIN[2]), dims=(1, 1, 1), first_id=g.n_ids, signs=1.0)
    out = to_map([g, lone])
    fl = [tuple(ORIGIN[i] + p[i] for i in range(3)) for p in flagged] + [lone.origin]
    return out + (fl,) if with_plan else out


CUBE_CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]   # corner k sets bit k


def cube_configs(indices, layers, vps, min_weight=MESH_MIN_WEIGHT):
    """per block, the configuration number (bit k: corner k's distance < 0) of every cube and whether its eight corners are present
    and observed (weight >= min_weight): ASSUMPTIONS.md A.5 restated in numpy, without the triangle table.
    Returns (configs (n, vps, vps, vps) uint8 indexed [x, y, z], valid (same shape) bool)."""
    idx = [tuple(int(v) for v in b) for b in np.asarray(indices).reshape(-1, 3)]
    slot = {b: i for i, b in enumerate(idx)}
    n, T = len(idx), vps + 1
    grid = lambda a: a.reshape(vps, vps, vps).transpose(2, 1, 0)   # linear x + vps * (y + vps * z) -> [x, y, z]
    cfgs, valid = np.zeros((n, vps, vps, vps), np.uint8), np.zeros((n, vps, vps, vps), bool)
    for i, b in enumerate(idx):
        neg, ok = np.zeros((T, T, T), bool), np.zeros((T, T, T), bool)
        for o in OFFSETS:
            j = slot.get(tuple(b[a] + o[a] for a in range(3)))
            if j is None:
                continue
            dst = tuple(slice(vps, T) if o[a] else slice(0, vps) for a in range(3))
            src = tuple(slice(0, 1) if o[a] else slice(0, vps) for a in range(3))
            neg[dst] = grid(layers["distance"][j])[src] < 0
            ok[dst] = grid(layers["weight"][j])[src] >= min_weight
        c, v = np.zeros((vps, vps, vps), np.uint8), np.ones((vps, vps, vps), bool)
        for k, (dx, dy, dz) in enumerate(CUBE_CORNERS):
            s = (slice(dx, dx + vps), slice(dy, dy + vps), slice(dz, dz + vps))
            c |= (neg[s].astype(np.uint8) << k)
            v &= ok[s]
        cfgs[i], valid[i] = c, v
    return cfgs, valid
