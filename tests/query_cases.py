"""The point sets of the khr_query_points tests (tests/test_cpu_query_points.py fixes them and proves them non-vacuous on the replica
alone, tests/test_gpu_query_points.py compares the kernel on the same sets): built from a map's BlockSet and the stream's last
frame, deterministic."""
import numpy as np

import query_replica as qr

f32 = np.float32
EDGE_F = (f32(0.37), f32(0.62), f32(0.81))  # the fractions of the lattice's off-centre points, per axis


def exact_point(g, vs_inv):
    """a float32 coordinate p with p * vs_inv - 0.5 == g exactly (float32 arithmetic), or None: the candidates are the float
    nearest (g + 0.5) / vs_inv and its neighbours"""
    g = f32(g)
    p = f32((float(g) + 0.5) / float(vs_inv))
    cands = [p]
    lo = hi = p
    for _ in range(4):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        cands += [lo, hi]
    for c in cands:
        if f32(f32(c) * vs_inv) - f32(0.5) == g:
            return f32(c)
    return None


def surface_points(frame, sensor, truncation_distance):
    """the frame's valid depth pixels back-projected with its pose, at 0, -half and +half the truncation distance along the ray
    (in front of the surface, then behind it): three (n, 3) float32 arrays in pixel order, and the flat pixel indices"""
    depth = np.asarray(frame["depth"], np.float64)
    H, W = depth.shape
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sel = np.flatnonzero((depth > 0).ravel())
    z = depth.ravel()[sel]
    cam = np.stack([(uu.ravel()[sel] - sensor.cx) / sensor.fx * z, (vv.ravel()[sel] - sensor.cy) / sensor.fy * z, z], axis=1)
    rng = np.linalg.norm(cam, axis=1, keepdims=True)
    T = np.asarray(frame["pose"], np.float64).reshape(4, 4)
    out = []
    for off in (0.0, -0.5 * truncation_distance, 0.5 * truncation_distance):
        p = cam * (1.0 + off / rng)
        out.append((p @ T[:3, :3].T + T[:3, 3]).astype(f32))
    return out, sel


def box_points(blocks, voxel_size, n=4096, seed=77):
    """seeded uniform points in the bounding box of the allocated blocks inflated by one block"""
    bs = blocks.vps * float(voxel_size)
    idx = unpack(blocks.keys)
    lo, hi = (idx.min(axis=0) - 1) * bs, (idx.max(axis=0) + 2) * bs
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(f32)


def unpack(keys):
    k = np.asarray(keys, np.int64)
    return np.stack([(k & 0x1FFFFF) - (1 << 20), ((k >> 21) & 0x1FFFFF) - (1 << 20), ((k >> 42) & 0x1FFFFF) - (1 << 20)], axis=1)


def bad_points():
    return np.array([[np.nan, 0, 0], [0, np.nan, 1], [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, np.inf], [1e12, 0, 0], [0, 0, -1e12],
                     [500.0, -500.0, 300.0]], f32)


def pick_blocks(blocks, min_weight):
    """the lattice's two blocks: among the blocks with the most negative index components the one with the most observed voxels,
    and the same among the blocks with none (ties: the lowest key)"""
    idx = unpack(blocks.keys)
    seen = (blocks.weight[:len(idx)] >= f32(min_weight)).sum(axis=1)
    neg = (idx < 0).sum(axis=1)
    assert neg.max() >= 1 and neg.min() == 0
    a = int(np.argmax(np.where(neg == neg.max(), seen, -1)))
    b = int(np.argmax(np.where(neg == 0, seen, -1)))
    return idx[a], idx[b]


def lattice_points(blocks, voxel_size, min_weight):
    """hand-placed points around two allocated blocks: dict case name -> (n, 3) float32.
    centres: exact voxel centres (f = 0) at local indices 0, 1, vps-2, vps-1 on one axis and in the middle of the block;
    edge1 / edge2 / edge3: i0's local index in {0, 1, vps-2, vps-1} on one, two, three axes (the others mid-block);
    cut: the distance is valid while a shifted sample reaches into a block that is not allocated;
    hole: inside an allocated block, with an unobserved voxel among the taps."""
    v = blocks.vps
    vs = f32(voxel_size)
    vs_inv = f32(1) / vs
    edge, mid = (0, 1, v - 2, v - 1), v // 2
    cases = {"centres": [], "edge1": [], "edge2": [], "edge3": []}

    def centre(j):
        p = [exact_point(ja, vs_inv) for ja in j]
        return None if any(pa is None for pa in p) else p

    def off_centre(j):
        return [f32((float(ja) + 0.5 + float(fa)) * float(vs)) for ja, fa in zip(j, EDGE_F)]

    for blk in pick_blocks(blocks, min_weight):
        base = blk.astype(np.int64) * v
        for a in range(3):
            for l in edge:
                loc = [mid, mid, mid]
                loc[a] = l
                cases["edge1"].append(off_centre(base + loc))
                p = centre(base + loc)
                if p is not None:
                    cases["centres"].append(p)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    p = centre(base + [mid + dx, mid + dy, mid + dz])
                    if p is not None:
                        cases["centres"].append(p)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            for la in edge:
                for lb in edge:
                    loc = [mid, mid, mid]
                    loc[a], loc[b] = la, lb
                    cases["edge2"].append(off_centre(base + loc))
        for lx in edge:
            for ly in edge:
                for lz in edge:
                    cases["edge3"].append(off_centre(base + [lx, ly, lz]))
    # cut: candidates two voxels inside every face of an allocated block whose neighbour across the face is missing
    idx = unpack(blocks.keys)
    have = set(int(k) for k in blocks.keys)
    cand = []
    inner = range(2, v - 2, 3)
    for bi in idx:
        for a in range(3):
            for sgn in (-1, 1):
                nb = bi.copy()
                nb[a] += sgn
                if int(blocks.pack(*nb)) in have:
                    continue
                for s in inner:
                    for t in inner:
                        loc = [s, t]
                        loc.insert(a, 0 if sgn < 0 else v - 2)
                        cand.append(off_centre(bi.astype(np.int64) * v + loc))
    cand = np.array(cand, f32).reshape(-1, 3)
    st = qr.query(blocks, cand, voxel_size, min_weight)["status"]
    cases["cut"] = cand[(st & (qr.QP_VALUE | qr.QP_GRADIENT)) == qr.QP_VALUE][:16]
    # hole: unobserved voxels of allocated blocks (not on a block face, so that every tap lies in the block)
    rows, lins = np.nonzero(blocks.weight[:len(idx)] < f32(min_weight))
    loc = np.stack([lins % v, (lins // v) % v, lins // (v * v)], axis=1)
    keep = np.flatnonzero(((loc >= 2) & (loc <= v - 3)).all(axis=1))
    keep = keep[:: max(1, len(keep) // 16)][:16]
    cases["hole"] = np.array([off_centre(idx[rows[k]].astype(np.int64) * v + loc[k]) for k in keep], f32).reshape(-1, 3)
    return {k: np.array(p, f32).reshape(-1, 3) for k, p in cases.items()}


def all_sets(blocks, frame, sensor, voxel_size, truncation_distance, min_weight):
    """name -> (n, 3) float32: surface, box, lattice, bad, and `mixed`, their concatenation shuffled with a fixed seed"""
    (at, front, behind), _ = surface_points(frame, sensor, truncation_distance)
    sets = {"surface": np.concatenate([at, front, behind]), "box": box_points(blocks, voxel_size),
            "lattice": np.concatenate(list(lattice_points(blocks, voxel_size, min_weight).values())), "bad": bad_points()}
    mixed = np.concatenate(list(sets.values()))
    sets["mixed"] = mixed[np.random.default_rng(5).permutation(len(mixed))]
    return sets
