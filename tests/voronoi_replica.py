"""numpy restatement of khr_voronoi_field (ASSUMPTIONS.md A.20) over a query_replica.QueryBlocks block set.  The cell classes are
distance_replica.classify's.  The site transform exists in two forms that share nothing but the definition: `brute` (every cell
against every site, the first minimiser in (z, y, x) order) and `windowed` (three passes of the R-window minimum over the keys
value << 32 | site).  `line_walk` is the device's walk along one line with either stop rule.  The separation predicate, the basis
rule and the list follow; tests/test_cpu_voronoi_replica.py holds the forms to each other, the GPU tests use `windowed`."""
import numpy as np

import distance_replica as dr

f32 = np.float32
FAR = dr.FAR
NO_SITE = 0xFFFFFFFF
FAR_KEY = (FAR << 32) | NO_SITE
L1, ANGLE, L1_THEN_ANGLE, MAX_BASIS = 0, 1, 2, 4
DENSE = ("distance", "d2", "status", "site", "basis")
LIST = ("cells", "cell_distance", "cell_basis", "cell_sites")
STATS = dr.STATS + ("n_eligible", "n_basis2", "n_basis3", "n_basis4", "n_listed")
# the 26 neighbours: dz outer, dy middle, dx inner
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def brute(sites):
    """(least squared distance int64, linear index of the least such site in (z, y, x) order) per cell of `sites` (bool [z, y, x]);
    (FAR, NO_SITE) without sites"""
    nz, ny, nx = sites.shape
    s = np.argwhere(sites).astype(np.int64)   # ascending (z, y, x) = ascending linear index
    if len(s) == 0:
        return np.full(sites.shape, FAR, np.int64), np.full(sites.shape, NO_SITE, np.int64)
    lin = s[:, 2] + nx * (s[:, 1] + ny * s[:, 0])
    c = np.argwhere(np.ones(sites.shape, bool)).astype(np.int64)
    best = np.full(len(c), FAR, np.int64)
    arg = np.full(len(c), NO_SITE, np.int64)
    for k in range(0, len(s), 256):
        d = ((c[:, None, :] - s[None, k:k + 256, :]) ** 2).sum(axis=2)
        j = d.argmin(axis=1)                   # the first minimiser of the chunk
        v = d[np.arange(len(c)), j]
        take = v < best                        # (strictly: an earlier chunk holds the smaller indices)
        best, arg = np.where(take, v, best), np.where(take, lin[k + j], arg)
    return best.reshape(sites.shape), arg.reshape(sites.shape)


def windowed(sites, R):
    """(value, site) after three passes of min over |i - j| <= R of key(j) + ((i - j)^2 << 32) along x, y, z, a key whose value
    reaches FAR reset to FAR_KEY.  Equals `brute` wherever that is <= R^2; the value exceeds R^2 everywhere else"""
    lin = np.arange(sites.size, dtype=np.int64).reshape(sites.shape)
    g = np.where(sites, lin, FAR_KEY).astype(np.int64)
    for axis in (2, 1, 0):
        n = g.shape[axis]
        f = g
        out = f.copy()
        for k in range(1, min(R, n - 1) + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - k), slice(k, n)
            lo, hi = tuple(lo), tuple(hi)
            add = np.int64(k * k) << 32
            out[hi] = np.minimum(out[hi], f[lo] + add)   # j = i - k
            out[lo] = np.minimum(out[lo], f[hi] + add)   # j = i + k
        g = np.where((out >> 32) >= FAR, FAR_KEY, out)
    return g >> 32, g & NO_SITE


def line_walk(keys, R, strict=True):
    """the device's walk along one line of keys (python ints): outwards from each position until k^2 exceeds the best value
    (strict) -- or, the distance field's rule that is WRONG for sites, until k^2 reaches it"""
    n = len(keys)
    out = []
    for i in range(n):
        best = keys[i]
        for k in range(1, min(R, n - 1) + 1):
            kk = k * k
            if (kk > (best >> 32)) if strict else (kk >= (best >> 32)):
                break
            for j in (i - k, i + k):
                if 0 <= j < n:
                    best = min(best, keys[j] + (kk << 32))
        out.append(FAR_KEY if (best >> 32) >= FAR else best)
    return out


def separated(c, p, q, mode, l1_sep, cos_sep):
    """are the sites p, q separated as seen from cell c: integer triples, or arrays of them (..., 3)"""
    c, p, q = (np.asarray(v, np.int64) for v in (c, p, q))
    same = (p == q).all(axis=-1)
    by_l1 = np.abs(p - q).sum(axis=-1) >= int(l1_sep)
    a, b = p - c, q - c
    dot, aa, bb = (a * b).sum(axis=-1), (a * a).sum(axis=-1), (b * b).sum(axis=-1)
    by_angle = dot.astype(np.float64) <= np.float64(f32(cos_sep)) * np.sqrt(aa.astype(np.float64) * bb.astype(np.float64))
    r = by_l1 if mode == L1 else (by_angle if mode == ANGLE else (by_l1 | by_angle))
    return r & ~same


def basis_rule(has, eligible, site, mode, l1_sep, cos_sep):
    """(basis uint8 [z, y, x], B int64 [z, y, x, MAX_BASIS, 3] box-local (x, y, z), unused entries zero).  has / eligible: bool
    [z, y, x]; site: the linear index where `has`"""
    nz, ny, nx = has.shape

    def xyz(l):
        return np.stack([l % nx, (l // nx) % ny, l // (nx * ny)], axis=-1)

    cz, cy, cx = (v.ravel() for v in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"))
    idx = np.flatnonzero(eligible.ravel())
    c = np.stack([cx[idx], cy[idx], cz[idx]], axis=-1).astype(np.int64)
    B = np.zeros((len(idx), MAX_BASIS, 3), np.int64)
    B[:, 0] = xyz(site.ravel()[idx].astype(np.int64))
    nb = np.ones(len(idx), np.int64)
    for dx, dy, dz in OFFSETS:
        X, Y, Z = c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz
        ok = (X >= 0) & (X < nx) & (Y >= 0) & (Y < ny) & (Z >= 0) & (Z < nz)
        at = np.where(ok, X + nx * (Y + ny * Z), 0)
        ok &= has.ravel()[at] & (nb < MAX_BASIS)
        q = xyz(np.where(ok, site.ravel()[at], 0).astype(np.int64))
        for j in range(MAX_BASIS):
            ok &= (j >= nb) | separated(c, B[:, j], q, mode, l1_sep, cos_sep)
        rows = np.flatnonzero(ok)
        B[rows, nb[rows]] = q[rows]
        nb[rows] += 1
    basis = np.zeros(has.size, np.uint8)
    basis[idx] = nb
    full = np.zeros((has.size, MAX_BASIS, 3), np.int64)
    full[idx] = B
    return basis.reshape(has.shape), full.reshape(has.shape + (MAX_BASIS, 3))


def field_of(in_set, observed, obstacle, origin, cell, R, max_distance, min_distance=0.0, mode=L1_THEN_ANGLE, parent_l1_separation=20,
             parent_cos_angle_separation=0.2, min_basis=2, form="windowed"):
    """the outputs of FusionContext.voronoi_field from the cell classes (bool [z, y, x]); cell: the float32 cell size"""
    nz, ny, nx = in_set.shape
    value, site = windowed(in_set, R) if form == "windowed" else brute(in_set)
    in_range = value <= R * R
    has = in_range & ~in_set
    mag = np.where(in_range, value, FAR)
    dist = np.where(in_range, f32(cell) * np.sqrt(np.where(in_range, mag, 0).astype(f32)), f32(max_distance)).astype(f32)
    eligible = has & (dist >= f32(min_distance))
    basis, B = basis_rule(has, eligible, site, mode, parent_l1_separation, parent_cos_angle_separation)
    out = {"distance": dist, "d2": mag.astype(np.int32),
           "status": (observed * dr.DF_OBSERVED + obstacle * dr.DF_OBSTACLE + in_range * dr.DF_IN_RANGE).astype(np.uint8),
           "site": np.where(has, site, -1).astype(np.int32), "basis": basis}
    mb = 2 if min_basis == 0 else min_basis
    lin = np.flatnonzero(basis.ravel() >= mb)
    local = np.stack([lin % nx, (lin // nx) % ny, lin // (nx * ny)], axis=-1)
    o = np.asarray(origin, np.int64)
    nb = basis.ravel()[lin]
    used = np.arange(MAX_BASIS)[None, :] < nb[:, None]
    out["cells"] = (local + o).astype(np.int32).reshape(-1, 3)
    out["cell_distance"] = dist.ravel()[lin]
    out["cell_basis"] = nb.astype(np.uint8)
    out["cell_sites"] = np.where(used[:, :, None], B.reshape(-1, MAX_BASIS, 3)[lin] + o, 0).astype(np.int32)
    free = observed & ~obstacle
    out["stats"] = {"n_observed": int(observed.sum()), "n_obstacle": int(obstacle.sum()), "n_free": int(free.sum()), "n_in_range": int(in_range.sum()),
                    "n_eligible": int(eligible.sum()), "n_basis2": int((basis == 2).sum()), "n_basis3": int((basis == 3).sum()),
                    "n_basis4": int((basis == 4).sum()), "n_listed": len(lin)}
    out["cell_size"] = float(cell)
    return out


def voronoi_field(blocks, voxel_size, origin, dims, ratio=1, max_distance=1.0, min_weight=1e-4, surface_distance=0.0, unknown_is_obstacle=False,
                  classes=None, **kw):
    """the outputs of FusionContext.voronoi_field over a block set.  classes: what distance_replica.classify returned for the same
    box, ratio, min_weight and surface_distance; further keywords as field_of"""
    observed, obstacle = classes if classes is not None else dr.classify(blocks, origin, dims, ratio, min_weight, surface_distance)
    in_set = obstacle | (~observed if unknown_is_obstacle else np.zeros_like(observed))
    cell, R = dr.reach(voxel_size, ratio, max_distance)
    return field_of(in_set, observed, obstacle, origin, cell, R, max_distance, **kw)
