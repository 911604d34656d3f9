"""numpy restatement of khr_distance_field (ASSUMPTIONS.md A.15) over a query_replica.QueryBlocks block set.  The cell classes are
read voxel by voxel through BlockSet.lookup; the transform exists in two forms that share nothing but the definition: `brute`
(every cell against every site, int64) and `windowed` (three 1-D passes g(i) = min over |i - j| <= R of f(j) + (i - j)^2, values
capped at FAR).  tests/test_cpu_distance_field.py holds the two to each other; the GPU tests use `windowed`."""
import numpy as np

f32 = np.float32
DF_OBSERVED, DF_OBSTACLE, DF_IN_RANGE = 1, 2, 4
FAR = 1 << 30
FIELDS = ("distance", "d2", "status")
STATS = ("n_observed", "n_obstacle", "n_free", "n_in_range")


def classify(blocks, origin, dims, ratio, min_weight, surface_distance):
    """(observed, obstacle) bool arrays indexed [z, y, x] over the box"""
    nx, ny, nz = (int(d) for d in dims)
    cz, cy, cx = np.meshgrid(np.arange(nz) + int(origin[2]), np.arange(ny) + int(origin[1]), np.arange(nx) + int(origin[0]), indexing="ij")
    observed = np.zeros((nz, ny, nx), bool)
    value = np.full((nz, ny, nx), np.inf, f32)
    for dz in range(ratio):
        for dy in range(ratio):
            for dx in range(ratio):
                row, found, lin = blocks.lookup((cx * ratio + dx).ravel().astype(np.int64), (cy * ratio + dy).ravel().astype(np.int64),
                                                (cz * ratio + dz).ravel().astype(np.int64))
                obs = (found & (blocks.weight[row, lin] >= f32(min_weight))).reshape(nz, ny, nx)
                d = blocks.distance[row, lin].reshape(nz, ny, nx)
                value = np.where(obs, np.minimum(value, d), value)
                observed |= obs
    obstacle = observed & (value <= f32(surface_distance))
    return observed, obstacle


def reach(voxel_size, ratio, max_distance):
    """(cell_size float32, R)"""
    cell = f32(voxel_size) * f32(ratio)
    return cell, int(np.floor(f32(max_distance) / cell))


def brute(sites, targets=None):
    """least squared distance (int64) from every cell of the box to a cell of `sites` (bool [z, y, x]); FAR without sites"""
    out = np.full(sites.shape, FAR, np.int64)
    s = np.argwhere(sites).astype(np.int64)
    if len(s) == 0:
        return out
    c = np.argwhere(np.ones(sites.shape, bool)).astype(np.int64)
    best = np.full(len(c), FAR, np.int64)
    for k in range(0, len(s), 256):
        d = ((c[:, None, :] - s[None, k:k + 256, :]) ** 2).sum(axis=2).min(axis=1)
        best = np.minimum(best, d)
    return best.reshape(sites.shape)


def windowed(sites, R):
    """three passes of the R-window min-plus along x, y, z; values capped at FAR.  Equals `brute` wherever that is <= R^2 and
    exceeds R^2 everywhere else"""
    g = np.where(sites, 0, FAR).astype(np.int64)
    for axis in (2, 1, 0):
        n = g.shape[axis]
        f = g
        out = f.copy()
        for k in range(1, min(R, n - 1) + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - k), slice(k, n)
            lo, hi = tuple(lo), tuple(hi)
            out[hi] = np.minimum(out[hi], f[lo] + k * k)   # j = i - k
            out[lo] = np.minimum(out[lo], f[hi] + k * k)   # j = i + k
        g = np.minimum(out, FAR)
    return g


def distance_field(blocks, voxel_size, origin, dims, ratio=1, max_distance=1.0, min_weight=1e-4, surface_distance=0.0,
                   unknown_is_obstacle=False, positive_only=False, form="windowed", classes=None):
    """the outputs of FusionContext.distance_field: arrays shaped (nz, ny, nx) plus the four counters.  classes: what `classify`
    returned for the same box, ratio, min_weight and surface_distance (a caller that varies only the other switches computes it once)"""
    observed, obstacle = classes if classes is not None else classify(blocks, origin, dims, ratio, min_weight, surface_distance)
    free = observed & ~obstacle
    in_set = obstacle | (~observed if unknown_is_obstacle else np.zeros_like(observed))
    cell, R = reach(voxel_size, ratio, max_distance)
    xf = (lambda s: windowed(s, R)) if form == "windowed" else brute
    mag = xf(in_set)
    neg = np.zeros_like(in_set)
    if positive_only:
        mag = np.where(in_set, 0, mag)
    else:
        mag = np.where(in_set, xf(free), mag)
        neg = in_set
    in_range = mag <= R * R
    mag = np.where(in_range, mag, FAR)
    with np.errstate(invalid="ignore"):
        dist = np.where(in_range, cell * np.sqrt(np.where(in_range, mag, 0).astype(f32)), f32(max_distance)).astype(f32)
    out = {"distance": np.where(neg, -dist, dist).astype(f32), "d2": np.where(neg, -mag, mag).astype(np.int32),
           "status": (observed * DF_OBSERVED + obstacle * DF_OBSTACLE + in_range * DF_IN_RANGE).astype(np.uint8)}
    out["stats"] = {"n_observed": int(observed.sum()), "n_obstacle": int(obstacle.sum()), "n_free": int(free.sum()), "n_in_range": int(in_range.sum())}
    out["cell_size"] = float(cell)
    return out
