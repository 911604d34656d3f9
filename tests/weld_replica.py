"""A numpy restatement of khr_weld_mesh (ASSUMPTIONS.md A.16): the triangle soup as khr_download_mesh hands it out -> the indexed
mesh, one vertex per cell of a grid of `r` metres.  weld() is the vectorised form the device is compared with; weld_sequential() is
the plain first-come walk it is checked against on the CPU (tests/test_cpu_weld_replica.py)."""
import numpy as np

FIELDS = ("points", "colors", "labels", "first_seen", "stamps")
LIMIT = 1 << 20   # cell indices lie in [-LIMIT, LIMIT): the project's 3 x 21-bit packing


class OutOfRange(ValueError):
    """a vertex that is not finite, or whose cell index does not fit the key"""


def cells(points, r):
    """floorf(p / r) per axis with the IEEE float32 quotient, as float32 (n, 3); OutOfRange as the device reports it"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = np.floor(p / np.float32(r))
    assert c.dtype == np.float32
    ok = np.isfinite(p) & (c >= -LIMIT) & (c < LIMIT)   # (a NaN or an infinite quotient fails the comparisons)
    if not ok.all():
        raise OutOfRange("%d vertices outside the cell range at resolution %g" % (int((~ok).any(axis=1).sum()), r))
    return c


def keys(points, r):
    """packKey of khr_device.h: biased x | y << 21 | z << 42"""
    c = cells(points, r).astype(np.int64) + LIMIT
    return (c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)).astype(np.uint64)


def _finish(soup, rep_of):
    """rep_of[i] = soup index of the representative of i's cell -> every output"""
    n = len(rep_of)
    reps = np.flatnonzero(rep_of == np.arange(n))          # ascending soup index
    s2v = np.searchsorted(reps, rep_of).astype(np.uint32)
    tri = s2v.reshape(-1, 3)
    keep = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    out = {k: np.ascontiguousarray(soup[k][reps]) for k in FIELDS}
    out["faces"] = np.ascontiguousarray(tri[keep])
    out["soup_to_vertex"] = s2v
    out["stats"] = {"n_soup_vertices": n, "n_vertices": len(reps), "n_faces": int(keep.sum()), "n_degenerate_faces": int((~keep).sum())}
    return out


def weld(soup, r):
    """soup: dict of FIELDS arrays (3 vertices per face, in soup order); r: resolution in metres"""
    n = len(soup["points"])
    assert n % 3 == 0
    if n == 0:
        return _finish(soup, np.zeros(0, np.int64))
    k = keys(soup["points"], r)
    _, first, inv = np.unique(k, return_index=True, return_inverse=True)   # first = the least index of each key
    return _finish(soup, first[inv.reshape(-1)].astype(np.int64))


def sphere(vps, origin=(-3, 2, -1), seed=23):
    """a smooth surface for the weld's conditions: 2 x 2 x 2 blocks whose distances are those of a sphere (radius a third of the box,
    centre off the lattice so that no distance is exactly 0), clipped to the truncation distance -> (indices, layers) like mesh_cases"""
    import mesh_cases as mc
    g = mc.Group(np.random.default_rng(seed), vps, origin, signs=1.0)
    ax = [np.arange(2 * vps, dtype=np.float64)] * 3
    x, y, z = np.meshgrid(*ax, indexing="ij")
    centre = vps - 0.5 + np.array([0.13, 0.29, 0.41])
    dist = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - 2 * vps / 3.0
    g.d = np.clip(dist * mc.VOXEL_SIZE, -mc.TRUNCATION, mc.TRUNCATION).astype(np.float32)
    return mc.to_map([g])


def weld_sequential(soup, r):
    """the same by a first-come walk over the soup, one dictionary of cells (N-version check of weld())"""
    c = cells(soup["points"], r)
    index, reps, s2v = {}, [], []
    for i, cell in enumerate(map(tuple, c.astype(np.int64).tolist())):
        j = index.get(cell)
        if j is None:
            j = index[cell] = len(reps)
            reps.append(i)
        s2v.append(j)
    faces = [t for t in zip(s2v[0::3], s2v[1::3], s2v[2::3]) if len(set(t)) == 3]
    reps = np.array(reps, np.int64)
    out = {k: np.ascontiguousarray(soup[k][reps]) for k in FIELDS}
    out["faces"] = np.array(faces, np.uint32).reshape(-1, 3)
    out["soup_to_vertex"] = np.array(s2v, np.uint32)
    out["stats"] = {"n_soup_vertices": len(s2v), "n_vertices": len(reps), "n_faces": len(faces), "n_degenerate_faces": len(s2v) // 3 - len(faces)}
    return out
