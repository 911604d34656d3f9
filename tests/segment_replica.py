"""Plain restatement of khr_segment_map (ASSUMPTIONS.md A.19) on (indices, layers) as khronos_amd.checkpoint.unpack gives them:
the members by numpy, block after block in (x, y, z) order; the components by a breadth-first flood fill over a dictionary of the
member voxels (deliberately no union-find: the kernels use one).  Needs no device and no library."""
from collections import deque

import numpy as np

f32 = np.float32
STATS = ("n_blocks", "n_member_voxels", "n_components_all", "n_too_small", "n_too_large", "n_components", "n_voxels")
COMPONENT_FIELDS = (("label", np.int32, ()), ("n_voxels", np.uint64, ()), ("bbox_min", np.int32, (3,)), ("bbox_max", np.int32, (3,)),
                    ("sum", np.int64, (3,)), ("representative", np.int32, (3,)), ("last_observed_max", np.uint64, ()), ("first", np.uint64, ()))
VOXEL_FIELDS = (("voxels", np.int32, (3,)), ("voxel_component", np.uint32, ()))
VOX_ACTIVE, VOX_EVER_FREE, VOX_PUBLIC = 1, 2, 0x0f
# the forward half of the 26-neighbourhood: 3 faces, 6 edges, 4 corners; with their negatives the 6-, 18- and 26-neighbourhoods
FACES = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
EDGES = [(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]
CORNERS = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]
_BIAS, _BITS = 1 << 25, 27  # a global voxel index lies in [-2^24, 2^24)


def offsets(connectivity):
    half = {6: FACES, 18: FACES + EDGES, 26: FACES + EDGES + CORNERS}[connectivity]
    return half + [(-x, -y, -z) for x, y, z in half]


def _key(x, y, z):
    return ((x + _BIAS) << (2 * _BITS)) | ((y + _BIAS) << _BITS) | (z + _BIAS)


def members(config, idx, layers, min_weight=0.0, surface_distance=0.0, labels=None, flags_require=0, flags_exclude=0, mesh_min_weight=1e-4):
    """the member voxels in A.19's order: (global voxel indices (n, 3) int64, labels (n,) uint32, last_observed (n,) uint64)"""
    vps = int(config["voxels_per_side"])
    sem, trk = bool(config["with_semantics"]), bool(config["with_tracking"])
    mw = f32(min_weight) if min_weight > 0 else f32(mesh_min_weight)
    sd = f32(surface_distance)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    lin = np.arange(vps ** 3, dtype=np.int64)
    iv = np.stack([lin % vps, (lin // vps) % vps, lin // (vps * vps)], axis=1)
    wanted = None if not labels else np.array([int(v) & 0xffffffff for v in labels], np.uint32)  # (compared as 32-bit patterns)
    g, lab, stamp = [], [], []
    for r in np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0])):
        fl = (layers["flags"][r] & np.uint8(VOX_PUBLIC)).astype(np.uint32)
        label = layers["sem_label"][r].astype(np.uint32) if sem else np.zeros(vps ** 3, np.uint32)
        req, exc = np.uint32(flags_require), np.uint32(flags_exclude)
        m = (layers["weight"][r] >= mw) & (layers["distance"][r] <= sd) & ((fl & req) == req) & ((fl & exc) == 0)
        if wanted is not None:
            m &= np.isin(label, wanted)
        sel = np.flatnonzero(m)
        g.append(idx[r] * vps + iv[sel])
        lab.append(label[sel])
        stamp.append(layers["last_observed"][r][sel].astype(np.uint64) if trk else np.zeros(len(sel), np.uint64))
    if not g:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    return np.concatenate(g), np.concatenate(lab), np.concatenate(stamp)


def flood(g, lab, connectivity, by_label):
    """components by breadth-first search: a list of ascending lists of positions in the member order, in ascending order of
    their first (= least) position"""
    keys = [_key(int(x), int(y), int(z)) for x, y, z in g]
    at = {k: i for i, k in enumerate(keys)}
    steps = [_key(x, y, z) - _key(0, 0, 0) for x, y, z in offsets(connectivity)]
    lab = lab.tolist()
    seen = [False] * len(keys)
    comps = []
    for s in range(len(keys)):
        if seen[s]:
            continue
        seen[s] = True
        comp, todo = [s], deque([s])
        while todo:
            i = todo.popleft()
            k = keys[i]
            for d in steps:
                j = at.get(k + d)
                if j is None or seen[j] or (by_label and lab[j] != lab[i]):
                    continue
                seen[j] = True
                comp.append(j)
                todo.append(j)
        comp.sort()
        comps.append(comp)
    return comps


def segment(config, idx, layers, min_weight=0.0, surface_distance=0.0, connectivity=26, by_label=None, labels=None, flags_require=0,
            flags_exclude=0, min_voxels=1, max_voxels=0, want_voxels=True, mesh_min_weight=1e-4):
    """the result of FusionContext.segment_map as a dict: "stats", the arrays of COMPONENT_FIELDS, "centroid" and, with want_voxels,
    those of VOXEL_FIELDS; `config`: checkpoint.config_fields.  by_label None = True with semantics."""
    assert connectivity in (6, 18, 26)
    by_label = bool(config["with_semantics"]) if by_label is None else bool(by_label)
    g, lab, stamp = members(config, idx, layers, min_weight, surface_distance, labels, flags_require, flags_exclude, mesh_min_weight)
    comps = flood(g, lab, connectivity, by_label)
    lo, hi = max(int(min_voxels), 1), int(max_voxels)
    assert hi <= 0 or hi >= lo
    stats = dict.fromkeys(STATS, 0)
    stats["n_blocks"], stats["n_member_voxels"], stats["n_components_all"] = len(np.asarray(idx).reshape(-1, 3)), len(g), len(comps)
    stats["n_too_small"] = sum(len(c) < lo for c in comps)
    stats["n_too_large"] = sum(hi > 0 and len(c) > hi for c in comps)
    kept = [c for c in comps if len(c) >= lo and (hi <= 0 or len(c) <= hi)]
    stats["n_components"], stats["n_voxels"] = len(kept), sum(len(c) for c in kept)
    m = len(kept)
    out = {name: np.zeros((m,) + sh, dt) for name, dt, sh in COMPONENT_FIELDS}
    first = 0
    for i, c in enumerate(kept):
        v = g[c]
        out["label"][i] = np.uint32(lab[c[0]]).astype(np.int32)
        out["n_voxels"][i] = len(c)
        out["bbox_min"][i], out["bbox_max"][i] = v.min(axis=0), v.max(axis=0)
        out["sum"][i] = v.sum(axis=0, dtype=np.int64)
        out["representative"][i] = v[0]
        out["last_observed_max"][i] = stamp[c].max()
        out["first"][i] = first
        first += len(c)
    out["centroid"] = (out["sum"].astype(np.float64) / np.maximum(out["n_voxels"], 1).astype(np.float64)[:, None] + 0.5) * float(f32(config["voxel_size"]))
    if want_voxels:
        out["voxels"] = (np.concatenate([g[c] for c in kept]) if kept else np.zeros((0, 3))).astype(np.int32).reshape(-1, 3)
        out["voxel_component"] = np.concatenate([np.full(len(c), i + 1, np.uint32) for i, c in enumerate(kept)] + [np.zeros(0, np.uint32)])
    out["stats"] = stats
    return out
