"""numpy restatement of khr_query_points (ASSUMPTIONS.md A.13) over a render_replica.BlockSet: vectorised over points, every one of
the 56 taps of a point's seven samples looked up on its own (no shared neighbourhood, no block reuse), so that it has nothing in
common with the kernel but the definition.  All arithmetic in float32, in the order A.13 writes it."""
import numpy as np

import render_replica as rr

f32 = np.float32
QP_VALUE, QP_GRADIENT, QP_VOXEL = 1, 2, 4
FIELDS = ("distance", "gradient", "weight", "color", "label", "flags", "last_observed", "status")


class QueryBlocks(rr.BlockSet):
    """render_replica.BlockSet plus the last_observed layer (the blocks are fetched once: the extra layer is taken from the
    dicts as they pass through)"""

    def __init__(self, indices, get_block, vps):
        stamps = []

        def grab(idx):
            b = get_block(idx)
            stamps.append((self.pack(int(idx[0]), int(idx[1]), int(idx[2])), np.asarray(b["last_observed"], np.uint64)))
            return b

        super().__init__(indices, grab, vps)
        self.last_observed = np.zeros((len(self.keys) + 1, self.nv), np.uint64)
        for key, lo in stamps:
            self.last_observed[int(np.searchsorted(self.keys, key))] = lo


def index_and_fraction(points, vs_inv):
    """A.13 indices: (in range, [i0 per axis] int64, [f per axis] float32); out-of-range points get index 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = [points[:, a] * vs_inv - f32(0.5) for a in range(3)]
        ok = np.ones(len(points), bool)
        for ga in g:
            ok &= np.abs(ga) < rr.INDEX_LIMIT  # (False for NaN)
        g = [np.where(ok, ga, f32(0)) for ga in g]
        i0 = [np.floor(ga).astype(np.int64) for ga in g]
        f = [ga - ia.astype(f32) for ga, ia in zip(g, i0)]
    return ok, i0, f


def sample_at(blocks, j, f, min_weight):
    """S(j): the trilinear combination of the taps j + (t & 1, (t >> 1) & 1, t >> 2) with the fractions f: (valid, distance)"""
    valid = np.ones(j[0].shape, bool)
    d = []
    for t in range(8):
        row, found, lin = blocks.lookup(j[0] + (t & 1), j[1] + ((t >> 1) & 1), j[2] + (t >> 2))
        valid &= found & (blocks.weight[row, lin] >= min_weight)
        d.append(blocks.distance[row, lin])
    with np.errstate(invalid="ignore", over="ignore"):
        c00, c10 = d[0] + f[0] * (d[1] - d[0]), d[2] + f[0] * (d[3] - d[2])
        c01, c11 = d[4] + f[0] * (d[5] - d[4]), d[6] + f[0] * (d[7] - d[6])
        c0, c1 = c00 + f[1] * (c10 - c00), c01 + f[1] * (c11 - c01)
        return valid, c0 + f[2] * (c1 - c0)


def query(blocks, points, voxel_size, min_weight=1e-4, with_semantics=True, with_tracking=True):
    """the outputs of FusionContext.query_points for `points` (n, 3) plus n_value / n_gradient / n_voxel"""
    pts = np.ascontiguousarray(points, f32).reshape(-1, 3)
    n = len(pts)
    vs_inv = f32(1) / f32(voxel_size)
    min_weight = f32(min_weight)
    ok, i0, f = index_and_fraction(pts, vs_inv)
    status = np.zeros(n, np.uint8)
    # distance
    valid, d = sample_at(blocks, i0, f, min_weight)
    valid &= ok
    distance = np.where(valid, d, f32(0)).astype(f32)
    status[valid] |= QP_VALUE
    # gradient: central differences one voxel to either side in index space, the fractions unchanged
    scale = f32(0.5) * vs_inv
    all_valid = ok.copy()
    grad = []
    for a in range(3):
        jp, jm = list(i0), list(i0)
        jp[a], jm[a] = i0[a] + 1, i0[a] - 1
        vp, dp = sample_at(blocks, jp, f, min_weight)
        vm, dm = sample_at(blocks, jm, f, min_weight)
        all_valid &= vp & vm
        with np.errstate(invalid="ignore", over="ignore"):
            grad.append((dp - dm) * scale)
    gradient = np.stack([np.where(all_valid, ga, f32(0)) for ga in grad], axis=1).astype(f32)
    status[all_valid] |= QP_GRADIENT
    # attribute voxel: floor(p * voxel_size_inv)
    with np.errstate(invalid="ignore", over="ignore"):
        gi = [np.floor(pts[:, a] * vs_inv) for a in range(3)]
        vok = ok.copy()
        for ga in gi:
            vok &= np.abs(ga) < rr.INDEX_LIMIT
        gi = [np.where(vok, ga, f32(0)).astype(np.int64) for ga in gi]
    row, found, lin = blocks.lookup(*gi)
    found &= vok
    status[found] |= QP_VOXEL
    out = {
        "distance": distance, "gradient": gradient, "status": status,
        "weight": np.where(found, blocks.weight[row, lin], f32(0)).astype(f32),
        "color": np.where(found[:, None], blocks.color[row, lin], 0).astype(np.uint8),
        "label": (np.where(found, blocks.label[row, lin], 0) if with_semantics else np.zeros(n)).astype(np.uint32),
        "flags": np.where(found, blocks.flags[row, lin], 0).astype(np.uint8),
        "last_observed": (np.where(found, blocks.last_observed[row, lin], 0) if with_tracking else np.zeros(n)).astype(np.uint64),
    }
    out["n_value"], out["n_gradient"], out["n_voxel"] = int(valid.sum()), int(all_valid.sum()), int(found.sum())
    return out
