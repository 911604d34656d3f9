"""numpy restatement of khr_merge_map (ASSUMPTIONS.md A.17) on (indices, layers) as khronos_amd.checkpoint.unpack gives them: a
plain loop over candidate blocks, every voxel of a block at once.  The RESAMPLE sample is query_replica.query at the transformed
voxel centre.  All arithmetic in float32, in the order A.17 writes it.  Needs no device and no library."""
import numpy as np

import query_replica as qr
import render_replica as rr

f32 = np.float32
ALIGNED, RESAMPLE = 0, 1
VOX_ACTIVE, VOX_EVER_FREE, VOX_TO_REMOVE, VOX_SEM_VALID = 1, 2, 4, 8
BLK_TOUCHED, BLK_HAS_ACTIVE = 7, 8  # UPDATED | MESH_UPDATED | TRACKING_UPDATED
KEY_LIM = 1 << 20
STATS = ("n_src_blocks", "n_candidate_blocks", "n_touched_blocks", "n_new_blocks", "n_added_voxels", "n_merged_voxels")


class MergeRangeError(ValueError):
    """a touched destination block lies outside the 21-bit key range (KHR_EINVAL)"""


def src_T_dst(pose):
    """[R^T | -R^T t] formed in double, cast to float32 once; returns the 3 x 4 float32 matrix"""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    M = np.zeros((3, 4), np.float64)
    for a in range(3):
        t = 0.0
        for k in range(3):
            M[a, k] = T[k, a]
            t += T[k, a] * T[k, 3]
        M[a, 3] = -t
    return M.astype(f32)


def _xf(M, x, y, z):
    return [((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)]


def _in_range(b):
    return all(-KEY_LIM <= int(v) < KEY_LIM for v in b)


def candidates(src_idx, vps, vs, mode, voxel_offset, pose):
    """the destination blocks the source blocks can reach (a superset of the touched ones), as a sorted list of tuples"""
    out = set()
    vs = f32(vs)
    bs, vs_inv = vs * f32(vps), f32(1) / vs
    for b in np.asarray(src_idx, np.int64).reshape(-1, 3):
        if mode == ALIGNED:
            lo = [(int(b[a]) * vps + int(voxel_offset[a])) // vps for a in range(3)]
            hi = [(int(b[a]) * vps + int(voxel_offset[a]) + vps - 1) // vps for a in range(3)]
        else:
            F = np.asarray(pose, np.float64).reshape(4, 4)[:3].astype(f32)
            mn, mx = None, None
            for c in range(8):
                q = []
                for a in range(3):
                    l = f32(b[a]) * bs + f32(0.5) * vs
                    q.append(l + bs if (c >> a) & 1 else l)
                t = _xf(F, q[0], q[1], q[2])
                mn = t if mn is None else [min(m, v) for m, v in zip(mn, t)]
                mx = t if mx is None else [max(m, v) for m, v in zip(mx, t)]
            lim = float(rr.INDEX_LIMIT)
            lo = [(int(min(max(np.floor(mn[a] * vs_inv), -lim), lim)) - 1) // vps for a in range(3)]
            hi = [min((int(min(max(np.floor(mx[a] * vs_inv), -lim), lim)) + 1) // vps, lo[a] + 2) for a in range(3)]
        for z in range(lo[2], hi[2] + 1):
            for y in range(lo[1], hi[1] + 1):
                for x in range(lo[0], hi[0] + 1):
                    out.add((x, y, z))
    return sorted(out)


class _Src:
    """the source blocks by index; find(): global voxel indices -> (row, allocated, linear index)"""

    def __init__(self, idx, vps):
        self.vps = vps
        self.rows = {tuple(int(v) for v in b): i for i, b in enumerate(np.asarray(idx, np.int64).reshape(-1, 3))}

    def find(self, gx, gy, gz):
        v = self.vps
        bx, by, bz = gx // v, gy // v, gz // v  # floor division (A.1)
        row = np.zeros(gx.shape, np.int64)
        found = np.zeros(gx.shape, bool)
        for b in set(zip(bx.tolist(), by.tolist(), bz.tolist())):
            if b in self.rows and _in_range(b):
                sel = (bx == b[0]) & (by == b[1]) & (bz == b[2])
                row[sel], found[sel] = self.rows[b], True
        return row, found, (gx % v) + v * ((gy % v) + v * (gz % v))


def merge(config, dst_idx, dst_layers, src_idx, src_layers, mode=ALIGNED, voxel_offset=(0, 0, 0), pose=None, min_weight=0.0,
          max_weight=1e4, mesh_min_weight=1e-4):
    """(indices, layers, stats) of the destination after the merge; `config`: checkpoint.config_fields.  The inputs are left
    unchanged; the blocks come back in (x, y, z) order."""
    vps, vs, trunc = int(config["voxels_per_side"]), f32(config["voxel_size"]), f32(config["truncation_distance"])
    trk, sem = bool(config["with_tracking"]), bool(config["with_semantics"])
    nv = vps ** 3
    mw = f32(min_weight) if min_weight > 0 else f32(mesh_min_weight)
    max_weight = f32(max_weight)
    dst_idx = np.asarray(dst_idx, np.int32).reshape(-1, 3)
    src_idx = np.asarray(src_idx, np.int32).reshape(-1, 3)
    D = {k: [np.array(r) for r in v] for k, v in dst_layers.items()}  # per layer, a list of per-block arrays (grows)
    didx = [tuple(int(v) for v in b) for b in dst_idx]
    drow = {b: i for i, b in enumerate(didx)}
    S = src_layers
    src = _Src(src_idx, vps)
    stats = dict.fromkeys(STATS, 0)
    stats["n_src_blocks"] = len(src_idx)
    lin = np.arange(nv, dtype=np.int64)
    ix, iy, iz = lin % vps, (lin // vps) % vps, lin // (vps * vps)
    if mode == RESAMPLE:
        M = src_T_dst(pose)
        zero = {"sem_label": np.zeros(nv, np.uint32), "last_observed": np.zeros(nv, np.uint64)}

        def get_block(b):
            r = src.rows[tuple(int(v) for v in b)]
            return {"distance": S["distance"][r], "weight": S["weight"][r], "color": S["color"][r], "flags": S["flags"][r],
                    "sem_label": S["sem_label"][r] if sem else zero["sem_label"],
                    "last_observed": S["last_observed"][r] if trk else zero["last_observed"]}

        qblocks = qr.QueryBlocks(src_idx, get_block, vps)
    for b in candidates(src_idx, vps, vs, mode, voxel_offset, pose):
        in_range = _in_range(b)
        stats["n_candidate_blocks"] += 1 if in_range else 0
        # the source sample of every voxel of the block
        if mode == ALIGNED:
            g = [b[a] * vps + (ix, iy, iz)[a] - int(voxel_offset[a]) for a in range(3)]
            row, found, sl = src.find(*g)
            valid = found & (S["weight"][row, sl] >= mw)
            d_s = S["distance"][row, sl]
            have = found
        else:
            bs = vs * f32(vps)
            c = [f32(b[a]) * bs + ((ix, iy, iz)[a].astype(f32) + f32(0.5)) * vs for a in range(3)]
            p = np.stack(_xf(M, c[0], c[1], c[2]), axis=1).astype(f32)
            q = qr.query(qblocks, p, vs, min_weight=mw, with_semantics=sem, with_tracking=trk)
            valid = (q["status"] & qr.QP_VALUE) != 0
            d_s = np.minimum(np.maximum(q["distance"], -trunc), trunc).astype(f32)
            vs_inv = f32(1) / vs
            with np.errstate(invalid="ignore", over="ignore"):
                gi = [np.floor(p[:, a] * vs_inv) for a in range(3)]
                ok = np.ones(nv, bool)
                for ga in gi:
                    ok &= np.abs(ga) < rr.INDEX_LIMIT
                gi = [np.where(ok, ga, f32(0)).astype(np.int64) for ga in gi]
            row, have, sl = src.find(*gi)
            have &= ok
        if not valid.any():
            continue
        if not in_range:
            raise MergeRangeError("touched block %r outside the key range" % (b,))
        stats["n_touched_blocks"] += 1
        if b not in drow:
            stats["n_new_blocks"] += 1
            drow[b] = len(didx)
            didx.append(b)
            for k, v in D.items():
                v.append(np.zeros(v[0].shape if v else dst_layers[k].shape[1:], dst_layers[k].dtype))
        r = drow[b]

        def s_of(name, dtype):  # the attribute voxel's value, 0 where there is none
            a = S[name][row, sl]
            return np.where(have.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0).astype(dtype)

        w_s, col_s, vf_s = s_of("weight", f32), s_of("color", np.uint8), s_of("flags", np.uint8)
        w_d, d_d, col_d, vf_d = D["weight"][r], D["distance"][r], D["color"][r], D["flags"][r]
        add = valid & (w_d == 0)
        mrg = valid & ~add
        stats["n_added_voxels"] += int(add.sum())
        stats["n_merged_voxels"] += int(mrg.sum())
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ws = w_d + w_s
            d_m = (d_d * w_d + d_s * w_s) / ws
            cd, cs = col_d[:, :3].astype(f32), col_s[:, :3].astype(f32)
            c_m = np.floor((cd * w_d[:, None] + cs * w_s[:, None]) / ws[:, None] + f32(0.5))
        c_m = np.concatenate([np.nan_to_num(c_m).astype(np.uint8), np.full((nv, 1), 255, np.uint8)], axis=1)
        a_s, a_d = col_s[:, 3] != 0, col_d[:, 3] != 0
        col_m = np.where((a_s & a_d)[:, None], c_m, np.where(a_s[:, None], col_s, col_d))
        vf_m = ((vf_d | vf_s) & (VOX_ACTIVE | VOX_SEM_VALID)) | (vf_d & vf_s & (VOX_EVER_FREE | VOX_TO_REMOVE))
        D["distance"][r] = np.where(add, d_s, np.where(mrg, d_m, d_d)).astype(f32)
        D["weight"][r] = np.where(add, np.minimum(w_s, max_weight), np.where(mrg, np.minimum(ws, max_weight), w_d)).astype(f32)
        D["color"][r] = np.where(add[:, None], col_s, np.where(mrg[:, None], col_m, col_d)).astype(np.uint8)
        D["flags"][r] = np.where(add, vf_s, np.where(mrg, vf_m, vf_d)).astype(np.uint8)
        if trk:
            for name in ("last_observed", "last_occupied"):
                t_s, t_d = s_of(name, np.uint64), D[name][r]
                D[name][r] = np.where(add, t_s, np.where(mrg, np.maximum(t_s, t_d), t_d)).astype(np.uint64)
        if sem:
            lab_s, l_s = s_of("sem_label", np.uint32), s_of("likelihoods", f32)
            lab_d, l_d = D["sem_label"][r], D["likelihoods"][r]
            sv_s, sv_d = (vf_s & VOX_SEM_VALID) != 0, (vf_d & VOX_SEM_VALID) != 0
            l_s = np.where(sv_s[:, None], l_s, f32(0))
            both, s_only = mrg & sv_s & sv_d, mrg & sv_s & ~sv_d
            l_sum = (l_d + l_s).astype(f32)
            D["likelihoods"][r] = np.where((add | s_only)[:, None], l_s, np.where(both[:, None], l_sum, l_d)).astype(f32)
            D["sem_label"][r] = np.where(add | s_only, lab_s, np.where(both, np.argmax(l_sum, axis=1), lab_d)).astype(np.uint32)
        act = bool((D["flags"][r] & VOX_ACTIVE).any())
        D["block_flags"][r] = np.uint8(int(D["block_flags"][r]) | BLK_TOUCHED | (BLK_HAS_ACTIVE if act else 0))
    idx = np.array(didx, np.int32).reshape(-1, 3)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0])) if len(idx) else np.zeros(0, np.int64)
    layers = {k: (np.stack([v[i] for i in order]) if len(order) else np.array(dst_layers[k])) for k, v in D.items()}
    return idx[order], layers, stats
