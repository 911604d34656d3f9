"""numpy restatement of khr_diff_map (ASSUMPTIONS.md A.18) on (indices, layers) as khronos_amd.checkpoint.unpack gives them: a
plain loop over the candidate blocks of A.17 that `now` holds, every voxel of a block at once.  The sample of `then` is A.17's
source sample (merge_replica's candidates, block lookup and transform; query_replica.query under RESAMPLE).  Float32 throughout.
Needs no device and no library."""
import numpy as np

import merge_replica as mr
import query_replica as qr
from merge_replica import ALIGNED, RESAMPLE, _Src, candidates, src_T_dst  # noqa: F401

f32 = np.float32
APPEARED, DISAPPEARED = 1, 2
STATS = ("n_ref_blocks", "n_candidate_blocks", "n_present_blocks", "n_compared_voxels", "n_appeared", "n_disappeared", "n_only_now",
         "n_only_then", "n_changed_blocks")
VOXEL_FIELDS = (("voxels", np.int32, (3,)), ("kind", np.uint8, ()), ("d_now", f32, ()), ("d_then", f32, ()), ("label", np.uint32, ()),
                ("stamp_now", np.uint64, ()), ("stamp_then", np.uint64, ()))
BLOCK_FIELDS = (("blocks", np.int32, (3,)), ("block_appeared", np.uint32, ()), ("block_disappeared", np.uint32, ()), ("block_first", np.uint32, ()))


class Sampler:
    """`then` sampled at the voxels of a block of `now`: (valid, d_then, label_then, stamp_then), label and stamp 0 where the
    attribute voxel is missing"""

    def __init__(self, config, then_idx, then_layers, mode, voxel_offset, pose, mw):
        self.vps, self.vs, self.trunc = int(config["voxels_per_side"]), f32(config["voxel_size"]), f32(config["truncation_distance"])
        self.trk, self.sem = bool(config["with_tracking"]), bool(config["with_semantics"])
        self.mode, self.off, self.mw, self.S = mode, [int(v) for v in voxel_offset], mw, then_layers
        nv = self.vps ** 3
        lin = np.arange(nv, dtype=np.int64)
        self.iv = (lin % self.vps, (lin // self.vps) % self.vps, lin // (self.vps * self.vps))
        self.src = _Src(then_idx, self.vps)
        if mode == RESAMPLE:
            self.M = src_T_dst(pose)
            S, zl, zs = then_layers, np.zeros(nv, np.uint32), np.zeros(nv, np.uint64)

            def get_block(b):
                r = self.src.rows[tuple(int(v) for v in b)]
                return {"distance": S["distance"][r], "weight": S["weight"][r], "color": S["color"][r], "flags": S["flags"][r],
                        "sem_label": S["sem_label"][r] if self.sem else zl, "last_observed": S["last_observed"][r] if self.trk else zs}

            self.blocks = qr.QueryBlocks(np.asarray(then_idx, np.int32).reshape(-1, 3), get_block, self.vps)

    def __call__(self, b):
        vps, S = self.vps, self.S
        nv = vps ** 3
        if self.mode == ALIGNED:
            g = [b[a] * vps + self.iv[a] - self.off[a] for a in range(3)]
            row, found, sl = self.src.find(*g)
            valid = found & (S["weight"][row, sl] >= self.mw)
            lab = np.where(found, S["sem_label"][row, sl], 0) if self.sem else np.zeros(nv)
            stamp = np.where(found, S["last_observed"][row, sl], 0) if self.trk else np.zeros(nv)
            return valid, S["distance"][row, sl].astype(f32), lab.astype(np.uint32), stamp.astype(np.uint64)
        bs = self.vs * f32(vps)
        c = [f32(b[a]) * bs + (self.iv[a].astype(f32) + f32(0.5)) * self.vs for a in range(3)]
        p = np.stack(mr._xf(self.M, c[0], c[1], c[2]), axis=1).astype(f32)
        q = qr.query(self.blocks, p, self.vs, min_weight=self.mw, with_semantics=self.sem, with_tracking=self.trk)
        valid = (q["status"] & qr.QP_VALUE) != 0
        d = np.minimum(np.maximum(q["distance"], -self.trunc), self.trunc).astype(f32)
        return valid, d, q["label"], q["last_observed"]


def diff(config, now_idx, now_layers, then_idx, then_layers, mode=ALIGNED, voxel_offset=(0, 0, 0), pose=None, min_weight=0.0,
         occupied_distance=0.0, free_distance=None, mesh_min_weight=1e-4):
    """the result of FusionContext.diff_map as a dict: "stats" and the arrays of VOXEL_FIELDS / BLOCK_FIELDS; `config`:
    checkpoint.config_fields.  free_distance None = voxel_size."""
    vps, vs = int(config["voxels_per_side"]), f32(config["voxel_size"])
    trk, sem = bool(config["with_tracking"]), bool(config["with_semantics"])
    mw = f32(min_weight) if min_weight > 0 else f32(mesh_min_weight)
    occ, free = f32(occupied_distance), vs if free_distance is None else f32(free_distance)
    assert np.isfinite(occ) and np.isfinite(free) and occ < free
    now_idx = np.asarray(now_idx, np.int32).reshape(-1, 3)
    then_idx = np.asarray(then_idx, np.int32).reshape(-1, 3)
    rows = {tuple(int(v) for v in b): i for i, b in enumerate(now_idx)}
    sample = Sampler(config, then_idx, then_layers, mode, voxel_offset, pose, mw)
    stats = dict.fromkeys(STATS, 0)
    stats["n_ref_blocks"] = len(then_idx)
    per_block = []
    for b in candidates(then_idx, vps, vs, mode, voxel_offset, pose):  # (sorted: the (x, y, z) order of the result)
        if not mr._in_range(b):
            continue
        stats["n_candidate_blocks"] += 1
        if b not in rows:
            continue
        stats["n_present_blocks"] += 1
        r = rows[b]
        T, d_then, lab_then, stamp_then = sample(b)
        N = now_layers["weight"][r] >= mw
        d_now = now_layers["distance"][r].astype(f32)
        cmp_ = N & T
        app = cmp_ & (d_then >= free) & (d_now <= occ)
        dis = cmp_ & (d_then <= occ) & (d_now >= free)
        stats["n_compared_voxels"] += int(cmp_.sum())
        stats["n_appeared"] += int(app.sum())
        stats["n_disappeared"] += int(dis.sum())
        stats["n_only_now"] += int((N & ~T).sum())
        stats["n_only_then"] += int((~N & T).sum())
        chg = np.flatnonzero(app | dis)  # (ascending linear index)
        if len(chg) == 0:
            continue
        stats["n_changed_blocks"] += 1
        lab_now = now_layers["sem_label"][r] if sem else np.zeros(vps ** 3, np.uint32)
        stamp_now = now_layers["last_observed"][r] if trk else np.zeros(vps ** 3, np.uint64)
        vox = np.stack([b[a] * vps + sample.iv[a][chg] for a in range(3)], axis=1)
        per_block.append(dict(block=b, n_app=int(app.sum()), n_dis=int(dis.sum()), voxels=vox, kind=np.where(app[chg], APPEARED, DISAPPEARED),
                              d_now=d_now[chg], d_then=d_then[chg], label=np.where(app[chg], lab_now[chg], lab_then[chg]),
                              stamp_now=stamp_now[chg], stamp_then=stamp_then[chg]))
    out = {"stats": stats}
    for name, dt, sh in VOXEL_FIELDS:
        parts = [np.asarray(pb[name]).astype(dt).reshape((-1,) + sh) for pb in per_block]
        out[name] = np.concatenate(parts) if parts else np.zeros((0,) + sh, dt)
    counts = [pb["n_app"] + pb["n_dis"] for pb in per_block]
    out["blocks"] = np.array([pb["block"] for pb in per_block], np.int32).reshape(-1, 3)
    out["block_appeared"] = np.array([pb["n_app"] for pb in per_block], np.uint32)
    out["block_disappeared"] = np.array([pb["n_dis"] for pb in per_block], np.uint32)
    out["block_first"] = (np.cumsum([0] + counts)[:-1]).astype(np.uint32)
    return out
