"""numpy restatement of khr_render_view (ASSUMPTIONS.md A.12): vectorised over pixels, a plain loop over the samples, no empty-space
skipping and no block cache.  Works from per-block dicts as FusionContext.download_block and the oracle's get_block hand out
(distance, weight, color (n, 4) u8, sem_label, flags), so the same code checks the kernel against this context's own blocks and
against the CPU oracle's.  All arithmetic in float32, in the order A.12 writes it."""
import numpy as np

f32 = np.float32
INDEX_LIMIT = f32(2.0 ** 30)  # |p * voxel_size_inv - 0.5| at or beyond this (or NaN): no voxel there
KEY_BIAS, KEY_RANGE = 1 << 20, 1 << 21


class BlockSet:
    """the blocks of a map stacked per field, found by packed block index (A.1's 21-bit-per-axis keys) with a sorted search"""

    def __init__(self, indices, get_block, vps):
        idx = np.asarray(indices, np.int64).reshape(-1, 3)
        self.vps, self.nv = int(vps), int(vps) ** 3
        keys = self.pack(idx[:, 0], idx[:, 1], idx[:, 2])
        order = np.argsort(keys)
        self.keys = keys[order]
        n = len(idx)
        self.distance = np.zeros((n + 1, self.nv), f32)  # (row n: the target of failed lookups, never used for a result)
        self.weight = np.full((n + 1, self.nv), -1, f32)
        self.color = np.zeros((n + 1, self.nv, 4), np.uint8)
        self.label = np.zeros((n + 1, self.nv), np.uint32)
        self.flags = np.zeros((n + 1, self.nv), np.uint8)
        for row, i in enumerate(order):
            b = get_block(idx[i].astype(np.int32))
            self.distance[row], self.weight[row] = b["distance"], b["weight"]
            self.color[row] = np.asarray(b["color"], np.uint8).reshape(self.nv, 4)
            self.label[row], self.flags[row] = b["sem_label"], b["flags"]

    @staticmethod
    def pack(bx, by, bz):
        bx, by, bz = (np.asarray(a, np.int64) for a in (bx, by, bz))
        ok = np.ones(bx.shape, bool)
        for a in (bx, by, bz):
            ok &= (a >= -KEY_BIAS) & (a < KEY_BIAS)
        k = (bx + KEY_BIAS) | ((by + KEY_BIAS) << 21) | ((bz + KEY_BIAS) << 42)
        return np.where(ok, k, -1)

    def lookup(self, gx, gy, gz):
        """global voxel indices (int64 arrays) -> (block row or the spare row, allocated mask, linear voxel index): A.1's
        keyFromGlobalIndex = floor division / non-negative remainder"""
        v = self.vps
        key = self.pack(gx // v, gy // v, gz // v)
        n = len(self.keys)
        pos = np.minimum(np.searchsorted(self.keys, key), max(n - 1, 0))
        found = (self.keys[pos] == key) & (key >= 0) if n else np.zeros(key.shape, bool)
        row = np.where(found, pos, n)
        lin = (gx % v) + v * ((gy % v) + v * (gz % v))
        return row, found, lin


def _xform(R, t, x, y, z):
    """((r0*x + r1*y) + r2*z) + t per world axis, float32"""
    return [((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a] for a in range(3)]


def sample(blocks, p, vs_inv, min_weight):
    """the trilinear sample of A.12 at the points p = [px, py, pz] (float32 arrays): (valid, distance)"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = [pa * vs_inv - f32(0.5) for pa in p]
        ok = np.ones(g[0].shape, bool)
        for ga in g:
            ok &= np.abs(ga) < INDEX_LIMIT  # (False for NaN)
        g = [np.where(ok, ga, f32(0)) for ga in g]
        fl = [np.floor(ga) for ga in g]
        i0 = [a.astype(np.int64) for a in fl]
        f = [ga - a.astype(f32) for ga, a in zip(g, i0)]
        valid = ok.copy()
        d = []
        for t in range(8):  # tap t: x offset = bit 0, y = bit 1, z = bit 2
            row, found, lin = blocks.lookup(i0[0] + (t & 1), i0[1] + ((t >> 1) & 1), i0[2] + (t >> 2))
            valid &= found & (blocks.weight[row, lin] >= min_weight)
            d.append(blocks.distance[row, lin])
        c00, c10 = d[0] + f[0] * (d[1] - d[0]), d[2] + f[0] * (d[3] - d[2])
        c01, c11 = d[4] + f[0] * (d[5] - d[4]), d[6] + f[0] * (d[7] - d[6])
        c0, c1 = c00 + f[1] * (c10 - c00), c01 + f[1] * (c11 - c01)
        return valid, c0 + f[2] * (c1 - c0)


def render(indices, get_block, vps, voxel_size, sensor, pose, step_voxels=0.0, min_weight=1e-4, with_semantics=True, blocks=None):
    """sensor: anything with width, height, fx, fy, cx, cy, min_range, max_range; pose: world_T_sensor 4x4 (double).  Returns the
    images of FusionContext.render_view plus n_hit / n_blocked / samples_per_ray.  `blocks`: a BlockSet built earlier (the
    downloads are the slow part when several views read one map)."""
    if blocks is None:
        blocks = BlockSet(indices, get_block, vps)
    W, H = int(sensor.width), int(sensor.height)
    vs = f32(voxel_size)
    vs_inv = f32(1) / vs
    fx, fy, cx, cy = f32(sensor.fx), f32(sensor.fy), f32(sensor.cx), f32(sensor.cy)
    t_min, t_max = f32(sensor.min_range), f32(sensor.max_range)
    dt = f32(0.5 if step_voxels == 0 else step_voxels) * vs
    K = int(np.floor((t_max - t_min) / dt)) + 1
    min_weight = f32(min_weight)
    T = np.asarray(pose, np.float64).reshape(4, 4)
    R, tw = T[:3, :3].astype(f32), T[:3, 3].astype(f32)  # the pose cast to float once, as frame ingest does
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = ((uu.ravel().astype(f32) - cx) / fx).astype(f32)
    y = ((vv.ravel().astype(f32) - cy) / fy).astype(f32)
    n = W * H
    status = np.zeros(n, np.uint8)
    t_hit = np.zeros(n, f32)
    prev_valid = np.zeros(n, bool)
    d_prev = np.zeros(n, f32)
    live = np.ones(n, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            if not live.any():
                break
            sel = np.flatnonzero(live)
            t = t_min + f32(k) * dt
            xs, ys = x[sel], y[sel]
            valid, d = sample(blocks, _xform(R, tw, xs * t, ys * t, np.full(len(sel), t, f32)), vs_inv, min_weight)
            ends = valid & (d <= 0)
            front = ends & prev_valid[sel] & (d_prev[sel] > 0)
            frac = d_prev[sel] / (d_prev[sel] - d)
            th = (t_min + f32(k - 1) * dt) + frac * dt
            status[sel[front]] = 1
            t_hit[sel[front]] = th[front]
            status[sel[ends & ~front]] = 2
            live[sel[ends]] = False
            prev_valid[sel] = valid
            d_prev[sel] = np.where(valid, d, f32(0))
        hit = np.flatnonzero(status == 1)
        depth = np.zeros(n, f32)
        normal = np.zeros((n, 3), f32)
        color = np.zeros((n, 4), np.uint8)
        label = np.zeros(n, np.uint32)
        flags = np.zeros(n, np.uint8)
        if len(hit):
            th = t_hit[hit]
            depth[hit] = th
            ph = _xform(R, tw, x[hit] * th, y[hit] * th, th)
            gi = [np.floor(pa * vs_inv) for pa in ph]
            ok = np.ones(len(hit), bool)
            for ga in gi:
                ok &= np.abs(ga) < INDEX_LIMIT
            gi = [np.where(ok, ga, f32(0)).astype(np.int64) for ga in gi]
            row, found, lin = blocks.lookup(*gi)
            found &= ok
            color[hit] = np.where(found[:, None], blocks.color[row, lin], 0)
            if with_semantics:
                label[hit] = np.where(found, blocks.label[row, lin], 0)
            flags[hit] = np.where(found, blocks.flags[row, lin], 0)
            g, all_valid = [], np.ones(len(hit), bool)
            for a in range(3):
                qp, qm = list(ph), list(ph)
                qp[a], qm[a] = ph[a] + vs, ph[a] - vs
                vp_, dp = sample(blocks, qp, vs_inv, min_weight)
                vm_, dm = sample(blocks, qm, vs_inv, min_weight)
                all_valid &= vp_ & vm_
                g.append(dp - dm)
            length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            keep = all_valid & (length != 0)
            for a in range(3):
                normal[hit, a] = np.where(keep, g[a] / length, f32(0))
    return {"depth": depth.reshape(H, W), "normal": normal.reshape(H, W, 3), "color": color.reshape(H, W, 4),
            "label": label.reshape(H, W), "flags": flags.reshape(H, W), "status": status.reshape(H, W),
            "n_hit": int((status == 1).sum()), "n_blocked": int((status == 2).sum()), "samples_per_ray": K}
