"""Timing of khr_align_linearize / khr_align_frame at the C3 geometry of bench.py: 1280x720, 2 cm voxels, 20 labels.  Fuses
`--frames` frames of the synthetic stream, then registers the last frame's depth image (device memory) from its true pose moved by
about 1 degree and 3 cm.  Measured in this one process, best and median of `--repeats` calls after a warm-up: one
khr_align_linearize call at strides 1, 2 and 4 (memset + kernel + 4 KiB copy + the host wait); khr_query_points with distance and
gradient alone on the same world points in device memory (call + khr_sync) -- the yardstick that exists without this feature; and
khr_align_frame's wall time per iteration.  Kernel times come from a separate run of this script under a kernel trace.
Prints one JSON line.  From the repository root:  python tools/align_timing.py [--frames 40]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--voxel-size", type=float, default=0.02)
    ap.add_argument("--max-blocks", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    from khronos_amd import FusionContext, default_config
    from khronos_amd.synth import SyntheticStream
    W, H = a.width, a.height
    cfg = default_config(voxel_size=a.voxel_size, truncation_distance=3 * a.voxel_size, with_semantics=1, with_tracking=1, num_labels=20,
                         max_blocks=a.max_blocks, max_frame_pixels=W * H, max_mesh_vertices=1 << 20)
    ctx = FusionContext(cfg)
    s = SyntheticStream(W, H)
    sen = ctx.make_sensor(W, H, s.fx, s.fy, s.cx, s.cy)
    for i in range(a.frames):
        fr = s.render(i)
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        ctx.integrate(slot)
        ctx.update_tracking(fr["stamp"])
    ctx.sync()
    truth = np.asarray(fr["pose"], np.float64).reshape(4, 4)
    c, sn = np.cos(np.deg2rad(1.0)), np.sin(np.deg2rad(1.0))
    start = truth.copy()
    start[:3, :3] = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]) @ truth[:3, :3]
    start[:3, 3] += [0.02, 0.015, -0.017]
    depth = np.ascontiguousarray(fr["depth"], np.float32)
    hip = C.CDLL("libamdhip64.so")

    def dmalloc(nbytes, src=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        if src is not None:
            assert hip.hipMemcpy(p, C.c_void_p(src.ctypes.data), C.c_size_t(nbytes), 1) == 0
        return p.value

    d_depth = dmalloc(depth.nbytes, depth)

    def timed(call):
        for _ in range(3):
            call()
        ts = []
        for _ in range(a.repeats):
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        return {"ms_best": min(ts), "ms_median": statistics.median(ts)}

    res = {"what": "khr_align timing", "width": W, "height": H, "voxel_size": a.voxel_size, "frames": a.frames, "blocks": ctx.num_blocks(),
           "repeats": a.repeats}
    words = np.zeros(32, np.uint64)
    freed = [d_depth]
    for stride in (1, 2, 4):
        rq, keep = ctx.align_request(start, depth=d_depth, sensor=sen, stride=stride, device=True)
        r = timed(lambda: ctx.align_linearize_into(rq, words, on_device=True))
        r.update(n_source=int(words[30]), n_gradient=int(words[29]), n_inlier=int(words[28]))
        # the yardstick: khr_query_points, distance and gradient alone, on the same world points
        sub = depth[::stride, ::stride]
        vv, uu = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
        ok = (sub > 0) & (sub >= sen.min_range) & (sub <= sen.max_range)
        z = sub[ok].astype(np.float64)
        cam = np.stack([(uu[ok] - s.cx) / s.fx * z, (vv[ok] - s.cy) / s.fy * z, z], axis=1)
        pw = np.ascontiguousarray((cam @ start[:3, :3].T + start[:3, 3]).astype(np.float32))
        n = len(pw)
        d_pw, d_dist, d_grad = dmalloc(pw.nbytes, pw), dmalloc(4 * n), dmalloc(12 * n)
        freed += [d_pw, d_dist, d_grad]
        q = timed(lambda: ctx.query_points_into(n, d_pw, {"distance": d_dist, "gradient": d_grad}, on_device=True, want_stats=False))
        r.update(query_points=n, query_ms_best=q["ms_best"], query_ms_median=q["ms_median"])
        # the loop: wall time per iteration
        pose = np.zeros(16)
        ts, its = [], 0
        for _ in range(max(3, a.repeats // 4)):
            t0 = time.perf_counter()
            rc, out = ctx.align_frame_into(rq, pose, on_device=True)
            ts.append(1e3 * (time.perf_counter() - t0))
            its = out["iterations"]
        r.update(loop_rc=rc, loop_iterations=its, loop_ms_median=statistics.median(ts), loop_ms_per_iteration=statistics.median(ts) / max(its, 1),
                 loop_inliers=[out["n_inlier_first"], out["n_inlier_last"]], loop_rmse=[out["rmse_first"], out["rmse_last"]])
        res["stride_%d" % stride] = r
    for p in freed:
        hip.hipFree(C.c_void_p(p))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
