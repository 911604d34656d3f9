"""Timing of khr_query_points at the C3 geometry of bench.py: 1280x720, 2 cm voxels, 20 labels.  Fuses `--frames` frames of the
synthetic stream, then asks the map about the last frame's back-projected depth pixels, in image order and shuffled with a fixed
seed, and measures in this one process the whole call in the device form (points and outputs in device memory, no counters: the
call is enqueued, then khr_sync) with every output, with the distance alone, and in the host form; best and median of
`--repeats` calls after a warm-up.  Kernel time comes from a separate run under a kernel trace (the same script: the launches are
ordered / all outputs, ordered / distance only, shuffled / all outputs, shuffled / distance only, then the host form).
Prints one JSON line.  From the repository root:  python tools/query_timing.py [--frames 40]"""
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
    depth = np.asarray(fr["depth"], np.float64)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sel = np.flatnonzero((depth > 0).ravel())
    z = depth.ravel()[sel]
    cam = np.stack([(uu.ravel()[sel] - s.cx) / s.fx * z, (vv.ravel()[sel] - s.cy) / s.fy * z, z], axis=1)
    T = np.asarray(fr["pose"], np.float64).reshape(4, 4)
    ordered = np.ascontiguousarray((cam @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
    shuffled = np.ascontiguousarray(ordered[np.random.default_rng(5).permutation(len(ordered))])
    n = len(ordered)
    hip = C.CDLL("libamdhip64.so")

    def dmalloc(nbytes, src=None):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        if src is not None:
            assert hip.hipMemcpy(p, C.c_void_p(src.ctypes.data), C.c_size_t(nbytes), 1) == 0
        return p.value

    host = {k: np.zeros((n,) + sh, dt) for k, dt, sh in ctx.QUERY_FIELDS}
    dev = {k: dmalloc(arr.nbytes) for k, arr in host.items()}
    d_pts = {"ordered": dmalloc(ordered.nbytes, ordered), "shuffled": dmalloc(shuffled.nbytes, shuffled)}

    def timed(points, out, on_device):
        for _ in range(3):
            rc, _ = ctx.query_points_into(n, points, out, on_device=on_device, want_stats=False)
            assert rc == 0
        ts = []
        for _ in range(a.repeats):
            ctx.sync()
            t0 = time.perf_counter()
            rc, _ = ctx.query_points_into(n, points, out, on_device=on_device, want_stats=False)
            ctx.sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        return {"ms_best": min(ts), "ms_median": statistics.median(ts), "points_per_s_median": n / (1e-3 * statistics.median(ts))}

    res = {"what": "khr_query_points timing", "width": W, "height": H, "voxel_size": a.voxel_size, "frames": a.frames,
           "blocks": ctx.num_blocks(), "points": n, "repeats": a.repeats}
    for order in ("ordered", "shuffled"):
        res[order + "_device_all"] = timed(d_pts[order], dev, True)
        res[order + "_device_distance_only"] = timed(d_pts[order], {"distance": dev["distance"]}, True)
    res["ordered_host_all"] = timed(ordered, host, False)
    rc, stats = ctx.query_points_into(n, ordered, host)
    res["stats"] = stats
    for p in list(dev.values()) + list(d_pts.values()):
        hip.hipFree(C.c_void_p(p))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
