"""Timing of khr_distance_field at the C3 geometry of bench.py: 1280x720, 2 cm voxels, 20 labels.  Fuses `--frames` frames of the
synthetic stream, then asks for the distance field of a box of `--dims` cells of `--ratio` voxels around the last camera position
with a range of `--max-distance` metres (the reference's freespace_places: ratio 2, 4.5 m), and measures in this one process the
whole call in the device form (outputs in device memory, no counters: the call is enqueued, then khr_sync), with and without the
inner transform, and in the host form; best and median of `--repeats` calls after a warm-up.
--trace DIR runs the same measurement once more in a child process under a kernel trace (rocprofv3 --kernel-trace --stats
--output-format csv) and adds the per-kernel times of the k_df_* kernels from its statistics.
Prints one JSON line.  From the repository root:  python tools/distance_timing.py [--frames 40] [--trace DIR]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_stats(trace_dir, argv):
    """the k_df_* rows of a kernel trace of this script: name -> calls, mean and total microseconds"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "distance", "--", sys.executable, os.path.abspath(__file__)] + argv
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            if "k_df_" in name:
                short = name[name.index("k_df_"):].split("(")[0]
                out[short] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) * 1e-3, "total_us": float(row["TotalDurationNs"]) * 1e-3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--voxel-size", type=float, default=0.02)
    ap.add_argument("--max-blocks", type=int, default=16384)
    ap.add_argument("--ratio", type=int, default=2)
    ap.add_argument("--max-distance", type=float, default=4.5)
    ap.add_argument("--dims", type=int, nargs=3, default=(256, 256, 64))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace", default=None, help="directory for a kernel trace of a second run")
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
    cell = float(np.float32(a.voxel_size) * np.float32(a.ratio))
    t = np.asarray(fr["pose"], np.float64).reshape(4, 4)[:3, 3]
    dims = tuple(a.dims)
    origin = tuple(int(np.floor(t[k] / cell)) - dims[k] // 2 for k in range(3))
    n = int(np.prod(dims))
    hip = C.CDLL("libamdhip64.so")

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p.value

    host = {k: np.zeros(n, dt) for k, dt in ctx.DF_FIELDS}
    dev = {k: dmalloc(arr.nbytes) for k, arr in host.items()}

    def timed(out, on_device, positive_only):
        rq = ctx.df_request(origin, dims, a.ratio, a.max_distance, positive_only=positive_only)
        for _ in range(3):
            rc, _ = ctx.distance_field_into(rq, out, on_device=on_device, want_stats=False)
            assert rc == 0, rc
        ts = []
        for _ in range(a.repeats):
            ctx.sync()
            t0 = time.perf_counter()
            rc, _ = ctx.distance_field_into(rq, out, on_device=on_device, want_stats=False)
            ctx.sync()
            ts.append(1e3 * (time.perf_counter() - t0))
        return {"ms_best": min(ts), "ms_median": statistics.median(ts), "cells_per_s_median": n / (1e-3 * statistics.median(ts))}

    res = {"what": "khr_distance_field timing", "width": W, "height": H, "voxel_size": a.voxel_size, "frames": a.frames, "blocks": ctx.num_blocks(),
           "origin": origin, "dims": dims, "cells": n, "ratio": a.ratio, "max_distance": a.max_distance,
           "range_cells": int(np.floor(np.float32(a.max_distance) / np.float32(cell))), "repeats": a.repeats}
    res["device_signed"] = timed(dev, True, False)
    res["device_positive_only"] = timed(dev, True, True)
    res["host_signed"] = timed(host, False, False)
    res["host_positive_only"] = timed(host, False, True)
    rc, res["stats"] = ctx.distance_field_into(ctx.df_request(origin, dims, a.ratio, a.max_distance), host)
    for p in dev.values():
        hip.hipFree(C.c_void_p(p))
    ctx.close()
    if a.trace:
        argv = ["--frames", str(a.frames), "--width", str(W), "--height", str(H), "--voxel-size", str(a.voxel_size), "--max-blocks", str(a.max_blocks),
                "--ratio", str(a.ratio), "--max-distance", str(a.max_distance), "--dims"] + [str(d) for d in dims] + ["--repeats", str(a.repeats)]
        res["kernels"] = kernel_stats(a.trace, argv)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
