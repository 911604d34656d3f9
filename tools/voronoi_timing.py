"""Timing of khr_voronoi_field beside khr_distance_field(positive_only = 1) on the same boxes, in one process.  Two set-ups:
  stream  the tests' stream (320x240, 10 cm voxels, 30 frames), the box of tests/distance_cases.stream_box: 40 x 40 x 24 cells of 2
          voxels around the last camera position, range 1.2 m
  large   the C3 geometry of bench.py (1280x720, 2 cm voxels, 20 labels, 40 frames), 256^3 cells of 2 voxels, range 4.5 m
Per set-up and call: a host clock around the call and the khr_sync that follows, the two calls alternating, best and median of
`--repeats` after a warm-up.  The distance field is asked for in its device form without counters (enqueue, then khr_sync); the
Voronoi field always waits once for its counters, the result stays on the device (no khr_voronoi_field_into in the timed region).
--trace DIR runs the same once more in a child process under a kernel trace (rocprofv3 --kernel-trace --stats --output-format csv) and
adds the per-kernel times of the k_df_* and k_vor_* kernels from its statistics.
Prints one JSON line.  From the repository root:  python tools/voronoi_timing.py [--setups stream large] [--trace DIR]"""
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

SETUPS = {"stream": dict(width=320, height=240, voxel_size=0.1, frames=30, max_blocks=4096, num_labels=20, dims=(40, 40, 24), ratio=2, max_distance=1.2),
          "large": dict(width=1280, height=720, voxel_size=0.02, frames=40, max_blocks=16384, num_labels=20, dims=(256, 256, 256), ratio=2, max_distance=4.5)}


def kernel_stats(trace_dir, argv):
    """the k_df_* / k_vor_* rows of a kernel trace of this script: name -> calls, mean and total microseconds"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "voronoi", "--", sys.executable, os.path.abspath(__file__)] + argv
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            for tag in ("k_df_", "k_vor_"):
                if tag in name:
                    short = name[name.index(tag):].split("(")[0]
                    out[short] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) * 1e-3, "total_us": float(row["TotalDurationNs"]) * 1e-3}
    return out


def run(name, repeats):
    from khronos_amd import FusionContext, default_config
    from khronos_amd.capi import KHR_VOR_L1_THEN_ANGLE
    from khronos_amd.synth import SyntheticStream
    s_ = SETUPS[name]
    W, H = s_["width"], s_["height"]
    cfg = default_config(voxel_size=s_["voxel_size"], truncation_distance=3 * s_["voxel_size"], with_semantics=1, with_tracking=1, num_labels=s_["num_labels"],
                         max_blocks=s_["max_blocks"], max_frame_pixels=W * H, max_mesh_vertices=1 << 20)
    ctx = FusionContext(cfg)
    s = SyntheticStream(W, H, seed=1234)
    sen = ctx.make_sensor(W, H, s.fx, s.fy, s.cx, s.cy)
    for i in range(s_["frames"]):
        fr = s.render(i)
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        ctx.integrate(slot)
        ctx.update_tracking(fr["stamp"])
    ctx.sync()
    ratio, md, dims = s_["ratio"], s_["max_distance"], tuple(s_["dims"])
    cell = float(np.float32(s_["voxel_size"]) * np.float32(ratio))
    t = np.asarray(fr["pose"], np.float64).reshape(4, 4)[:3, 3]
    origin = tuple(int(np.floor(t[k] / cell)) - dims[k] // 2 for k in range(3))
    n = int(np.prod(dims))
    hip = C.CDLL("libamdhip64.so")
    dev = {}
    for k, dt in ctx.DF_FIELDS:
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(n * np.dtype(dt).itemsize)) == 0
        dev[k] = p.value
    df_rq = ctx.df_request(origin, dims, ratio, md, positive_only=True)
    # the reference's values: L1_THEN_ANGLE, 20 cells, cos 0.2, no Voronoi cell nearer than 0.3 m
    vor_rq = ctx.voronoi_request(origin, dims, ratio, md, min_distance=0.3, mode=KHR_VOR_L1_THEN_ANGLE, parent_l1_separation=20, parent_cos_angle_separation=0.2)

    def distance():
        rc, _ = ctx.distance_field_into(df_rq, dev, on_device=True, want_stats=False)
        assert rc == 0, rc

    def voronoi():
        rc, stats = ctx.voronoi_field_rc(vor_rq)
        assert rc == 0, rc
        return stats

    for _ in range(3):
        distance()
        stats = voronoi()
    ts = {"distance": [], "voronoi": []}
    for _ in range(repeats):
        for what, call in (("distance", distance), ("voronoi", voronoi)):
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            ts[what].append(1e3 * (time.perf_counter() - t0))
    for p in dev.values():
        hip.hipFree(C.c_void_p(p))
    blocks = ctx.num_blocks()
    ctx.close()
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"width": W, "height": H, "voxel_size": s_["voxel_size"], "frames": s_["frames"], "blocks": blocks, "origin": origin, "dims": dims, "cells": n,
            "ratio": ratio, "max_distance": md, "range_cells": int(np.floor(np.float32(md) / np.float32(cell))), "stats": stats,
            "distance_positive_only_ms": {"best": min(ts["distance"]), "median": med["distance"]},
            "voronoi_ms": {"best": min(ts["voronoi"]), "median": med["voronoi"]}, "ratio_of_medians": med["voronoi"] / med["distance"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", nargs="+", default=["stream", "large"], choices=sorted(SETUPS))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace", default=None, help="directory for a kernel trace of a second run")
    a = ap.parse_args()
    res = {"what": "khr_voronoi_field beside khr_distance_field(positive_only = 1)", "repeats": a.repeats}
    for name in a.setups:
        res[name] = run(name, a.repeats)
    if a.trace:
        # one set-up per traced child: the statistics do not tell the boxes apart
        res["kernels"] = {name: kernel_stats(os.path.join(a.trace, name), ["--setups", name, "--repeats", str(a.repeats)]) for name in a.setups}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
