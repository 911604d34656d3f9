"""Timing of khr_places_graph beside the khr_voronoi_field it reads, on the same boxes, in one process.  Two set-ups, those of
tools/voronoi_timing.py:
  stream  the tests' stream (320x240, 10 cm voxels, 30 frames), 40 x 40 x 24 cells of 2 voxels around the last camera position, range 1.2 m
  large   the C3 geometry of bench.py (1280x720, 2 cm voxels, 20 labels, 40 frames), 256^3 cells of 2 voxels, range 4.5 m
Per set-up: a host clock around each call and the khr_sync that follows -- the Voronoi field once per round, then the places graph at
every `--compressions` value -- best and median of `--repeats` rounds after a warm-up.  Both calls wait for their counters (one wait
and two); the results stay on the device (no *_into in the timed region).
--trace DIR runs the same once more in a child process under a kernel trace (rocprofv3 --kernel-trace --stats --output-format csv) and
adds the per-kernel times of the k_vor_* and k_pl_* kernels and of the library's scan and sort kernels from its statistics.
Prints one JSON line.  From the repository root:  python tools/places_timing.py [--setups stream large] [--trace DIR]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.voronoi_timing import SETUPS  # noqa: E402


def kernel_stats(trace_dir, argv):
    """the k_vor_* / k_pl_* / scan / sort rows of a kernel trace of this script: name -> calls, mean and total microseconds"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "places", "--", sys.executable, os.path.abspath(__file__)] + argv
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            short = None
            for tag in ("k_df_", "k_vor_", "k_pl_"):
                if tag in name:
                    short = name[name.index(tag):].split("(")[0]
            if short is None and "rocprim" in name:
                short = "rocprim:" + ("radix_sort" if "radix" in name or "sort" in name else "scan" if "scan" in name else "other")
            if short is None:
                continue
            e = out.setdefault(short, {"calls": 0, "total_us": 0.0})
            e["calls"] += int(row["Calls"])
            e["total_us"] += float(row["TotalDurationNs"]) * 1e-3
    for e in out.values():
        e["mean_us"] = e["total_us"] / max(e["calls"], 1)
    return out


def run(name, repeats, compressions):
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
    # the reference's values: L1_THEN_ANGLE, 20 cells, cos 0.2, no Voronoi cell nearer than 0.3 m; places no nearer than 0.4 m,
    # components of at least 3 places
    vor_rq = ctx.voronoi_request(origin, dims, ratio, md, min_distance=0.3, mode=KHR_VOR_L1_THEN_ANGLE, parent_l1_separation=20, parent_cos_angle_separation=0.2)
    pl_rq = {c: ctx.places_request(min_node_distance=0.4, compression=c, min_component_size=3) for c in compressions}

    def voronoi():
        rc, stats = ctx.voronoi_field_rc(vor_rq)
        assert rc == 0, rc
        return stats

    def places(c):
        rc, stats = ctx.places_graph_rc(pl_rq[c])
        assert rc == 0, rc
        return stats

    stats = {}
    for _ in range(3):
        stats["voronoi"] = voronoi()
        for c in compressions:
            stats[c] = places(c)
    ts = {"voronoi": [], **{c: [] for c in compressions}}
    for _ in range(repeats):
        for what, call in [("voronoi", voronoi)] + [(c, (lambda c=c: places(c))) for c in compressions]:
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            ts[what].append(1e3 * (time.perf_counter() - t0))
    blocks = ctx.num_blocks()
    ctx.close()
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"width": W, "height": H, "voxel_size": s_["voxel_size"], "frames": s_["frames"], "blocks": blocks, "origin": origin, "dims": dims,
            "cells": int(np.prod(dims)), "ratio": ratio, "max_distance": md, "voronoi_stats": stats["voronoi"],
            "voronoi_ms": {"best": min(ts["voronoi"]), "median": med["voronoi"]},
            "places": {str(c): {"stats": stats[c], "ms": {"best": min(ts[c]), "median": med[c]}, "ratio_of_medians": med[c] / med["voronoi"]} for c in compressions}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", nargs="+", default=["stream", "large"], choices=sorted(SETUPS))
    ap.add_argument("--compressions", nargs="+", type=int, default=[1, 7, 16])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace", default=None, help="directory for a kernel trace of a second run")
    a = ap.parse_args()
    res = {"what": "khr_places_graph beside khr_voronoi_field", "repeats": a.repeats}
    for name in a.setups:
        res[name] = run(name, a.repeats, a.compressions)
    if a.trace:
        # one set-up per traced child: the statistics do not tell the boxes apart
        res["kernels"] = {name: kernel_stats(os.path.join(a.trace, name), ["--setups", name, "--repeats", str(a.repeats), "--compressions"] + [str(c) for c in a.compressions])
                          for name in a.setups}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
