"""Timing of khr_travel_field beside the khr_voronoi_field it reads, on the same boxes, in one process.  Two set-ups, those of
tools/voronoi_timing.py:
  stream  the tests' stream (320x240, 10 cm voxels, 30 frames), 40 x 40 x 24 cells of 2 voxels around the last camera position, range 1.2 m
  large   the C3 geometry of bench.py (1280x720, 2 cm voxels, 20 labels, 40 frames), 256^3 cells of 2 voxels, range 4.5 m
Per set-up: a host clock around each call and the khr_sync that follows -- the Voronoi field and the places graph once per round, then
the travel field at connectivity 6 and 26 from one goal (the camera's cell) and from the centres of the kept places -- best and median
of `--repeats` rounds after a warm-up, with n_rounds and n_waits of each.  The calls wait for their counters themselves; the results
stay on the device (no *_into in the timed region; the place centres are fetched once, before it).
--trace DIR runs the same once more in a child process under a kernel trace (rocprofv3 --kernel-trace --stats --output-format csv) and
adds the per-kernel times of the k_vor_* and k_tf_* kernels from its statistics.
Prints one JSON line.  From the repository root:  python tools/travel_timing.py [--setups stream large] [--trace DIR]"""
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
    """the k_df_* / k_vor_* / k_tf_* rows of a kernel trace of this script: name -> calls, mean and total microseconds"""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "travel", "--", sys.executable, os.path.abspath(__file__)] + argv
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            short = None
            for tag in ("k_df_", "k_vor_", "k_tf_"):
                if tag in name:
                    short = name[name.index(tag):].split("(")[0]
            if short is None:
                continue
            e = out.setdefault(short, {"calls": 0, "total_us": 0.0})
            e["calls"] += int(row["Calls"])
            e["total_us"] += float(row["TotalDurationNs"]) * 1e-3
    for e in out.values():
        e["mean_us"] = e["total_us"] / max(e["calls"], 1)
    return out


def run(name, repeats, connectivities, clearance):
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
    camera = [int(np.floor(t[k] / cell)) for k in range(3)]
    origin = tuple(camera[k] - dims[k] // 2 for k in range(3))
    # the reference's values: L1_THEN_ANGLE, 20 cells, cos 0.2, no Voronoi cell nearer than 0.3 m; places no nearer than 0.4 m,
    # components of at least 3 places, compression 1.5 m
    vor_rq = ctx.voronoi_request(origin, dims, ratio, md, min_distance=0.3, mode=KHR_VOR_L1_THEN_ANGLE, parent_l1_separation=20, parent_cos_angle_separation=0.2)
    pl_rq = ctx.places_request(min_node_distance=0.4, compression=max(1, min(16, int(1.5 / cell))), min_component_size=3)

    def voronoi():
        rc, stats = ctx.voronoi_field_rc(vor_rq)
        assert rc == 0, rc
        rc, _ = ctx.places_graph_rc(pl_rq)   # (not timed: the travel field does not read it)
        assert rc == 0, rc
        return stats

    voronoi()
    goals = {"one": np.asarray([camera], np.int32), "places": ctx.places_centres()}
    goals = {k: g for k, g in goals.items() if len(g)}
    cases = [(g, c) for g in goals for c in connectivities]
    rqs = {c: ctx.travel_request(clearance, c) for c in connectivities}

    def travel(g, c):
        rc, stats = ctx.travel_field_rc(rqs[c], goals[g])
        assert rc == 0, rc
        return stats

    stats = {}
    for _ in range(3):
        stats["voronoi"] = voronoi()
        for g, c in cases:
            stats[(g, c)] = travel(g, c)
    ts = {"voronoi": [], **{k: [] for k in cases}}
    for _ in range(repeats):
        ctx.sync()
        t0 = time.perf_counter()
        rc, _ = ctx.voronoi_field_rc(vor_rq)
        ctx.sync()
        ts["voronoi"].append(1e3 * (time.perf_counter() - t0))
        assert rc == 0, rc
        for g, c in cases:
            ctx.sync()
            t0 = time.perf_counter()
            travel(g, c)
            ctx.sync()
            ts[(g, c)].append(1e3 * (time.perf_counter() - t0))
    blocks = ctx.num_blocks()
    ctx.close()
    med = {k: statistics.median(v) for k, v in ts.items()}
    return {"width": W, "height": H, "voxel_size": s_["voxel_size"], "frames": s_["frames"], "blocks": blocks, "origin": origin, "dims": dims,
            "cells": int(np.prod(dims)), "ratio": ratio, "max_distance": md, "clearance": clearance, "voronoi_stats": stats["voronoi"],
            "voronoi_ms": {"best": min(ts["voronoi"]), "median": med["voronoi"]},
            "travel": {"%s/%d" % k: {"n_goals": int(len(goals[k[0]])), "stats": stats[k], "ms": {"best": min(ts[k]), "median": med[k]},
                                     "ratio_of_medians": med[k] / med["voronoi"]} for k in cases}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", nargs="+", default=["stream", "large"], choices=sorted(SETUPS))
    ap.add_argument("--connectivities", nargs="+", type=int, default=[6, 26])
    ap.add_argument("--clearance", type=float, default=0.3, help="metres")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace", default=None, help="directory for a kernel trace of a second run")
    a = ap.parse_args()
    res = {"what": "khr_travel_field beside khr_voronoi_field", "repeats": a.repeats}
    for name in a.setups:
        res[name] = run(name, a.repeats, a.connectivities, a.clearance)
    if a.trace:
        # one set-up per traced child: the statistics do not tell the boxes apart
        res["kernels"] = {name: kernel_stats(os.path.join(a.trace, name), ["--setups", name, "--repeats", str(a.repeats), "--clearance", str(a.clearance), "--connectivities"] +
                                             [str(c) for c in a.connectivities]) for name in a.setups}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
