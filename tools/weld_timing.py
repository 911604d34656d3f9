"""Timing of khr_weld_mesh / khr_weld_mesh_into at the C3 geometry of bench.py: 1280x720, 2 cm voxels, 20 labels.  Fuses `--frames`
frames of the synthetic stream with the window's output cadence (meshing + archival every fourth frame) and takes the mesh of the
last output.  Measured in this one process, the device drained before each call, `--repeats` calls after a warm-up, median with
minimum and maximum:
  * khr_weld_mesh alone, with the wave-level key merge and without it (KHR_WELD_MERGE=0), the two interleaved;
  * khr_weld_mesh + khr_weld_mesh_into to host arrays, and to device arrays (+ khr_sync);
  * what exists without the weld: khr_fetch_mesh + khr_fetch_mesh_into (the soup to the host), to which a consumer adds its own weld.
The one-thread host weld itself is timed by `aw_demo --weld` (C++, a first-come unordered_map) over the window's mesh of the same
geometry (tools/aw_c3.yaml); its JSON line is embedded under "aw_demo".  Bytes that cross to the host are listed for both ways.
Prints one JSON line.  From the repository root:  python tools/weld_timing.py [--frames 40]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ts):
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--voxel-size", type=float, default=0.02)
    ap.add_argument("--resolution", type=float, default=0.0, help="metres; 0 = the voxel size")
    ap.add_argument("--max-blocks", type=int, default=40960)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-demo", action="store_true", help="skip the aw_demo --weld run")
    a = ap.parse_args()
    r = a.resolution if a.resolution > 0 else a.voxel_size
    res = {"what": "khr_weld_mesh timing", "width": a.width, "height": a.height, "voxel_size": a.voxel_size, "resolution": r,
           "frames": a.frames, "repeats": a.repeats}
    if not a.no_demo:   # (before this process opens the device: one process at a time is timed)
        demo = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")
        out = subprocess.run([demo, "--weld", os.path.join(ROOT, "tools", "aw_c3.yaml"), str(a.width), str(a.height), str(a.frames), repr(r),
                              str(a.repeats)], capture_output=True, text=True, timeout=900)
        res["aw_demo"] = json.loads(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else {"returncode": out.returncode,
                                                                                                     "stderr": out.stderr[-400:]}
    from khronos_amd import FusionContext, default_config
    from khronos_amd.synth import SyntheticStream
    W, H = a.width, a.height
    cfg = default_config(voxel_size=a.voxel_size, truncation_distance=3 * a.voxel_size, with_semantics=1, with_tracking=1, num_labels=20,
                         max_blocks=a.max_blocks, max_frame_pixels=W * H, max_mesh_vertices=1 << 23)
    ctx = FusionContext(cfg)
    s = SyntheticStream(W, H)
    sen = ctx.make_sensor(W, H, s.fx, s.fy, s.cx, s.cy)
    for i in range(a.frames):
        fr = s.render(i)
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        ctx.integrate(slot)
        ctx.update_tracking(fr["stamp"])
        if i % 4 == 3:
            ctx.generate_mesh(True, True)
            ctx.reset_inactive()
            ctx.clear_updated()
    ctx.sync()
    first = ctx.weld_mesh(r)
    st = first["stats"]
    ns, nv, nf = st["n_soup_vertices"], st["n_vertices"], st["n_faces"]
    res.update(stats=st, blocks=ctx.num_blocks(),
               bytes={"soup_to_host": 36 * ns, "indexed_to_host": 36 * nv + 12 * nf, "soup_to_vertex": 4 * ns})
    host = {k: np.zeros_like(first[k]) for k, _, _, _ in ctx.WELD_FIELDS}
    no_map = {k: v for k, v in host.items() if k != "soup_to_vertex"}
    hip = C.CDLL("libamdhip64.so")
    dev = {}
    for k, v in host.items():
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(v.nbytes, 16))) == 0
        dev[k] = p.value

    def weld_only():
        assert ctx.lib.khr_weld_mesh(ctx.h, r, None) == 0

    def weld_host():
        weld_only()
        assert ctx.weld_mesh_into(host) == 0

    def weld_host_no_map():
        weld_only()
        assert ctx.weld_mesh_into(no_map) == 0

    def weld_device():
        weld_only()
        assert ctx.weld_mesh_into(dev, on_device=True) == 0
        ctx.sync()

    bufs = {}

    def fetch_soup():
        assert ctx.fetch_mesh_reuse(bufs) == ns

    def timed(fn, env=None):
        old = os.environ.get("KHR_WELD_MERGE")
        if env is not None:
            os.environ["KHR_WELD_MERGE"] = env
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        dt = 1e3 * (time.perf_counter() - t0)
        if env is not None:
            if old is None:
                del os.environ["KHR_WELD_MERGE"]
            else:
                os.environ["KHR_WELD_MERGE"] = old
        return dt

    runs = {"weld_merge": (weld_only, "1"), "weld_no_merge": (weld_only, "0"), "weld_into_host": (weld_host, None),
            "weld_into_host_without_soup_to_vertex": (weld_host_no_map, None), "weld_into_device": (weld_device, None),
            "fetch_soup_to_host": (fetch_soup, None)}
    ts = {k: [] for k in runs}
    for rep in range(a.repeats + 3):   # the variants interleaved, so that drift of the machine reaches all of them alike
        for k, (fn, env) in runs.items():
            dt = timed(fn, env)
            if rep >= 3:
                ts[k].append(dt)
    for k in runs:
        res[k] = spread(ts[k])
    for p in dev.values():
        hip.hipFree(C.c_void_p(p))
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
