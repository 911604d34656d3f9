"""Save / load timing of a map checkpoint (khr_checkpoint_save / khr_checkpoint_load) at the C3 geometry of bench.py: 1280x720,
2 cm voxels, 20 labels.  Fuses `--frames` frames of the synthetic stream, then measures, in this one process:
  * the save into page-locked and into pageable host memory (time, bytes, GB/s),
  * the only whole-map read the library offered before: a khr_download_block loop over khr_block_indices,
  * the load into a fresh context from page-locked and from pageable memory,
  * the page-locked host-to-device copy rate of the same number of bytes (the link's bound for the load).
Prints one JSON line.  From the repository root:  python tools/checkpoint_timing.py [--frames 40]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from khronos_amd import FusionContext, default_config  # noqa: E402
from khronos_amd.synth import SyntheticStream  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--voxel-size", type=float, default=0.02)
    ap.add_argument("--max-blocks", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
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
    nbytes, nblocks = ctx.checkpoint_size()
    hip = C.CDLL("libamdhip64.so")
    pin = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(pin), C.c_size_t(nbytes), C.c_uint(0)) == 0
    pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(nbytes,))
    pageable = np.zeros(nbytes, np.uint8)

    def best(f):
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return min(ts)

    res = {"what": "map checkpoint timing", "width": W, "height": H, "voxel_size": a.voxel_size, "num_labels": 20, "frames": a.frames,
           "blocks": nblocks, "bytes": nbytes, "pool_blocks": a.max_blocks}
    for name, buf in (("save_pinned", pinned), ("save_pageable", pageable)):
        ctx.save_map(out=buf)  # (first call: staging allocation)
        t = best(lambda: ctx.save_map(out=buf))
        res[name + "_ms"], res[name + "_GBps"] = 1e3 * t, nbytes / t / 1e9
    assert pinned.tobytes() == pageable.tobytes()
    idx = ctx.block_indices()
    t0 = time.perf_counter()
    for b in idx:
        ctx.download_block(b)
    t = time.perf_counter() - t0
    res["download_block_loop_ms"], res["download_block_loop_GBps"] = 1e3 * t, nbytes / t / 1e9
    want = ctx.map_digest()
    dst = FusionContext(cfg)
    for name, buf in (("load_pinned", pinned), ("load_pageable", pageable)):
        ts = []
        for _ in range(a.repeats + 1):
            dst.reset_map(cfg.voxel_size, cfg.truncation_distance)
            dst.sync()
            t0 = time.perf_counter()
            kept = dst.load_map(buf)
            ts.append(time.perf_counter() - t0)
            assert kept == nblocks
        assert [int(x) for x in dst.map_digest()] == [int(x) for x in want]
        t = min(ts[1:])
        res[name + "_ms"], res[name + "_GBps"] = 1e3 * t, nbytes / t / 1e9
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes)) == 0
    for name, kind, (to, frm) in (("h2d_pinned_copy", 1, (dev, pin)), ("d2h_pinned_copy", 2, (pin, dev))):
        hip.hipMemcpy(to, frm, C.c_size_t(nbytes), kind)
        t = best(lambda: hip.hipMemcpy(to, frm, C.c_size_t(nbytes), kind))
        res[name + "_ms"], res[name + "_GBps"] = 1e3 * t, nbytes / t / 1e9
    hip.hipFree(dev)
    hip.hipHostFree(pin)
    res["staging_device_bytes"] = 2 * (32 << 20)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
