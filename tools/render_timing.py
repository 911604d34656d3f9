"""Timing of khr_render_view at the C3 geometry of bench.py: 1280x720, 2 cm voxels, 20 labels.  Fuses `--frames` frames of the
synthetic stream, then renders the map at the last frame's own pose (step_voxels 0.5) and measures, in this one process:
  * the whole call in the device form (images into device memory, counters requested: one host wait) and in the host form
    (staging + page-locked mirror + copies into the caller's arrays); best and median of `--repeats` calls after a warm-up,
  * the share of the samples the march visited.
Kernel time comes from a separate run under a kernel trace.  --library names another build of libkhronos_amd.so (the
-DKHR_RENDER_NO_SKIP build of the A/B measurement; both builds must give the same images: --digest prints them).
Prints one JSON line.  From the repository root:  python tools/render_timing.py [--frames 40]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from khronos_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--voxel-size", type=float, default=0.02)
    ap.add_argument("--max-blocks", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-voxels", type=float, default=0.5)
    ap.add_argument("--library", default=None)
    a = ap.parse_args()
    if a.library:
        capi.LIB_PATH = os.path.abspath(a.library)
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
    rq = ctx.render_request(sen, fr["pose"], a.step_voxels)
    host = {n: np.zeros((H, W) + sh, dt) for n, dt, sh in ctx.RENDER_FIELDS}
    hip = C.CDLL("libamdhip64.so")
    dev = {}
    for n, arr in host.items():
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(arr.nbytes)) == 0
        dev[n] = p.value

    def timed(out, on_device):
        for _ in range(3):
            rc, stats = ctx.render_view_into(rq, out, on_device=on_device)
            assert rc == 0
        ts = []
        for _ in range(a.repeats):
            ctx.sync()
            t0 = time.perf_counter()
            rc, stats = ctx.render_view_into(rq, out, on_device=on_device)
            ts.append(1e3 * (time.perf_counter() - t0))
        return min(ts), statistics.median(ts), stats

    res = {"what": "khr_render_view timing", "library": a.library or "shipped", "width": W, "height": H, "voxel_size": a.voxel_size,
           "frames": a.frames, "blocks": ctx.num_blocks(), "step_voxels": a.step_voxels}
    res["device_form_ms_best"], res["device_form_ms_median"], stats = timed(dev, True)
    res["host_form_ms_best"], res["host_form_ms_median"], stats = timed(host, False)
    res.update(stats)
    res["evaluated_share"] = stats["n_samples_evaluated"] / stats["n_samples_total"]
    res["image_sha1"] = {n: hashlib.sha1(arr.tobytes()).hexdigest()[:16] for n, arr in host.items()}
    for p in dev.values():
        hip.hipFree(C.c_void_p(p))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
