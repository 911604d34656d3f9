"""khr_distance_field's buffers -- the two work grids, the counters, the host form's staging pair -- have owners: the four counts of
khr_debug_live_resources rise while a context that answered a host-form and a device-form call lives, and return to where they were
after close() (tests/test_gpu_resource_lifetime.py explains the counts)."""
import gc

import numpy as np
import pytest

import distance_cases as dc
import mesh_cases as mc
from common import DeviceArray
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import live_resources

pytestmark = pytest.mark.gpu


def test_a_context_that_answered_distance_fields_leaves_nothing():
    gc.collect()
    start = live_resources()
    cfg = default_config(voxels_per_side=16, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
    ctx = FusionContext(cfg)
    created = live_resources()
    indices, layers = dc.wall(16)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    before = live_resources()
    origin, dims = dc.box_of("wall", 16, 1)
    host = ctx.distance_field(origin, dims, 1, max_distance=0.55)
    assert host["stats"]["n_obstacle"] > 0
    n = int(np.prod(dims))
    d = DeviceArray(np.zeros(n, np.float32))
    rc, stats = ctx.distance_field_into(ctx.df_request(origin, dims, 1, max_distance=0.55), {"distance": d.data_ptr()}, on_device=True)
    assert rc == 0 and stats == host["stats"]
    assert d.read(0, 4 * n).tobytes() == host["distance"].tobytes()
    d.free()
    now = live_resources()
    assert all(c > s for c, s in zip(created, start)), (start, created)
    # two work grids, the counters, the device staging; its page-locked mirror
    assert now[0] >= before[0] + 4 and now[1] >= before[1] + 1 and all(a > b for a, b in zip(now, start)), (start, before, now)
    # a larger box grows the grids and the staging in place: no further owners
    ctx.distance_field((origin[0] - 8, origin[1] - 8, origin[2] - 8), tuple(v + 16 for v in dims), 1, max_distance=0.55)
    assert live_resources() == now
    ctx.close()
    assert live_resources() == start
