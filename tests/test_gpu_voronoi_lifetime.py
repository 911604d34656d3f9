"""khr_voronoi_field's buffers -- the key grid, the dense outputs, the scan's storage, the list, the counters with their page-locked
mirror, the page-locked staging of the host form -- have owners: the counts of khr_debug_live_resources rise with the first call,
stay put when a larger box grows the buffers in place, and return to where they were after close() (tests/test_gpu_resource_lifetime.py
explains the counts)."""
import gc

import numpy as np
import pytest

import distance_cases as dc
import mesh_cases as mc
from common import DeviceArray
from khronos_amd import FusionContext, checkpoint as ck, default_config
from khronos_amd.capi import KHR_VOR_L1, live_resources

pytestmark = pytest.mark.gpu


def test_a_context_that_answered_voronoi_fields_leaves_nothing():
    gc.collect()
    start = live_resources()
    cfg = default_config(voxels_per_side=16, max_blocks=256, max_frame_pixels=64 * 48, exact_arithmetic=1, **mc.CONFIG)
    ctx = FusionContext(cfg)
    indices, layers = dc.random(16)
    assert ctx.load_map(ck.pack(cfg, indices, layers)) == len(indices)
    before = live_resources()
    origin, _ = dc.box_of("random", 16, 1)
    dims = (20, 12, 16)
    kw = dict(max_distance=100.0, min_distance=0.2, mode=KHR_VOR_L1, parent_l1_separation=4)
    host = ctx.voronoi_field(origin, dims, 1, **kw)
    assert host["stats"]["n_listed"] > 0
    n = int(np.prod(dims))
    d = DeviceArray(np.zeros(n, np.int32))
    assert ctx.voronoi_field_into({"site": d.data_ptr()}, on_device=True) == 0
    ctx.sync()
    assert d.read(0, 4 * n).tobytes() == host["site"].tobytes()
    d.free()
    now = live_resources()
    # the seed grid, the keys, the dense outputs, the scan's storage, the list, the counters; their mirror and the host staging
    assert now[0] >= before[0] + 6 and now[1] >= before[1] + 2 and now[2:] == before[2:], (start, before, now)
    # a larger box, with a longer list, grows all of them in place: no further owners
    larger = ctx.voronoi_field(tuple(o - 8 for o in origin), tuple(v + 16 for v in dims), 1, **kw)
    assert larger["stats"]["n_listed"] > host["stats"]["n_listed"]
    assert live_resources() == now
    # an empty list keeps its owner too
    assert ctx.voronoi_field(origin, (3, 3, 3), 1, max_distance=1.0, min_distance=10.0)["stats"]["n_listed"] == 0
    assert live_resources() == now
    ctx.close()
    assert live_resources() == start
