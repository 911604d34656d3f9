"""-m "not gpu": the kernels of khr_segment_map (khronos_amd/csrc/khr_kernels_segment.h) carry no scratch memory and spill nothing,
in any instantiation, as the compiler reports it (khronos_amd/lib/resource_usage.txt, written by __graft_entry__.build())."""
import re

import pytest

from test_cpu_query_resources import _kernels

# per kernel its instantiations: voxels_per_side 8 and 16; k_seg_reduce also with and without the voxel list; k_seg_count and
# k_seg_flag work on node ids alone
KERNELS = {"k_seg_local": 2, "k_seg_seams": 2, "k_seg_count": 1, "k_seg_flag": 1, "k_seg_heads": 2, "k_seg_reduce": 4, "k_seg_emit": 2}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_segment_kernels_use_no_scratch_and_spill_nothing(kernel):
    sel = {k: v for k, v in _kernels().items() if re.match(r"^_ZN3khr%d%s(E|I)" % (len(kernel), kernel), k)}
    assert len(sel) == KERNELS[kernel], sorted(sel)
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)


def test_every_segment_kernel_is_listed():
    seen = {m.group(1) for k in _kernels() for m in [re.match(r"^_ZN3khr\d+(k_seg_[a-z]+)(E|I)", k)] if m}
    assert seen == set(KERNELS), seen
