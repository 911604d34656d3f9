"""-m "not gpu": the kernels of khr_diff_map (khronos_amd/csrc/khr_kernels_diff.h) carry no scratch memory and spill nothing, in any
instantiation (voxels_per_side, mode), as the compiler reports it (khronos_amd/lib/resource_usage.txt, written by
__graft_entry__.build())."""
import re

import pytest

from test_cpu_query_resources import _kernels

KERNELS = {"k_diff_count": 4, "k_diff_block_counts": 1, "k_diff_emit": 4}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_diff_kernels_use_no_scratch_and_spill_nothing(kernel):
    sel = {k: v for k, v in _kernels().items() if re.match(r"^_ZN3khr%d%s(E|I)" % (len(kernel), kernel), k)}
    assert len(sel) == KERNELS[kernel], sorted(sel)  # (templates: voxels_per_side 8 and 16, and the two modes)
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
