"""-m "not gpu": the kernels of khr_merge_map (khronos_amd/csrc/khr_kernels_merge.h) carry no scratch memory and spill nothing, in
any instantiation (voxels_per_side, mode), as the compiler reports it (khronos_amd/lib/resource_usage.txt, written by
__graft_entry__.build())."""
import re

import pytest

from test_cpu_query_resources import _kernels

KERNELS = {"k_merge_candidates": 2, "k_merge_probe": 4, "k_merge_insert": 1, "k_merge_rows": 4, "k_merge_attributes": 4, "k_merge_apply": 4}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_merge_kernels_use_no_scratch_and_spill_nothing(kernel):
    sel = {k: v for k, v in _kernels().items() if re.match(r"^_ZN3khr%d%s(E|I)" % (len(kernel), kernel), k)}
    assert len(sel) == KERNELS[kernel], sorted(sel)  # (templates: voxels_per_side 8 and 16, and the two modes)
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
