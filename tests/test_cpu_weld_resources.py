"""-m "not gpu": the kernels of khr_weld_mesh (khronos_amd/csrc/khr_kernels_weld.h) carry no scratch memory and spill nothing, in
either instantiation of the insert, as the compiler reports it (khronos_amd/lib/resource_usage.txt, written by
__graft_entry__.build())."""
import re

import pytest

from test_cpu_query_resources import _kernels

KERNELS = ("k_weld_clear", "k_weld_block_counts", "k_weld_insert", "k_weld_resolve", "k_weld_vertices", "k_weld_face_flags", "k_weld_faces")


@pytest.mark.parametrize("kernel", KERNELS)
def test_weld_kernels_use_no_scratch_and_spill_nothing(kernel):
    sel = {k: v for k, v in _kernels().items() if re.match(r"^_ZN3khr%d%s(E|I)" % (len(kernel), kernel), k)}
    assert len(sel) == (2 if kernel == "k_weld_insert" else 1), sorted(sel)   # (the insert: with and without the wave-level merge)
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 0, (name, r)
