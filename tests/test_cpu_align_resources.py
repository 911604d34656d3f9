"""-m "not gpu": k_align_linearize keeps its working set -- the 32 (distance, weight) pairs of a point's neighbourhood, the Jacobian and
one product at a time -- in registers: no scratch memory and no spills in any of its four instantiations, as the compiler reports
it (khronos_amd/lib/resource_usage.txt, written by __graft_entry__.build())."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "khronos_amd", "lib", "resource_usage.txt")


def _kernels():
    if not os.path.exists(PATH):
        pytest.skip("khronos_amd/lib/resource_usage.txt is written by __graft_entry__.build() when it compiles the HIP library")
    out, cur = {}, None
    for ln in open(PATH):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def test_k_align_linearize_uses_no_scratch_and_spills_nothing():
    sel = {k: v for k, v in _kernels().items() if re.search(r"^_ZN3khr17k_align_linearizeILi(16|8)ELi(0|1)EEE", k)}
    assert len(sel) == 4, sorted(sel)
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] <= 128, (name, r)  # (four waves per SIMD)
