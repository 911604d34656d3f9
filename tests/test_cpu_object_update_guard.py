"""-m "not gpu": the budgets of the object mini-map's multi-frame update kernel (k_fuse_obj), read from the compiler's report
(khronos_amd/lib/resource_usage.txt, written by __graft_entry__.build()) the way tests/test_cpu_resource_guard.py reads it.  The kernel
keeps a voxel's whole state in registers across the frames of a launch: a spill would put memory traffic back into the frame loop."""
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


def test_k_fuse_obj_budget():
    """both arithmetic modes: no scratch, at most 128 VGPRs = 4 waves per SIMD, and no more LDS than the k_fuse2<8, ..>
    instantiations it replaces for the extractor (their per-wave record lists are gone: what is left are the queue and statistics words)"""
    k = _kernels()
    sel = {n: r for n, r in k.items() if re.search(r"^_ZN3khr10k_fuse_objI", n)}
    assert len(sel) == 2, sorted(sel)
    old = {n: r for n, r in k.items() if re.search(r"^_ZN3khr7k_fuse2ILi8E", n)}
    assert old, "k_fuse2<8, ..> instantiations"
    lds_old = min(r["LDS Size"] for r in old.values())
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] <= 128 and r["Occupancy"] >= 4, (name, r)
        assert r["LDS Size"] <= lds_old, (name, r, lds_old)
