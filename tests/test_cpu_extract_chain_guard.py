"""-m "not gpu": the kernels of the object extractor's fused call sequence (khr_begin_object_map, khr_integrate_prune_batch), read
from the compiler's report (khronos_amd/lib/resource_usage.txt, written by __graft_entry__.build()) the way
tests/test_cpu_object_update_guard.py reads it: the set-up kernel and the ordering kernel compile without scratch, and the pruning
epilogue has not pushed k_fuse_obj -- which now carries a third argument block -- out of its budget."""
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


@pytest.mark.parametrize("kernel", ["_ZN3khr11k_setup_boxE", "_ZN3khr13k_multi_orderE", "_ZN3khr14k_mesh_prepareE", "_ZN3khr11k_reset_mapE"])
def test_chain_kernels_compile_without_scratch(kernel):
    sel = {n: r for n, r in _kernels().items() if n.startswith(kernel)}
    assert len(sel) == 1, (kernel, sorted(sel))
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)


def test_k_fuse_obj_prunes_within_its_budget():
    """two instantiations (the pruning is a run-time switch in an argument block of its own: NS_9FusePruneE in the mangled name),
    no scratch, at most 128 VGPRs"""
    sel = {n: r for n, r in _kernels().items() if re.search(r"^_ZN3khr10k_fuse_objI", n)}
    assert len(sel) == 2, sorted(sel)
    for name, r in sel.items():
        assert "FusePrune" in name, name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] <= 128 and r["Occupancy"] >= 4, (name, r)
