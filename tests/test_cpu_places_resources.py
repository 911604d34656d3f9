"""-m "not gpu": the compiler's resource report for the places-graph kernels (khr_kernels_places.h), from
khronos_amd/lib/resource_usage.txt as __graft_entry__.build() writes it: no scratch memory, no spilled VGPRs, LDS within 64 KB --
the labelling kernel's parent words, roots and per-place slots are static, so the report sees all of them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "khronos_amd", "lib", "resource_usage.txt")
EXPECTED = ["k_pl_label", "k_pl_pairsILi0", "k_pl_pairsILi1", "k_pl_edge_heads", "k_pl_edge_reduce", "k_pl_comp_union", "k_pl_comp_flatten",
            "k_pl_comp_keep", "k_pl_finish_cells", "k_pl_finish_edges"]


def _kernels():
    assert os.path.exists(PATH), "khronos_amd/lib/resource_usage.txt is written by __graft_entry__.build()"
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


def test_places_kernels_stay_in_registers_and_lds():
    sel = {k: v for k, v in _kernels().items() if re.search(r"^_ZN3khr\d+k_pl_", k)}
    names = sorted(sel)
    assert len(names) == len(EXPECTED) and all(sum(e in n for n in names) == 1 for e in EXPECTED), names
    for name, r in sel.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] <= 64 * 1024, (name, r)
        if "k_pl_label" in name:
            # 16 KB of parent words, 8 KB of roots, two 8 KB slot tables: three workgroups share a CU's 160 KB
            assert 0 < r["LDS Size"] <= 48 * 1024, (name, r)
