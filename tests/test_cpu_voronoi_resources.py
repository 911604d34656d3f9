"""-m "not gpu": the compiler's resource report for the Voronoi-field kernels (khr_kernels_voronoi.h), from
khronos_amd/lib/resource_usage.txt as __graft_entry__.build() writes it: no scratch memory, no spilled VGPRs, LDS within 64 KB --
the key tile of a pass is exactly that, static, so the report sees all of it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "khronos_amd", "lib", "resource_usage.txt")


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


def test_voronoi_kernels_stay_in_registers_and_lds():
    sel = {k: v for k, v in _kernels().items() if re.search(r"^_ZN3khr\d+k_vor_", k)}
    names = sorted(sel)
    # a pass per axis, the classification, the list
    assert sum("k_vor_passILi" in n for n in names) == 3 and sum("k_vor_classify" in n for n in names) == 1 and sum("k_vor_emit" in n for n in names) == 1, names
    assert len(names) == 5, names
    for name, r in sel.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] <= 64 * 1024, (name, r)
        if "k_vor_pass" in name:
            assert r["LDS Size"] > 0, name
