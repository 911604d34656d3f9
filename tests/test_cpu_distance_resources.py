"""-m "not gpu": the compiler's resource report for the distance-field kernels (khr_kernels_distance.h), from
khronos_amd/lib/resource_usage.txt as __graft_entry__.build() writes it: no scratch memory, no spilled VGPRs, LDS within 64 KB."""
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


def test_distance_kernels_stay_in_registers_and_lds():
    sel = {k: v for k, v in _kernels().items() if re.search(r"^_ZN3khr\d+k_df_", k)}
    names = sorted(sel)
    # gather for both block sizes and the three ratios, a pass per axis, the finish
    assert sum("k_df_gatherILi16E" in n for n in names) == 3 and sum("k_df_gatherILi8E" in n for n in names) == 3, names
    assert sum("k_df_passILi" in n for n in names) == 3 and sum("k_df_finish" in n for n in names) == 1, names
    for name, r in sel.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] <= 64 * 1024, (name, r)
    for name in names:
        if "k_df_pass" in name:
            assert sel[name]["LDS Size"] > 0, name   # (the line tile is static: the report sees all of it)
