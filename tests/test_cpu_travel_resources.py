"""-m "not gpu": the compiler's resource report for the travel-field kernels (khr_kernels_travel.h), from
khronos_amd/lib/resource_usage.txt as __graft_entry__.build() writes it: no scratch memory, no spilled VGPRs, and the relaxation
kernel's LDS -- a tile of 8^3 keys with its halo, static, so the report sees all of it -- within the 10 KB DESIGN.md states."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "khronos_amd", "lib", "resource_usage.txt")
EXPECTED = ["k_tf_seed", "k_tf_relaxILi6E", "k_tf_relaxILi18E", "k_tf_relaxILi26E", "k_tf_finishILi6E", "k_tf_finishILi18E", "k_tf_finishILi26E",
            "k_tf_path_count", "k_tf_path_emit"]


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


def test_travel_kernels_stay_in_registers_and_lds():
    sel = {k: v for k, v in _kernels().items() if re.search(r"^_ZN3khr\d+k_tf_", k)}
    names = sorted(sel)
    assert len(names) == len(EXPECTED) and all(sum(e in n for n in names) == 1 for e in EXPECTED), names
    for name, r in sel.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        if "k_tf_relax" in name:
            # 10^3 keys of 8 bytes and a word: LDS never limits the workgroups of a CU (160 KB)
            assert 8000 <= r["LDS Size"] <= 10 * 1024, (name, r)
            assert r["Occupancy"] >= 4, (name, r)
        else:
            assert r["LDS Size"] == 0, (name, r)
