"""khr_configure_object_voxel_sets: declared in the C header, exported by the library, bound in Python (no GPU needed)."""
import ctypes as C
import os
import re

from khronos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    name = "khr_configure_object_voxel_sets"
    assert name in capi.EXPORTS
    assert not re.search(r"\d", name)  # (the header / export comparison of test_cpu_oracle.py only sees names without digits)
    hdr = open(os.path.join(ROOT, "include", "khronos_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*khr_ctx\s*\*\s*\w+\s*,\s*float\s+voxel_size\s*\)\s*;" % name, hdr)
    lib = capi.load_library()
    fn = getattr(lib, name)
    assert fn.argtypes == [C.c_void_p, C.c_float]
    assert fn(None, 0.2) < 0  # a null context is an error, not a crash
    for method in ("configure_object_voxel_sets", "cluster_voxels_launch", "cluster_voxels_fetch"):
        assert callable(getattr(capi.FusionContext, method))
