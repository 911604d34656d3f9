"""-m "not gpu": the owner types of khronos_amd/csrc/khr_owned.h, checked by a stand-alone program (tests/owned_selftest.cpp).
Without a HIP device every allocation fails, which is what the program then checks: the error code, an empty object, live counts
of zero; moves, repeated resets and a referred-to stream need no device at all."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_types_selftest(tmp_path):
    exe = tmp_path / "owned_selftest"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", str(exe),
                        os.path.join(ROOT, "tests", "owned_selftest.cpp"), "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                        "-Wl,-rpath," + os.path.join(rocm, "lib")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "owned selftest ok" in out.stdout


def test_runtime_allocation_calls_occur_only_in_the_owners():
    """khr_debug_live_resources counts what the owners hold, so a raw hipHostMalloc kept in a raw member would leak unseen by
    tests/test_gpu_resource_lifetime.py.  This closes that gap by reading: outside khr_owned.h no code of csrc/ calls the
    allocate / create / free / destroy functions of the runtime (comments and string literals may name them)."""
    import re
    csrc = os.path.join(ROOT, "khronos_amd", "csrc")
    calls = re.compile(r"\b(hipMalloc\w*|hipFree\w*|hipHostMalloc|hipHostAlloc|hipHostFree|hipHostGetDevicePointer|hipEventCreate\w*|hipEventDestroy|"
                       r"hipStreamCreate\w*|hipStreamDestroy)\s*\(")
    seen = 0
    for name in sorted(os.listdir(csrc)):
        if name == "khr_owned.h" or not name.endswith((".h", ".hip")):
            continue
        seen += 1
        for no, line in enumerate(open(os.path.join(csrc, name), errors="replace"), 1):
            code = re.sub(r'"(\\.|[^"\\])*"', '""', line).split("//")[0]
            assert not calls.search(code), "%s:%d calls the runtime directly: %s" % (name, no, line.strip())
    assert seen >= 10
    own = open(os.path.join(csrc, "khr_owned.h")).read()
    assert all(f in own for f in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipEventCreateWithFlags(", "hipEventDestroy",
                                  "hipStreamCreateWithFlags(", "hipStreamDestroy"))
