"""The slice height -> global voxel z rule (getVoxelKey((0, 0, h)).z, ASSUMPTIONS.md A.10) as a known-answer table, held in
its three forms: khronos_amd.capi.slice_voxel_z (Python), hydra::sliceVoxelZ (the header-only C++ helper the host code uses,
compiled here with g++) and khr_slice_voxel_z (C ABI).  Plus the visualizer's three slice classifications (hydra::everFreeSlice /
trackingSlice / tsdfSlice) against a numpy restatement of active_window_visualizer.cpp:382-397, 443-459, 500-512."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from khronos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (height, voxel_size, voxels_per_side, voxel z).  Heights and sizes are float32; the last four rows are heights where the
# block-then-voxel floor lands the local index on -1 / vps by rounding (the index then names the neighbouring layer's edge voxel).
TABLE = [
    (0.0, 0.1, 16, 0), (-0.0, 0.1, 16, 0), (0.05, 0.1, 16, 0), (0.15, 0.1, 16, 1), (-0.05, 0.1, 16, -1), (-0.5, 0.1, 16, -5),
    (0.3, 0.1, 16, 3),                                        # multiple of the voxel size
    (1.6, 0.1, 16, 16), (3.2, 0.1, 16, 32), (-1.6, 0.1, 16, -16), (-3.2, 0.1, 16, -32),  # multiples of the block size
    (0.32, 0.02, 16, 16), (-0.32, 0.02, 16, -16), (1.0, 0.02, 16, 50),
    (0.5, 0.05, 8, 9),                                        # 0.5f / 0.05f = 9.99999985
    (-0.4, 0.05, 8, -8), (2.5, 0.25, 8, 10), (-2.0, 0.25, 8, -8), (12.34, 0.05, 16, 246), (-7.77, 0.05, 16, -156),
    (-1.6, 0.02, 8, -81), (-0.48, 0.02, 8, -24), (-6.4, 0.02, 8, -321),  # local index -1 (the block below's top voxel)
    (-1e-45, 0.02, 8, 0),                                     # local index vps of block -1 (= voxel 0 of block 0)
]


def _local(h, vs, vps):
    f32 = np.float32
    bs = f32(vs) * f32(vps)
    bz = int(np.floor(f32(h) * (f32(1) / bs)))
    return bz, int(np.floor((f32(h) - f32(bz) * bs) * (f32(1) / f32(vs))))


def test_python_rule_table():
    for h, vs, vps, want in TABLE:
        assert capi.slice_voxel_z(h, vs, vps) == want, (h, vs, vps)
    # the edge rows really are edge rows
    assert _local(-1.6, 0.02, 8)[1] == -1 and _local(-1e-45, 0.02, 8)[1] == 8
    with pytest.raises(ValueError):
        capi.slice_voxel_z(float("nan"), 0.1, 16)


def _compile(tmp_path, name, src):
    cpp = tmp_path / (name + ".cpp")
    cpp.write_text(src)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "khronos_amd", "host"), "-o", str(exe), str(cpp)])
    return str(exe)


def test_cpp_helper_agrees(tmp_path):
    exe = _compile(tmp_path, "vz", r'''
#include <cstdio>
#include <cstdlib>
#include "hydra_compat.h"
int main(int argc, char** argv) {
  float h, vs; int vps;
  while (std::scanf("%a %a %d", &h, &vs, &vps) == 3) std::printf("%lld\n", static_cast<long long>(hydra::sliceVoxelZ(h, vs, vps)));
  return 0;
}
''')
    inp = "".join("%s %s %d\n" % (float(np.float32(h)).hex(), float(np.float32(vs)).hex(), vps) for h, vs, vps, _ in TABLE)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(v) for v in out] == [t[3] for t in TABLE]


def test_c_abi_agrees():
    lib = capi.load_library()
    z = C.c_int64(0)
    for h, vs, vps, want in TABLE:
        assert lib.khr_slice_voxel_z(C.c_float(h), C.c_float(vs), vps, C.byref(z)) == 0
        assert z.value == want, (h, vs, vps)
    assert lib.khr_slice_voxel_z(C.c_float(float("inf")), C.c_float(0.1), 16, C.byref(z)) == capi.KHR_EINVAL
    assert lib.khr_slice_voxel_z(C.c_float(1.0), C.c_float(0.0), 16, C.byref(z)) == capi.KHR_EINVAL


def _restate_classes(d, w, lo, fl, stamp_ns, trunc, show):
    """(voxel, class, value) lists of the three slices; classes as hydra::SliceClass (0 unknown, 1 free, 2 occupied, 3 too old,
    4 value)"""
    ef, tr, ts = [], [], []
    stamp_s = stamp_ns / 1e9
    for i in range(len(d)):
        unknown = int(lo[i]) == 0
        if not unknown or show:
            ef.append((i, 0 if unknown else (1 if fl[i] & 2 else 2), 0.0))
            if unknown:
                tr.append((i, 0, 0.0))
            else:
                age = np.float32(stamp_s - int(lo[i]) / 1e9)
                tr.append((i, 3, 0.0) if age > np.float32(3) else (i, 4, float(age)))
        if float(w[i]) < 1e-6:
            ts.append((i, 0, 0.0))
        else:
            ts.append((i, 4, float(np.float32(0.5 + 0.5 * float(d[i]) / float(np.float32(trunc))))))
    return ef, tr, ts


def test_slice_classifications(tmp_path):
    exe = _compile(tmp_path, "cls", r'''
#include <cstdio>
#include <cinttypes>
#include "hydra_compat.h"
int main() {
  size_t n; unsigned long long stamp; float trunc; int show;
  if (std::scanf("%zu %llu %a %d", &n, &stamp, &trunc, &show) != 4) return 2;
  hydra::MapSlice s;
  s.distance.resize(n); s.weight.resize(n); s.last_observed.resize(n); s.flags.resize(n);
  for (size_t i = 0; i < n; ++i) {
    unsigned long long lo; unsigned f;
    if (std::scanf("%a %a %llu %u", &s.distance[i], &s.weight[i], &lo, &f) != 4) return 2;
    s.last_observed[i] = lo; s.flags[i] = static_cast<uint8_t>(f);
  }
  const hydra::SlicePoints r[3] = {hydra::everFreeSlice(s, show != 0), hydra::trackingSlice(s, stamp, show != 0), hydra::tsdfSlice(s, trunc)};
  for (const auto& p : r) {
    std::printf("%zu\n", p.voxel.size());
    for (size_t k = 0; k < p.voxel.size(); ++k) std::printf("%u %d %a\n", p.voxel[k], int(p.cls[k]), p.value[k]);
  }
  return 0;
}
''')
    rng = np.random.default_rng(3)
    n = 600
    stamp = 10_000_000_000
    d = rng.uniform(-0.4, 0.4, n).astype(np.float32)
    w = np.where(rng.random(n) < 0.2, np.float32(0), rng.uniform(0, 5, n)).astype(np.float32)
    w[:5] = np.float32(1e-6)  # the threshold itself: float 1e-6 < double 1e-6 decides
    lo = np.where(rng.random(n) < 0.25, 0, stamp - rng.integers(0, 6_000_000_000, n)).astype(np.uint64)
    lo[5] = stamp - 3_000_000_000  # age exactly max_age: value, not too old
    fl = rng.integers(0, 16, n).astype(np.uint8)
    trunc = 0.3
    for show in (0, 1):
        inp = "%d %d %s %d\n" % (n, stamp, float(np.float32(trunc)).hex(), show) + "".join(
            "%s %s %d %d\n" % (float(d[i]).hex(), float(w[i]).hex(), int(lo[i]), int(fl[i])) for i in range(n))
        out = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
        got, pos = [], 0
        for _ in range(3):
            m = int(out[pos])
            got.append([(int(a), int(b), float.fromhex(c)) for a, b, c in (ln.split() for ln in out[pos + 1: pos + 1 + m])])
            pos += 1 + m
        want = _restate_classes(d, w, lo, fl, stamp, trunc, show)
        for g, e, name in zip(got, want, ("ever_free", "tracking", "tsdf")):
            assert g == e, name
