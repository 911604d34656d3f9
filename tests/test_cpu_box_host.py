"""-m "not gpu": the host side the box-field calls share (khronos_amd/csrc/khr_box_host.h: the 256-byte arena and the layouts
carved with it, the check of a cell box, the launch geometry of a separable pass, the box a result describes), through a
stand-alone program (tests/box_host_selftest.cpp) built with the address and undefined-behaviour sanitizers.  The program prints;
every expectation is written out here."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 24

# The frozen record of the layouts: (field, bytes per element, elements) in the order the fields lie in memory, as khronos_amd.hip
# carved them (`carve(...)` lines of vorDense, vorList, plDense, plWork, plOut, tfDense, tfStarts; the hand-summed offsets of
# khr_places_graph_from and khr_travel_field_from) before the layouts moved into the header.  `floor`: the least size of the block.
LAYOUTS = {
    "vorDense": dict(fields=lambda n, _: [("distance", 4, n), ("d2", 4, n), ("site", 4, n), ("status", 1, n), ("basis", 1, n), ("wg_count", 4, (n + 255) // 256 + 1)]),
    "vorList": dict(fields=lambda m, _: [("cells", 12, m), ("distance", 4, m), ("basis", 1, m), ("sites", 12 * 4, m)], floor=256),
    "plIn": dict(fields=lambda n, _: [("distance", 4, n), ("d2", 4, n), ("basis", 1, n), ("site", 4, n)]),
    "plDense": dict(fields=lambda n, _: [("rec_key", 8, n), ("rec_acc", 8, n), ("label", 4, n), ("number", 4, n + 1), ("pair_count", 4, n + 1), ("place", 4, n)]),
    "plWork": dict(fields=lambda m, p: [("keys", 8, m), ("keys_sorted", 8, m), ("vals", 4, m), ("vals_sorted", 4, m), ("head", 4, m + 1), ("n_unique", 4, 1),
                                        ("edge_a", 4, m), ("edge_b", 4, m), ("edge_clear", 4, m), ("edge_contacts", 4, m), ("edge_new", 4, m + 1),
                                        ("parent", 4, p), ("root", 4, p), ("size", 4, p), ("place_new", 4, p + 1), ("comp_new", 4, p + 1)]),
    "plOut": dict(fields=lambda p, e: [("sum", 24, p), ("centre", 12, p), ("centre_d2", 4, p), ("radius", 4, p), ("basis", 1, p), ("site", 12, p), ("n_cells", 4, p),
                                       ("degree", 4, p), ("component", 4, p), ("edge_a", 4, e), ("edge_b", 4, e), ("edge_clear", 4, e), ("edge_contacts", 4, e)],
                  floor=256),
    "tfIn": dict(fields=lambda n, g: [("distance", 4, n), ("status", 1, n), ("goals", 12, g)]),
    "tfDense": dict(fields=lambda n, t: [("keys", 8, n), ("cost", 4, n), ("goal", 4, n), ("parent", 1, n), ("mask", 1, n), ("flags", 2, t), ("go_on", 4, 8)]),
    "tfStarts": dict(fields=lambda s, _: [("offsets", 8, s + 1), ("starts", 12, s), ("path_cost", 4, s), ("path_goal", 4, s)]),
}
ONE = [(n, 0) for n in (0, 1, 255, 256, 257, BIG)]
TWO = [(0, 0), (0, 1), (1, 0), (1, 1), (255, 257), (256, 256), (257, 255), (256, 0), (0, 256), (BIG, 1), (1, BIG), (BIG, BIG)]
ARGS = {"vorDense": ONE, "vorList": ONE, "plIn": ONE, "plDense": ONE, "tfStarts": ONE, "plWork": TWO, "plOut": TWO, "tfIn": TWO,
        # cells and the tiles they lie in (8^3 cells a tile; at least one)
        "tfDense": [(0, 0), (1, 1), (255, 1), (256, 1), (257, 2), (512, 1), (513, 2), (BIG, BIG // 512), (BIG, 64 * 64 * 8), (257, 257), (256, 255), (1, 255), (255, 256)]}

DF_TILE, VOR_TILE, STRIP = 8192, 8192, 16   # kDfTileCells, kVorTileCells, kDfStrip of the kernel headers
EDGE, MAX_DIM = 1 << 30, 512
OK, BAD_DIM, BAD_RANGE, BAD_CELLS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = tmp_path_factory.mktemp("box_host") / "box_host_selftest"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                        os.path.join(ROOT, "tests", "box_host_selftest.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def _ask(exe, requests):
    out = subprocess.run([exe], input="\n".join(" ".join(str(v) for v in rq) for rq in requests) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stdout[-500:] + out.stderr[-3000:]   # (a sanitizer report is a failure)
    lines = out.stdout.splitlines()
    assert len(lines) == len(requests)
    return [ln.split() for ln in lines]


def _al(b):
    return (b + 255) // 256 * 256


def test_the_tile_sizes_are_the_kernel_headers():
    csrc = os.path.join(ROOT, "khronos_amd", "csrc")
    assert "constexpr int kDfTileCells = %d;" % DF_TILE in open(os.path.join(csrc, "khr_kernels_distance.h")).read()
    assert "constexpr int kDfStrip = %d;" % STRIP in open(os.path.join(csrc, "khr_kernels_distance.h")).read()
    assert "constexpr int kVorTileCells = %d;" % VOR_TILE in open(os.path.join(csrc, "khr_kernels_voronoi.h")).read()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_offsets_are_the_parent_commits(selftest, name):
    spec, args = LAYOUTS[name], ARGS[name]
    assert len(args) >= (12 if args is not ONE else 6)
    for (a, b), words in zip(args, _ask(selftest, [("layout", name, a, b) for a, b in args])):
        assert words[:4] == [name, str(a), str(b), ":"] and words[-2] == "bytes", words
        got_names, got = words[4:-2:2], [int(w) for w in words[5:-2:2]]
        total = int(words[-1])
        fields = spec["fields"](a, b)
        # the fields in the documented order, at the running sum of the 256-rounded sizes
        assert got_names == [f[0] for f in fields], (name, a, b)
        want, at = [], 0
        for _, per, count in fields:
            want.append(at)
            at += _al(per * count)
        assert got == want, (name, a, b, got_names)
        # ... which makes every offset a multiple of 256, leaves each field its true size, and ends the block behind the last
        assert all(o % 256 == 0 for o in got)
        ends = got[1:] + [total]
        assert all(o + per * count <= nxt for o, (_, per, count), nxt in zip(got, fields, ends)), (name, a, b)
        assert total == max(at, spec.get("floor", 0)), (name, a, b)
        if (a, b) == (0, 0) and "floor" in spec:
            assert at == 0 and total == 256   # (never empty)


def _box_rule(origin, dims, ratio):
    """the rules in the order khr_distance_field has always applied them: per axis the dim, then the range; then the cell count"""
    cells = 1
    for a in range(3):
        if not 1 <= dims[a] <= MAX_DIM:
            return BAD_DIM, a, 0
        lo, hi = origin[a] * ratio, (origin[a] + dims[a]) * ratio - 1
        if lo <= -EDGE or hi >= EDGE:
            return BAD_RANGE, a, 0
        cells *= dims[a]
    return (BAD_CELLS if cells > BIG else OK), -1, cells


def _box_cases():
    cases = []   # (origin, dims, ratio, rule the case is there for)
    for ratio in (1, 2, 4):
        for axis in range(3):
            def on_axis(v, rest):
                return tuple(v if a == axis else rest for a in range(3))
            for d, rule in ((0, BAD_DIM), (-1, BAD_DIM), (1, OK), (512, OK), (513, BAD_DIM)):
                cases.append(((0, 0, 0), on_axis(d, 4), ratio, rule))
            # hi = (origin + dim) * ratio - 1 on the edge: with dim 3, the last origin whose hi stays below 2^30, and the next
            o_hi = EDGE // ratio - 3
            cases.append((on_axis(o_hi, 0), on_axis(3, 2), ratio, OK))
            cases.append((on_axis(o_hi + 1, 0), on_axis(3, 2), ratio, BAD_RANGE))
            # lo = origin * ratio on the edge
            o_lo = -(EDGE // ratio) + 1
            cases.append((on_axis(o_lo, 0), on_axis(3, 2), ratio, OK))
            cases.append((on_axis(o_lo - 1, 0), on_axis(3, 2), ratio, BAD_RANGE))
        cases.append(((-256, -256, -32), (512, 512, 64), ratio, OK))           # 2^24 cells
        cases.append(((-256, -256, -32), (512, 512, 65), ratio, BAD_CELLS))
        cases.append(((0, 0, 0), (512, 65, 512), ratio, BAD_CELLS))
    for o in (2**31 - 1, -2**31):   # no overflow at the ends of int32
        for axis in range(3):
            cases.append((tuple(o if a == axis else 0 for a in range(3)), (512, 512, 64), 4, BAD_RANGE))
    cases.append(((2**31 - 1,) * 3, (512,) * 3, 4, BAD_RANGE))
    cases.append(((0, 0, 0), (0, 513, 512), 1, BAD_DIM))           # the first bad axis is reported
    cases.append(((EDGE, 0, 0), (4, 0, 4), 1, BAD_RANGE))          # ... whichever rule it breaks
    return cases


def test_cell_box_check(selftest):
    cases = _box_cases()
    got = _ask(selftest, [("box",) + o + d + (r,) for o, d, r, _ in cases])
    for (origin, dims, ratio, rule), words in zip(cases, got):
        want = _box_rule(origin, dims, ratio)
        assert want[0] == rule, (origin, dims, ratio)   # (the case is what it was written for)
        assert [int(w) for w in words[1:]] == list(want), (origin, dims, ratio, words)
    # the edges sit where the issue puts them: hi == 2^30 - 1 passes, lo == -2^30 + 1 passes
    for ratio in (1, 2, 4):
        assert (EDGE // ratio - 3 + 3) * ratio - 1 == EDGE - 1 and (-(EDGE // ratio) + 1) * ratio == -EDGE + ratio
    ok_lo = [c for c in cases if c[2] == 1 and c[3] == OK and min(c[0]) == -EDGE + 1]
    assert len(ok_lo) == 3


def _grid(axis, nx, ny, nz, tile, strip):
    """the launch geometry as khr_distance_field and khr_voronoi_field wrote it out at their six launches"""
    if axis == 0:
        per_wg = max(1, tile // nx)
        return (ny * nz + per_wg - 1) // per_wg, 1, per_wg
    if axis == 1:
        per_wg = max(1, tile // (ny * strip))
        return (nx + strip - 1) // strip, (nz + per_wg - 1) // per_wg, per_wg
    per_wg = max(1, tile // (nz * strip))
    return (nx + strip - 1) // strip, (ny + per_wg - 1) // per_wg, per_wg


def test_pass_geometry(selftest):
    sizes = (1, 2, 7, 8, 9, 512)
    cases = [(axis, nx, ny, nz, tile, STRIP) for tile in dict.fromkeys((DF_TILE, VOR_TILE)) for axis in range(3) for nx, ny, nz in itertools.product(sizes, repeat=3)]
    for case, words in zip(cases, _ask(selftest, [("grid",) + c for c in cases])):
        axis, nx, ny, nz, tile, strip = case
        gx, gy, per_wg = (int(w) for w in words[1:])
        assert (gx, gy, per_wg) == _grid(*case), case
        assert per_wg >= 1 and gx >= 1 and gy >= 1
        if axis == 0:   # whole lines: every one of the ny * nz lines, and no more cells than the tile holds
            assert gy == 1 and gx * per_wg >= ny * nz and (gx - 1) * per_wg < ny * nz
            assert per_wg * nx <= tile
        else:           # strips of x by groups of the other axis
            length, other = (ny, nz) if axis == 1 else (nz, ny)
            assert gx * strip >= nx and (gx - 1) * strip < nx
            assert gy * per_wg >= other and (gy - 1) * per_wg < other
            assert per_wg * length * strip <= tile


def test_box_result(selftest):
    (words,) = _ask(selftest, [("result", -7, 8, 9, 20, 12, 16)])
    assert [int(w) for w in words[1:]] == [1, 20 * 12 * 16, -7, 8, 9, 20, 12, 16]
