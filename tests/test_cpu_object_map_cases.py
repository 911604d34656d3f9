"""The cases of tests/object_map_cases.py on the CPU oracle alone: every case is shown to be what it claims to be -- the frames a case
declares untouched update no voxel, the straddling and partial ones fewer than an ordinary frame and more than none, every other
frame at least one; the mixed-allocation cases update more blocks than the grid of k_multi_order reaches with one thread per item;
the geometry each k_multi_cull case was built for is there (from the poses, in float64); the band case meets fuseBandRowsOk.
Nothing here runs the code under test."""
import os
import re

import numpy as np
import pytest

import object_map_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = oc.COARSE[0] * oc.VPS
_results = {}


def oracle(name):
    if name not in _results:
        _results[name] = oc.run_oracle(oc.CASES[name])
    return _results[name]


def last_batch(case):
    return [s for s in case["objects"][-1]["steps"] if s[0] == "batch"][-1][1]


def corners(case, k, indices=oc.WALL_BOX, bs=BS):
    """pixel coordinates and camera z of the eight corners of the block box in frame k"""
    T = np.linalg.inv(case["frames"][k]["pose"])
    pc = oc.box_corners(indices, bs) @ T[:3, :3].T + T[:3, 3]
    fx, fy, cx, cy = oc.intrinsics(case)
    with np.errstate(divide="ignore", invalid="ignore"):
        return fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy, pc[:, 2]


@pytest.mark.parametrize("name", list(oc.CASES))
def test_every_frame_is_what_the_case_says(name):
    case, r = oc.CASES[name], oracle(name)
    n = {k: st["n_updated_voxels"] for _, k, st in r["per_frame"]}
    print(name, "blocks", r["n_blocks"], "blocks a batch changed", r["updated"], "n_updated_voxels per frame", n)
    ordinary = n[case["ordinary_frame"]] if case["partial"] else None
    for k in last_batch(case):
        if k in case["untouched"]:
            assert n[k] == 0, (k, n[k])
        elif k in case["partial"]:
            assert 0 < n[k] < ordinary, (k, n[k], ordinary)
        else:
            assert n[k] > 0, k
    # a surface came out, no pool ran out
    assert len(r["mesh"]["points"]) > 0
    assert r["n_blocks"] <= case["mini"]["max_blocks"]
    assert 0 < r["updated"] <= r["n_blocks"]


@pytest.mark.parametrize("name", oc.C_AGAIN)
def test_label_map_variants_update_the_same_voxels(name):
    """the update count does not depend on the layout: the C cases that run again with LABEL_MAP keep their property"""
    a = oc.run_oracle(oc.variant(name, "label"))
    assert [st["n_updated_voxels"] for _, _, st in a["per_frame"]] == [st["n_updated_voxels"] for _, _, st in oracle(name)["per_frame"]]
    assert a["pruned"] is None


# ---------------------------------------------------------------------------------------------------------------------- group R
def test_reuse_cases_are_built_as_stated():
    for name in oc.R_CASES:
        case = oc.CASES[name]
        scales = [o["scale"] for o in case["objects"]]
        assert len(scales) >= 2 and all(x != y for x, y in zip(scales, scales[1:])), name
        assert len(case["frames"]) + 2 <= (42 if name in ("R2", "R3") else 16) and case["size"] == (160, 120)
    first, later = [[s for s in o["steps"] if s[0] in ("alloc", "batch")] for o in oc.CASES["R1"]["objects"]]
    assert 300 <= len(first[0][1]) <= 400 and oc.K_MULTI_CHUNK < len(first[1][1]) <= 2 * oc.K_MULTI_CHUNK
    assert len(later[0][1]) <= 40 and len(later[1][1]) == 3
    lo, hi = first[0][1].min(0), first[0][1].max(0)
    assert ((later[0][1] >= lo) & (later[0][1] <= hi)).all(), "the later box's indices are indices of the first box"
    r = oracle("R1")
    assert r["updated"] < r["n_blocks"], "the frames see only part of the box"
    words = lambda name, i: (len(oc.CASES[name]["objects"][i]["steps"][1][1]) + 31) // 32
    assert (words("R2", 0), words("R2", 1), words("R3", 0), words("R3", 1)) == (1, 2, 2, 1)
    assert [len(s[1]) for s in oc.CASES["R4"]["objects"][0]["steps"] if s[0] == "batch"] == [1, 0]
    assert oc.CASES["R5"]["layout"] == "label" and oc.LAYOUTS["label"]["with_tracking"] == 1 and oc.LAYOUTS["label"]["num_labels"] == 4
    assert oc.CASES["R6"]["objects"][0]["steps"][-1] == ("prune_mesh",)


# ---------------------------------------------------------------------------------------------------------------------- group M
@pytest.mark.parametrize("name", oc.M_CASES)
def test_mixed_allocation_updates_blocks_beyond_the_order_grid(name):
    """U blocks change their weight in frames 1..8; slots are dense from 0 on a context whose free list is the identity, so with
    U > 128 * ceil(8 E / 1024) at least one of them lies beyond what one thread per item of that grid reaches"""
    case, r = oc.CASES[name], oracle(name)
    E, reach = oc.explicit_count(case), oc.order_reach(case)
    print(name, "E", E, "reach", reach, "U", r["updated"], "blocks", r["n_blocks"])
    assert E == (200 if name == "M3" else 6)
    assert reach == 128 * -(-8 * E // 1024)
    assert r["updated"] > reach
    assert r["n_blocks"] <= case["mini"]["max_blocks"] <= 8192
    assert last_batch(case) == list(range(1, 9))
    if name != "M3":
        present = r["after_alloc_frame"]
        assert all(tuple(b) in present for b in oc.M_PRESENT) and not any(tuple(b) in present for b in oc.M_OUTSIDE)
        assert r["n_blocks"] == len(present) + len(oc.M_OUTSIDE)
    else:
        assert case["objects"][-1]["steps"][0][0] == "alloc" and r["n_blocks"] > E


# ---------------------------------------------------------------------------------------------------------------------- group C
def test_cull_case_geometry():
    C = oc.CASES
    u, v, z = corners(C["C1"], 1)
    assert (z < 0).all(), "C1: the box is behind the camera"
    for name, test in (("C2", lambda z, lo, hi: (z > hi).all()), ("C2b", lambda z, lo, hi: (z < lo).all())):
        lo, hi = C[name]["frames"][1]["ranges"]
        assert test(corners(C[name], 1)[2], lo, hi), name
        assert C[name]["frames"][0]["ranges"] == (0.1, 5.0)
    p = C["C3"]["frames"][1]["pose"][:3, 3]
    assert (p > oc.WALL_BOX.min(0) * BS).all() and (p < (oc.WALL_BOX.max(0) + 1) * BS).all(), "C3: the camera centre is inside the box"
    W, H = C["C4"]["size"]
    sides = {1: lambda u, v: (u < -2).all(), 2: lambda u, v: (u > W + 1).all(), 3: lambda u, v: (v > H + 1).all(), 4: lambda u, v: (v < -2).all()}
    seen = set()
    for k in (1, 2, 3, 4):
        u, v, z = corners(C["C4"], k)
        assert (z > 0.05).all()
        side = [s for s, out in sides.items() if out(u, v)]
        assert len(side) == 1, ("C4: wholly outside one border", k, side)
        seen.add(side[0])
        u, v, z = corners(C["C4b"], k)
        assert (z > 0.05).all()
        lo, hi, limit = ((u.min(), u.max(), W) if side[0] in (1, 2) else (v.min(), v.max(), H))
        edge = 0 if side[0] in (1, 4) else limit
        assert lo < edge < hi, ("C4b: straddles the same border", k)
    assert seen == {1, 2, 3, 4}, "C4: one frame per side"
    fx, fy, cx, cy = oc.intrinsics(C["C5"])
    assert fx != fy and cx != W / 2 and cy != H / 2
    for f in C["C5"]["frames"]:
        assert np.abs(f["pose"][:3, :3]).min() > 0.05, "C5: no entry of the rotation is near zero"
    u, v, z = corners(C["C5"], 2)
    assert u.min() < 0 < u.max() or u.min() < W < u.max()
    f = oc.render(C["C6"])
    assert f[1]["label"][H // 2, W // 2] == oc.MOVER and not (f[0]["label"] == oc.MOVER).any()
    u0, v0, u1, v1 = oc.footprint(C["C6"], C["C6"]["frames"][1]["pose"], oc.WALL_BOX, BS, margin=0)
    assert (f[1]["label"][v0:v1 + 1, u0:u1 + 1] == oc.MOVER).all(), "C6: the screen covers the whole footprint"
    assert (f[1]["depth"][v0:v1 + 1, u0:u1 + 1] < corners(C["C6"], 1)[2].min() - oc.COARSE[1]).all()
    f = oc.render(C["C6b"])
    assert not (f[1]["label"] == oc.MOVER).any() and (f[0]["label"] == oc.MOVER).any()
    u0, v0, u1, v1 = oc.footprint(C["C6b"], C["C6b"]["frames"][1]["pose"], oc.MOVER_BOX, BS, margin=0)
    assert (f[1]["depth"][v0:v1 + 1, u0:u1 + 1] > corners(C["C6b"], 1, oc.MOVER_BOX)[2].max() + oc.COARSE[1]).all(), "C6b: free space"
    for name, k in (("C7", 1), ("C7b", 2)):
        d = oc.render(C[name])[k]["depth"]
        u0, v0, u1, v1 = oc.footprint(C[name], C[name]["frames"][k]["pose"], oc.WALL_BOX, BS, margin=0)
        part = d[v0:v1 + 1, u0:(u1 if name == "C7" else (u0 + u1) // 2 - 4) + 1]
        assert not (part > 0).any() and np.isnan(part).any() and (part == 0).any(), name
        if name == "C7b":
            assert (d[v0:v1 + 1, (u0 + u1) // 2 + 8:u1 + 1] > 0).all()
    c8 = C["C8"]
    assert c8["size"] == (320, 240) and len(oc.SLAB) == 25 and len(np.unique(oc.SLAB[:, 2])) == 1
    above = (4, 0, 9)   # the block over the camera
    assert any((oc.SLAB == above).all(1))
    t = [oc.tiles_under(c8, c8["frames"][k]["pose"], above, BS, 0) for k in range(4)]
    print("C8: tiles under the lowest item of the block over the camera, per frame:", t)
    assert t[1] > 96 and max(t[0], t[2], t[3]) <= 96
    assert abs((oc.SLAB[0][2] * BS) - c8["frames"][1]["pose"][2, 3] - 0.3) < 0.06, "about 0.3 m under the slab"
    c9 = C["C9"]
    W, H = c9["size"]
    assert (W, H) == (161, 119) and W % 16 and H % 16
    u, v, z = corners(c9, 1)
    assert (z > 0.05).all() and u.min() < W - 1 < u.max() and v.min() < H - 1 < v.max()
    for name in oc.C_CASES:
        assert 3 <= len(C[name]["frames"]) <= 6 and 18 <= len(C[name]["objects"][0]["steps"][0][1]) <= 50
        assert not set(C[name]["untouched"] + C[name]["partial"]) & {0, len(C[name]["frames"]) - 1}, "ordinary frames around the special ones"


# ---------------------------------------------------------------------------------------------------------------------- group B
def test_band_case_takes_the_row_form():
    rows, records = oc.CASES["B_rows"], oc.CASES["B_records"]
    cr, cc = (oc.mini_config(c, c["objects"][0]["scale"]) for c in (rows, records))
    assert cr.max_frame_pixels == 641 * 480 and cc.max_frame_pixels == 320 * 240 and rows["size"] == records["size"] == (320, 240)
    for cfg in (cr, cc):
        assert cfg.with_semantics == 1 and cfg.semantic_mode == 0 and cfg.num_labels == 20 and cfg.packed_likelihood_rows == 0
        assert oc.padded_row(cfg) % 32 == 0 and oc.padded_row(cfg) >= cfg.num_labels
        assert oc.band_rows_ok(cfg)
    assert all(f["rgb"] is not None and f["label"] is not None for f in oc.render(rows))
    assert (oc.band_mode(cr), oc.band_mode(cc)) == (1, 0)
    assert not oc.band_rows_ok(oc.mini_config(oc.CASES["R5"], oc.COARSE)), "four labels: rows are not padded"
    n = len(last_batch(rows))
    assert n == 15 == len(last_batch(records)) and -(-n // oc.K_MULTI_CHUNK) == 3
    assert rows["frames"] == records["frames"] and rows["objects"] == records["objects"]
    # the restatements above are those of the sources
    dev = open(os.path.join(ROOT, "khronos_amd", "csrc", "khr_device.h")).read()
    assert re.search(r"likStride\(int K\) \{ return K <= 4 \? K : \(\(K \+ 31\) & ~31\); \}", dev)
    fuse = open(os.path.join(ROOT, "khronos_amd", "csrc", "khr_kernels_fuse.h")).read()
    assert "return do_sem && has_color && sem_mode != 1 && (KS & 31) == 0 && KS <= 256;" in fuse
    hip = open(os.path.join(ROOT, "khronos_amd", "csrc", "khronos_amd.hip")).read()
    assert "a->band_mode = c->cfg.max_frame_pixels <= 640u * 480u ? 0 : 1;" in hip
    assert "constexpr int kMultiChunk = %d;" % oc.K_MULTI_CHUNK in hip
