"""-m "not gpu": properties of the numpy restatement of khr_merge_map (tests/merge_replica.py, ASSUMPTIONS.md A.17) that hold
whatever the maps are; tests/test_gpu_merge_map.py then holds the kernels to the replica byte for byte."""
import numpy as np

import merge_cases as mc
import merge_replica as mr
from khronos_amd import checkpoint as ck

f32 = np.float32
F16 = ck.config_fields(mc.CFG16)
KW = dict(min_weight=float(mc.MIN_WEIGHT), max_weight=float(mc.MAX_WEIGHT))


def by_index(idx, layers):
    return {tuple(int(v) for v in b): i for i, b in enumerate(idx)}


def test_into_an_empty_map_returns_the_observed_source():
    si, sl = mc.rich_map(mc.CFG16, [((0, 0, 0), "rich"), ((-1, 2, 0), "rich"), ((4, 4, 4), "zero")], 1)
    oi, ol, st = mr.merge(F16, np.zeros((0, 3), np.int32), mc.empty_layers(mc.CFG16), si, sl, **KW)
    assert [tuple(b) for b in oi] == [(-1, 2, 0), (0, 0, 0)]  # (the all-zero block allocates nothing)
    assert st["n_src_blocks"] == 3 and st["n_new_blocks"] == st["n_touched_blocks"] == 2 and st["n_merged_voxels"] == 0
    rows = by_index(si, sl)
    seen = 0
    for i, b in enumerate(oi):
        r = rows[tuple(b)]
        ok = sl["weight"][r] >= mc.MIN_WEIGHT
        seen += int(ok.sum())
        for k in ol:
            if k == "block_flags":
                continue
            assert np.array_equal(ol[k][i][ok], sl[k][r][ok]), k
            assert not ol[k][i][~ok].any(), k  # (a fresh block's voxels)
        assert ol["block_flags"][i] == 7 | (8 if (sl["flags"][r][ok] & 1).any() else 0)
    assert st["n_added_voxels"] == seen


def test_disjoint_maps_give_the_union():
    di, dl = mc.rich_map(mc.CFG16, [((0, 0, 0), "rich"), ((1, 0, 0), "rich")], 2)
    si, sl = mc.rich_map(mc.CFG16, [((5, 5, 5), "solid"), ((-3, 0, 0), "solid")], 3)
    oi, ol, st = mr.merge(F16, di, dl, si, sl, **KW)
    assert len(oi) == 4 and st["n_new_blocks"] == 2 and st["n_merged_voxels"] == 0
    rows, drows, srows = by_index(oi, ol), by_index(di, dl), by_index(si, sl)
    for b, r in drows.items():  # untouched: every value and flag bit for bit
        for k in ol:
            assert np.array_equal(ol[k][rows[b]], dl[k][r]), k
    for b, r in srows.items():
        for k in ("distance", "weight", "color", "flags", "last_observed", "last_occupied", "sem_label", "likelihoods"):
            assert np.array_equal(ol[k][rows[b]], sl[k][r]), k


def test_distance_and_weight_commute():
    ai, al = mc.rich_map(mc.CFG16, [((0, 0, 0), "rich"), ((0, 1, 0), "rich")], 4)
    bi, bl = mc.rich_map(mc.CFG16, [((0, 0, 0), "rich"), ((0, 1, 0), "rich")], 5)
    oi1, o1, s1 = mr.merge(F16, ai, al, bi, bl, min_weight=1e-6, max_weight=float(mc.MAX_WEIGHT))
    oi2, o2, s2 = mr.merge(F16, bi, bl, ai, al, min_weight=1e-6, max_weight=float(mc.MAX_WEIGHT))
    both = (al["weight"] > 0) & (bl["weight"] > 0)
    assert both.sum() > 1000 and s1["n_merged_voxels"] == s2["n_merged_voxels"] == int(both.sum())
    assert np.array_equal(o1["distance"][both].view(np.uint32), o2["distance"][both].view(np.uint32))
    assert np.array_equal(o1["weight"][both].view(np.uint32), o2["weight"][both].view(np.uint32))
    assert (o1["weight"] <= mc.MAX_WEIGHT).all() and (o1["weight"][both] == mc.MAX_WEIGHT).any()


def test_linear_field_survives_a_rigid_resample():
    """d(p) = n . p - c sampled trilinearly is exact up to rounding: at every valid destination voxel the merged-in distance is
    n' . c_v - c' within 1e-5 m (about 10 rounded operations at coordinates <= 4 m and values <= 0.3 m: ~1e-6 m, times ten)"""
    n, c0 = np.array([0.05, -0.03, 0.04]), 0.02
    blocks = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    si, sl = mc.ragged_map(mc.CFG16, blocks, 6)
    sl["weight"][:] = 2  # fully observed: the interior is valid everywhere
    T = mc.pose((1.0, 2.0, -0.5), 30.0, (0.137, -0.291, 0.053))
    oi, ol, st = mr.merge(F16, np.zeros((0, 3), np.int32), mc.empty_layers(mc.CFG16), si, sl, mode=mr.RESAMPLE, pose=T, **KW)
    assert st["n_added_voxels"] > 5000 and st["n_merged_voxels"] == 0
    vps, vs = 16, 0.1
    lin = np.arange(vps ** 3)
    Rm, t = T[:3, :3], T[:3, 3]
    n2 = Rm @ n                      # d(src_T_dst c) = n . R^T (c - t) - c0
    c2 = c0 + n2 @ t
    worst = 0.0
    for i, b in enumerate(oi):
        cv = np.stack([(int(b[a]) * vps + (lin // vps ** a) % vps + 0.5) * vs for a in range(3)], axis=1)
        ok = ol["weight"][i] > 0
        worst = max(worst, float(np.abs(ol["distance"][i][ok].astype(np.float64) - (cv[ok] @ n2 - c2)).max()))
    assert worst <= 1e-5, worst


def test_cases_meet_every_rule():
    """the hand-built cases reach what they were built for (tests/merge_cases.py)"""
    c = mc.BY_NAME["odd_offset"]
    oi, ol, st = mc.replica_of(c)
    assert st["n_new_blocks"] > 0 and st["n_added_voxels"] > 0 and st["n_merged_voxels"] > 0
    assert st["n_touched_blocks"] < st["n_candidate_blocks"]  # (the zero-weight source block touches nothing)
    rows, drows = by_index(oi, ol), by_index(*c["dst"])
    r = drows[(6, 6, 6)]
    for k in ol:  # a block no sample reaches
        assert np.array_equal(ol[k][rows[(6, 6, 6)]], c["dst"][1][k][r]), k
    # block (0, 0, 0) of zero_offset is rich on both sides: every case of every per-voxel rule occurs among its voxel pairs
    z = mc.BY_NAME["zero_offset"]
    d = {k: v[by_index(*z["dst"])[(0, 0, 0)]] for k, v in z["dst"][1].items()}
    s = {k: v[by_index(*z["src"])[(0, 0, 0)]] for k, v in z["src"][1].items()}
    mw, below = mc.MIN_WEIGHT, np.nextafter(mc.MIN_WEIGHT, f32(0))
    seen, both = s["weight"] >= mw, (s["weight"] >= mw) & (d["weight"] > 0)
    assert (s["weight"] == mw).any() and (s["weight"] == below).any() and (seen & (d["weight"] == 0)).any()
    assert (both & (d["weight"] + s["weight"] == mc.MAX_WEIGHT)).any() and (both & (d["weight"] + s["weight"] > mc.MAX_WEIGHT)).any()
    for a_d in (0, 255):
        for a_s in (0, 255):
            assert (both & (d["color"][:, 3] == a_d) & (s["color"][:, 3] == a_s)).any(), (a_d, a_s)
    for bits in range(16):  # SEM_VALID and the three tracking bits, every pair of words
        assert all((both & (d["flags"] == bits) & (s["flags"] == other)).any() for other in range(16)), bits
    for name in ("last_observed", "last_occupied"):
        assert (both & (d[name] < s[name])).any() and (both & (d[name] > s[name])).any(), name
    sv = both & ((d["flags"] & 8) != 0) & ((s["flags"] & 8) != 0)
    rows = (d["likelihoods"] + s["likelihoods"])[sv]
    top = np.sort(rows, axis=1)
    assert (top[:, -1] == top[:, -2]).any()  # a tied row sum: the first argmax decides
    q = mc.replica_of(mc.BY_NAME["resample"])[2]
    assert q["n_added_voxels"] > 0 and q["n_merged_voxels"] > 0 and q["n_new_blocks"] > 0
