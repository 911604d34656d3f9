"""-m "not gpu": properties of the numpy restatement of khr_diff_map (tests/diff_replica.py, ASSUMPTIONS.md A.18) that hold whatever
the maps are, and that the hand-built cases (tests/diff_cases.py) reach what they were built for; tests/test_gpu_diff_map.py then
holds the kernels to the replica byte for byte."""
import functools

import numpy as np
import pytest

import diff_cases as dc
import diff_replica as dr
import merge_cases as mc
from khronos_amd import checkpoint as ck

f32 = np.float32
F16 = ck.config_fields(mc.CFG16)
ARRAYS = [n for n, _, _ in dr.VOXEL_FIELDS + dr.BLOCK_FIELDS]


@functools.lru_cache(maxsize=None)
def expected(name):
    return dc.replica_of(dc.BY_NAME[name])


def loop_diff(case):
    """A.18 under ALIGNED as a plain loop over blocks and voxels on Python scalars"""
    cfg = ck.config_fields(case["cfg"])
    vps = cfg["voxels_per_side"]
    (ni, nl), (ti, tl) = case["now"], case["then"]
    mw, occ = f32(case["min_weight"]), f32(case["occupied_distance"] or 0.0)
    free = f32(cfg["voxel_size"]) if case["free_distance"] is None else f32(case["free_distance"])
    off = case["voxel_offset"]
    then_rows = {tuple(int(v) for v in b): i for i, b in enumerate(ti)}
    cand = set()
    for b in then_rows:
        for c in range(8):
            cand.add(tuple((b[a] * vps + off[a] + (vps - 1 if (c >> a) & 1 else 0)) // vps for a in range(3)))
    stats = dict.fromkeys(dr.STATS, 0)
    stats["n_ref_blocks"], stats["n_candidate_blocks"] = len(ti), len(cand)
    rows = []
    order = sorted(range(len(ni)), key=lambda i: tuple(int(v) for v in ni[i]))
    for i in order:
        b = tuple(int(v) for v in ni[i])
        if b not in cand:
            continue
        stats["n_present_blocks"] += 1
        n_before = len(rows)
        for lin in range(vps ** 3):
            g = [b[0] * vps + lin % vps, b[1] * vps + (lin // vps) % vps, b[2] * vps + lin // (vps * vps)]
            s = [g[a] - off[a] for a in range(3)]
            r = then_rows.get(tuple(v // vps for v in s))
            sl = (s[0] % vps) + vps * ((s[1] % vps) + vps * (s[2] % vps))
            T = r is not None and tl["weight"][r, sl] >= mw
            N = nl["weight"][i, lin] >= mw
            stats["n_compared_voxels"] += int(N and T)
            stats["n_only_now"] += int(N and not T)
            stats["n_only_then"] += int(T and not N)
            if not (N and T):
                continue
            d_now, d_then = nl["distance"][i, lin], tl["distance"][r, sl]
            kind = 1 if (d_then >= free and d_now <= occ) else (2 if (d_then <= occ and d_now >= free) else 0)
            if kind:
                stats["n_appeared" if kind == 1 else "n_disappeared"] += 1
                rows.append((g, kind, d_now, d_then, nl["sem_label"][i, lin] if kind == 1 else tl["sem_label"][r, sl],
                             nl["last_observed"][i, lin], tl["last_observed"][r, sl]))
        stats["n_changed_blocks"] += int(len(rows) > n_before)
    return stats, rows


@pytest.mark.parametrize("name", ["zero_offset", "odd_offset", "vps8_odd_offset", "three_blocks_default_thresholds"])
def test_vectorised_replica_matches_a_per_voxel_loop(name):
    c, got = dc.BY_NAME[name], expected(name)
    stats, rows = loop_diff(c)
    assert got["stats"] == stats and len(rows) > 50
    assert got["voxels"].tolist() == [r[0] for r in rows]
    assert got["kind"].tolist() == [r[1] for r in rows]
    for k, col in (("d_now", 2), ("d_then", 3)):
        assert got[k].tobytes() == np.array([r[col] for r in rows], f32).tobytes(), k
    assert got["label"].tolist() == [int(r[4]) for r in rows]
    assert got["stamp_now"].tolist() == [int(r[5]) for r in rows] and got["stamp_then"].tolist() == [int(r[6]) for r in rows]
    assert int(got["block_appeared"].sum()) == stats["n_appeared"] and int(got["block_disappeared"].sum()) == stats["n_disappeared"]


def test_a_map_against_itself_has_no_changes():
    r = expected("no_change")
    idx, L = dc.BY_NAME["no_change"]["now"]
    st = r["stats"]
    assert st["n_present_blocks"] == len(idx) == 3 and st["n_changed_blocks"] == st["n_appeared"] == st["n_disappeared"] == 0
    assert st["n_only_now"] == st["n_only_then"] == 0 and st["n_compared_voxels"] == int((L["weight"] >= dc.MIN_WEIGHT).sum()) > 0
    assert all(len(r[k]) == 0 for k in ARRAYS)


def test_swapping_the_maps_swaps_appeared_and_disappeared():
    c = dc.BY_NAME["order"]  # ALIGNED, zero offset, equal block sets
    kw = dc.request_of(c)
    ab = dr.diff(F16, *c["now"], *c["then"], **kw)
    ba = dr.diff(F16, *c["then"], *c["now"], **kw)
    a, b = ab["kind"] == dr.APPEARED, ba["kind"] == dr.DISAPPEARED
    assert a.sum() > 100 and (~a).sum() > 100
    assert ab["voxels"][a].tolist() == ba["voxels"][b].tolist()
    assert ab["d_now"][a].tobytes() == ba["d_then"][b].tobytes() and ab["d_then"][a].tobytes() == ba["d_now"][b].tobytes()
    assert ab["label"][a].tolist() == ba["label"][b].tolist()  # (the occupied side is the same map both times)
    assert ab["stamp_now"][a].tolist() == ba["stamp_then"][b].tolist()
    assert ab["stats"]["n_appeared"] == ba["stats"]["n_disappeared"] and ab["stats"]["n_disappeared"] == ba["stats"]["n_appeared"]


def test_a_carved_ball_gives_exactly_its_voxels():
    """a solid ball in `then` (distance -0.1) that `now` has carved free (+0.1), everything else equal and free"""
    blocks = [(x, y, 0) for x in (0, 1) for y in (0, 1)]
    now, then = dc.solid_map(mc.CFG16, blocks, 61, 0.1), dc.solid_map(mc.CFG16, blocks, 62, 0.1)
    lin = np.arange(16 ** 3)
    want = []
    for i, b in enumerate(then[0]):
        g = np.stack([int(b[a]) * 16 + (lin // 16 ** a) % 16 for a in range(3)], axis=1)
        ball = ((g - np.array([16, 16, 8])) ** 2).sum(axis=1) <= 36
        then[1]["distance"][i][ball] = f32(-0.1)
        want += [(tuple(v), int(then[1]["sem_label"][i][l]), int(now[1]["last_observed"][i][l]), int(then[1]["last_observed"][i][l]))
                 for v, l in zip(g[ball].tolist(), lin[ball])]
    r = dr.diff(F16, *now, *then, min_weight=0.5, occupied_distance=0.0, free_distance=0.05)
    assert r["stats"]["n_disappeared"] == len(want) > 800 and r["stats"]["n_appeared"] == 0 and r["stats"]["n_changed_blocks"] == 4
    assert (r["kind"] == dr.DISAPPEARED).all()
    got = sorted(zip(map(tuple, r["voxels"].tolist()), r["label"].tolist(), r["stamp_now"].tolist(), r["stamp_then"].tolist()))
    assert got == sorted(want)


@pytest.mark.parametrize("name", ["order", "odd_offset", "resample"])
def test_list_order_is_a_lexsort(name):
    r = expected(name)
    vps = dc.BY_NAME[name]["cfg"]["voxels_per_side"]
    b = r["blocks"]
    assert len(b) >= 2 and np.array_equal(np.lexsort((b[:, 2], b[:, 1], b[:, 0])), np.arange(len(b)))
    v = r["voxels"]
    blk, loc = v // vps, v % vps
    lin = loc[:, 0] + vps * (loc[:, 1] + vps * loc[:, 2])
    assert np.array_equal(np.lexsort((lin, blk[:, 2], blk[:, 1], blk[:, 0])), np.arange(len(v)))
    n = r["block_appeared"] + r["block_disappeared"]
    assert np.array_equal(r["block_first"], np.concatenate([[0], np.cumsum(n)[:-1]])) and int(n.sum()) == len(v)
    assert np.array_equal(blk[r["block_first"]], b)


def test_cases_reach_what_they_were_built_for():
    o = expected("order")
    assert list(map(tuple, o["blocks"].tolist())) == sorted(dc.ORDER_BLOCKS)
    packed = sorted(dc.ORDER_BLOCKS, key=lambda b: (b[2], b[1], b[0]))  # packKey: x in the low bits
    assert sorted(dc.ORDER_BLOCKS) != packed and sorted(dc.ORDER_BLOCKS) != dc.ORDER_BLOCKS
    assert [expected(n)["stats"]["n_changed_blocks"] for n in ("no_change", "one_block", "three_blocks_default_thresholds")] == [0, 1, 3]
    for name, nv in (("all_changed", 4096), ("all_changed_vps8", 512)):
        r = expected(name)
        assert r["stats"]["n_appeared"] + r["stats"]["n_disappeared"] == nv == len(r["kind"]) and r["stats"]["n_changed_blocks"] == 1
    s = expected("singles")
    assert s["voxels"].tolist() == [[0, 0, 0], [47, -1, 15]] and s["kind"].tolist() == [1, 2] and s["block_first"].tolist() == [0, 1]
    for name, vps in (("four_waves_vps16", 16), ("four_waves_vps8", 8)):
        r = expected(name)
        loc = r["voxels"] - vps
        groups = (loc[:, 0] + vps * (loc[:, 1] + vps * loc[:, 2])) // 64
        assert set((groups % 4).tolist()) == {0, 1, 2, 3} and {1, 2} == set(r["kind"].tolist())
    z = expected("zero_offset")["stats"]
    assert z["n_ref_blocks"] == 5 and z["n_candidate_blocks"] == 5 and z["n_present_blocks"] == 4  # (0, 0, 1) is absent, (3, 3, 3) unreached
    assert z["n_only_now"] > 4096 * 0.4 and z["n_only_then"] > 4096 * 0.4 and z["n_changed_blocks"] == 2
    # the distance list puts voxels on each threshold and next to it, on either side of the comparison
    c = dc.BY_NAME["zero_offset"]
    d = np.concatenate([c["now"][1]["distance"].ravel(), c["then"][1]["distance"].ravel()])
    for t in (dc.OCC, dc.FREE):
        assert all((d == v).any() for v in (t, np.nextafter(t, -dc.INF), np.nextafter(t, dc.INF)))
    q = expected("resample")["stats"]
    assert q["n_appeared"] > 50 and q["n_disappeared"] > 50 and q["n_only_now"] > 0 and q["n_present_blocks"] == 3 and q["n_changed_blocks"] >= 2
    for name in ("block_offset", "odd_offset", "vps8_zero_offset", "vps8_block_offset", "vps8_odd_offset"):
        st = expected(name)["stats"]
        assert st["n_appeared"] > 20 and st["n_disappeared"] > 20 and st["n_present_blocks"] < st["n_candidate_blocks"], (name, st)
