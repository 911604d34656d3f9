"""-m "not gpu": properties of tests/segment_replica.py (the numpy / plain-Python restatement of khr_segment_map, ASSUMPTIONS.md
A.19) on the hand-built maps of tests/segment_cases.py -- the hand-written component counts, partition, refinement across the
connectivities and across by_label, shift and permutation invariance, consistency of the per-component values with the voxel list,
and a second, independent closure (repeated min-propagation over a dense array) on two dense cases."""
import numpy as np
import pytest

import segment_cases as sc
import segment_replica as sr
from khronos_amd import checkpoint as ck

NAMES = [c["name"] for c in sc.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_hand_written_counts_and_consistency(name):
    c = sc.BY_NAME[name]
    for i, run in enumerate(c["runs"]):
        r = sc.replica_of(c, i)
        st = r["stats"]
        print(name, sc.request_of(run), st)
        if run["expect"] is not None:
            assert st["n_components"] == run["expect"], (name, run, st)
        assert st["n_components_all"] == st["n_too_small"] + st["n_too_large"] + st["n_components"]
        assert st["n_blocks"] == len(c["now"][0])
        # the kept components partition the kept members, grouped in ascending id, ascending voxel order inside
        v, vc, n = r["voxels"], r["voxel_component"], r["n_voxels"].astype(np.int64)
        assert len(v) == st["n_voxels"] == int(n.sum()) and len(np.unique(v, axis=0)) == len(v)
        assert vc.tolist() == np.repeat(np.arange(1, len(n) + 1), n).tolist()
        assert r["first"].tolist() == (np.cumsum(n) - n).tolist()
        vps = c["cfg"]["voxels_per_side"]
        for k in range(len(n)):
            run_ = v[int(r["first"][k]): int(r["first"][k]) + int(n[k])].astype(np.int64)
            assert r["sum"][k].tolist() == run_.sum(axis=0).tolist()
            assert r["bbox_min"][k].tolist() == run_.min(axis=0).tolist() and r["bbox_max"][k].tolist() == run_.max(axis=0).tolist()
            assert r["representative"][k].tolist() == run_[0].tolist()
            b, l = run_ // vps, run_ % vps  # ascending voxel order: block (x, y, z), then linear index
            order = list(zip(b[:, 0].tolist(), b[:, 1].tolist(), b[:, 2].tolist(), (l[:, 0] + vps * (l[:, 1] + vps * l[:, 2])).tolist()))
            assert order == sorted(order)
        reps = r["representative"].astype(np.int64)
        b, l = reps // vps, reps % vps
        order = list(zip(b[:, 0].tolist(), b[:, 1].tolist(), b[:, 2].tolist(), (l[:, 0] + vps * (l[:, 1] + vps * l[:, 2])).tolist()))
        assert order == sorted(order) and len(set(order)) == len(order)
        # want_voxels = 0 changes nothing else
        q = sc.replica_of(c, i, want_voxels=False)
        assert "voxels" not in q and q["stats"] == st and all(q[k].tobytes() == r[k].tobytes() for k, _, _ in sr.COMPONENT_FIELDS)


def test_named_expectations():
    c = sc.BY_NAME["pairs"]
    for i, run in enumerate(c["runs"]):
        r = sc.replica_of(c, i)
        comp = {tuple(v): int(k) for v, k in zip(r["voxels"].tolist(), r["voxel_component"].tolist())}
        for kind, a, b in c["pairs"]:
            joined = {"face": True, "edge": run["connectivity"] >= 18, "corner": run["connectivity"] == 26}[kind]
            assert (comp[a] == comp[b]) == joined, (kind, a, b, run["connectivity"])
    for name in ("snake", "snake_vps8", "ring_2x2", "ring_corner", "big"):
        c = sc.BY_NAME[name]
        r = sc.replica_of(c, 0)
        assert int(r["n_voxels"].sum()) == c["n_voxels"], name
    big = sc.replica_of(sc.BY_NAME["big"], 0)
    assert big["n_voxels"].tolist() == [8 * 16 ** 3] * 2 and (np.abs(big["sum"]) > 2 ** 32).all()
    assert big["bbox_min"][0].tolist() == [-(1 << 20) * 16] * 3 and big["bbox_max"][1].tolist() == [(1 << 20) * 16 - 1] * 3
    f = sc.BY_NAME["filter"]
    for i, run in enumerate(f["runs"]):
        r = sc.replica_of(f, i)
        assert r["n_voxels"].tolist() == run["sizes"] and r["stats"]["n_too_small"] == run["small"] and r["stats"]["n_too_large"] == run["large"]
    o = sc.BY_NAME["order"]
    r = sc.replica_of(o, 0)
    assert [sc.block_of(v, 16) for v in r["representative"].tolist()] == o["blocks"]


def _partition(r):
    return {tuple(v): int(k) for v, k in zip(r["voxels"].tolist(), r["voxel_component"].tolist())}


def _refines(fine, coarse):
    """every component of `fine` lies inside one component of `coarse`"""
    image = {}
    for v, k in fine.items():
        if image.setdefault(k, coarse[v]) != coarse[v]:
            return False
    return set(fine) == set(coarse)


@pytest.mark.parametrize("name", ["rich", "rich_vps8", "pairs", "zigzag_edge"])
def test_refinement_across_connectivity_and_by_label(name):
    c = sc.BY_NAME[name]
    f = ck.config_fields(c["cfg"])
    res = {(conn, bl): sr.segment(f, *c["now"], connectivity=conn, by_label=bl, min_weight=0.5) for conn in (6, 18, 26) for bl in (False, True)}
    for bl in (False, True):
        p6, p18, p26 = (_partition(res[(conn, bl)]) for conn in (6, 18, 26))
        assert _refines(p6, p18) and _refines(p18, p26)
        n = [res[(conn, bl)]["stats"]["n_components"] for conn in (6, 18, 26)]
        assert n[0] >= n[1] >= n[2] >= 1
    for conn in (6, 18, 26):
        assert _refines(_partition(res[(conn, True)]), _partition(res[(conn, False)]))
        assert res[(conn, True)]["stats"]["n_components"] >= res[(conn, False)]["stats"]["n_components"]


@pytest.mark.parametrize("name", ["rich_vps8", "zigzag_face", "filter"])
def test_shift_and_permutation(name):
    c = sc.BY_NAME[name]
    f = ck.config_fields(c["cfg"])
    idx, L = c["now"]
    kw = sc.request_of(c["runs"][0])
    base = sr.segment(f, idx, L, **kw)
    shift = np.array([-7, 3, 11], np.int32)
    moved = sr.segment(f, idx + shift, L, **kw)
    dv = shift.astype(np.int64) * f["voxels_per_side"]
    for k, _, _ in sr.COMPONENT_FIELDS + sr.VOXEL_FIELDS:
        want = base[k]
        if k in ("bbox_min", "bbox_max", "representative", "voxels"):
            want = (base[k].astype(np.int64) + dv).astype(np.int32)
        elif k == "sum":
            want = base[k] + dv * base["n_voxels"].astype(np.int64)[:, None]
        assert moved[k].tobytes() == want.tobytes(), k
    assert moved["stats"] == base["stats"]
    perm = np.random.default_rng(5).permutation(len(idx))
    again = sr.segment(f, idx[perm], {k: v[perm] for k, v in L.items()}, **kw)
    assert again["stats"] == base["stats"] and all(again[k].tobytes() == base[k].tobytes() for k, _, _ in sr.COMPONENT_FIELDS + sr.VOXEL_FIELDS)


def _closure_by_min_propagation(c, run):
    """the partition by repeated min-propagation over a dense array of the map's bounding box: every member takes the least id
    among itself and its neighbours until nothing changes (shares nothing with the flood fill but the member rule)"""
    f = ck.config_fields(c["cfg"])
    kw = sc.request_of(run)
    g, lab, _ = sr.members(f, *c["now"], min_weight=kw.get("min_weight", 0.0), surface_distance=kw.get("surface_distance", 0.0),
                           mesh_min_weight=sc.MESH_MIN_WEIGHT)
    lo = g.min(axis=0) - 1
    dims = tuple((g.max(axis=0) - lo + 2).tolist())
    big = np.iinfo(np.int64).max
    ids = np.full(dims, big, np.int64)
    labels = np.full(dims, -1, np.int64)
    p = g - lo
    ids[p[:, 0], p[:, 1], p[:, 2]] = np.arange(len(g))
    labels[p[:, 0], p[:, 1], p[:, 2]] = lab if kw.get("by_label", True) and f["with_semantics"] else 0
    member = ids != big
    core = (slice(1, -1),) * 3
    while True:
        best = ids.copy()
        for d in sr.offsets(kw.get("connectivity", 26)):
            src = tuple(slice(1 + d[a], dims[a] - 1 + d[a]) for a in range(3))
            ok = member[core] & member[src] & (labels[core] == labels[src])
            best[core] = np.where(ok, np.minimum(best[core], ids[src]), best[core])
        if (best == ids).all():
            break
        ids = best
    return {tuple(v): int(ids[tuple(q)]) for v, q in zip(g.tolist(), p.tolist())}


@pytest.mark.parametrize("name,run", [("rich_vps8", 0), ("rich_vps8", 3), ("rich_vps8", 5), ("checker_vps8", 1), ("snake_vps8", 0)])
def test_closure(name, run):
    c = sc.BY_NAME[name]
    r = sc.replica_of(c, run)
    assert r["stats"]["n_components"] == r["stats"]["n_components_all"]  # (no size filter in these runs)
    want = _closure_by_min_propagation(c, c["runs"][run])
    got = _partition(r)
    assert _refines(got, want) and _refines(want, got)
    assert len(set(want.values())) == r["stats"]["n_components"]
