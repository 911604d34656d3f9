"""-m "not gpu": the host stages of the motion detector's frame finish (khronos_amd/csrc/khr_md_host.h: cluster order, merge
groups from the device's overlap rows, size filter and ids, the seed-graph walk) against the oracle, through a stand-alone program
(tests/md_host_selftest.cpp) built with the address and undefined-behaviour sanitizers.  Every case starts from a hand-made
voxel-key image.  The compact lists, the adjacency and the component records the device would hand to the host are derived here
in numpy from their definitions; the program's final ids are painted by k_md_paint's rule and the image has to equal the
oracle's."""
import os
import subprocess

import numpy as np
import pytest

from khronos_amd import default_config
from oracle import pyoracle as po
from oracle.np_oracle import _neighbour_offsets
from test_cpu_motion_kat import SEED, _image, key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 128, 64
NONE, SEED_REF = 0xFFFFFFFF, 0x80000000
BIAS = 1 << 20


def _xyz(k):
    return (k & 0x1FFFFF) - BIAS, ((k >> 21) & 0x1FFFFF) - BIAS, ((k >> 42) & 0x1FFFFF) - BIAS


def _lists(img, nn, rng):
    """What k_md_compact / k_md_adjacency leave: seed and boundary voxel lists (key, pixel count) in no particular order and
    adj[s][j] = 0xffffffff for none, bit 31 | seed id, or a boundary id (an occupied non-seed voxel next to a seed)."""
    keys, counts = np.unique(img.ravel()[img.ravel() != 0], return_counts=True)
    keys, counts = [int(k) for k in keys], [int(n) for n in counts]
    seeds = [(k & ~SEED, n) for k, n in zip(keys, counts) if k & SEED]
    seeds = [seeds[i] for i in rng.permutation(len(seeds))]
    occupied = {k: n for k, n in zip(keys, counts) if not k & SEED}
    seed_id = {k: i for i, (k, _) in enumerate(seeds)}
    bnd_id, adj = {}, []
    for k, _ in seeds:
        x, y, z = _xyz(k)
        row = []
        for dx, dy, dz in _neighbour_offsets(nn):
            nk = key(x + dx, y + dy, z + dz)
            if nk in seed_id:
                row.append(SEED_REF | seed_id[nk])
            elif nk in occupied:
                row.append(bnd_id.setdefault(nk, len(bnd_id)))
            else:
                row.append(NONE)
        adj.append(row)
    bnd = [(k, occupied[k]) for k in bnd_id]  # (dicts keep insertion order: position = id)
    return seeds, bnd, adj


def _components(seeds, adj):
    parent = list(range(len(seeds)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for s, row in enumerate(adj):
        for a in row:
            if a != NONE and a & SEED_REF:
                parent[find(s)] = find(a & 0x7FFFFFFF)
    roots = sorted({find(s) for s in range(len(seeds))}, reverse=True)  # (any numbering will do)
    return [roots.index(find(s)) for s in range(len(seeds))], len(roots)


def _records(seeds, bnd, adj, comp_of, R, sep):
    """Component records by their definition: the pixel list's length with the reference's duplicates, canonKey of the first seed
    in (x, y, z) order, the box over seed and adjacent boundary voxels, and -- where the device computes them -- the overlap rows."""
    recs = [dict(px=0, min_key=1 << 63, vox=set()) for _ in range(R)]
    for s, (k, n) in enumerate(seeds):
        r = recs[comp_of[s]]
        x, y, z = _xyz(k)
        r["px"] += n
        r["min_key"] = min(r["min_key"], ((x + BIAS) << 42) | ((y + BIAS) << 21) | (z + BIAS))
        r["vox"].add((x, y, z))
        for a in adj[s]:
            if a != NONE and not a & SEED_REF:
                r["px"] += bnd[a][1]
                r["vox"].add(_xyz(bnd[a][0]))
    with_rows = 0.0 < sep <= 2.0 and R <= 64
    for i, r in enumerate(recs):
        v = np.array(sorted(r["vox"]), np.int64)
        r["lo"], r["hi"], r["v"], r["row"] = v.min(0), v.max(0), v, 0
    if with_rows:
        for i, a in enumerate(recs):
            for j, b in enumerate(recs):
                n2 = ((a["v"][:, None, :] - b["v"][None, :, :]) ** 2).sum(-1)
                if (np.floor(np.sqrt(n2.astype(np.float64))).astype(np.float32) < np.float32(sep)).any():
                    a["row"] |= 1 << j
            if R < 64:
                a["row"] |= 1 << 63  # (bits at or above R carry no meaning)
    return recs, with_rows


def _paint(img, seeds, bnd, seed_final, bnd_final):
    """k_md_paint: a seed pixel takes its voxel's entry of seed_final, any other pixel its voxel's entry of bnd_final when the voxel
    is in the boundary list, and 0 otherwise."""
    lut = {k | SEED: f for (k, _), f in zip(seeds, seed_final)}
    lut.update({k: f for (k, _), f in zip(bnd, bnd_final)})
    keys, inv = np.unique(img.ravel(), return_inverse=True)
    return np.array([lut.get(int(k), 0) for k in keys], np.int32)[inv.ravel()].reshape(img.shape)


def _blobs(rng):
    vox = np.unique(rng.integers(0, 12, (400, 3)), axis=0)
    return [(key(int(v[0]), int(v[1]), int(v[2]), bool(rng.uniform() < 0.35)), int(rng.integers(1, 7))) for v in vox]


PAIR = [(key(0, 0, 0, True), 3), (key(2, 0, 0, True), 3), (key(1, 0, 0), 5)]  # two seeds that only share a boundary voxel
TWO_ADJACENT = [(key(0, 0, 0, True), 3), (key(1, 0, 0, True), 3), (key(0, 1, 0), 5)]


def _cases():
    c = {}
    # the seven of tests/test_gpu_parity.py::test_motion_clustering_from_key_images
    rng = np.random.default_rng(8)
    c["boundary_counts"] = (TWO_ADJACENT, dict(md_min_cluster_size=16, md_min_separation_distance=0.5))
    c["truncated_norm_3.2"] = ([(key(0, 0, 0, True), 4), (key(2, 2, 2, True), 4)], dict(md_min_cluster_size=1, md_min_separation_distance=3.2))
    c["300_clusters"] = ([(key(4 * i, 0, 0, True), 3) for i in range(300)], dict(md_min_cluster_size=1, md_min_separation_distance=1.0))
    c["1500_components"] = ([(key(3 * (i % 40), 3 * (i // 40), 7, True), 2) for i in range(1500)],
                            dict(md_min_cluster_size=1, md_min_separation_distance=1.0))
    c["pair_sep0"] = (PAIR, dict(md_min_cluster_size=1, md_min_separation_distance=0.0))
    runs = _blobs(rng)
    c["blobs_min4"] = (runs, dict(md_min_cluster_size=4, md_min_separation_distance=1.0))
    c["blobs_min1_nn6_sep2.5"] = (runs, dict(md_min_cluster_size=1, md_min_separation_distance=2.5, md_neighbor_connectivity=6))
    # the situations of tests/test_cpu_motion_kat.py
    for lo, hi in ((16, 1000), (17, 1000), (1, 15), (1, 16)):
        c["size_filter_%d_%d" % (lo, hi)] = (TWO_ADJACENT, dict(md_min_cluster_size=lo, md_max_cluster_size=hi, md_min_separation_distance=0.5))
    c["lone_occupied_voxel"] = (TWO_ADJACENT + [(key(5, 5, 5), 7)], dict(md_min_cluster_size=1, md_min_separation_distance=0.5))
    for sep in (3.0, 3.5):
        c["gap_of_two_sep%.1f" % sep] = ([(key(0, 0, 0, True), 4), (key(3, 0, 0, True), 4)], dict(md_min_cluster_size=1, md_min_separation_distance=sep))
    c["truncated_norm_3.0"] = ([(key(0, 0, 0, True), 4), (key(2, 2, 2, True), 4)], dict(md_min_cluster_size=1, md_min_separation_distance=3.0))
    c["pair_sep1"] = (PAIR, dict(md_min_cluster_size=1, md_min_separation_distance=1.0))
    # the pair among isolated seeds: 12 components (rows) and 102 (more than the rows hold)
    for n in (10, 100):
        c["pair_and_%d" % n] = (PAIR + [(key(4 * i, 8, 0, True), 3) for i in range(n)], dict(md_min_cluster_size=1, md_min_separation_distance=1.0))
    # random blobs, every connectivity and separations on both sides of the rows' range
    for nn in (6, 18, 26):
        for sep in (0.0, 0.5, 1.0, 2.0, 2.5):
            c["blobs_nn%d_sep%.1f" % (nn, sep)] = (_blobs(np.random.default_rng(100 * nn + int(10 * sep))),
                                                   dict(md_min_cluster_size=1 if nn == 18 else 3, md_min_separation_distance=sep,
                                                        md_neighbor_connectivity=nn))
    # sparse blobs: few enough components for the rows, and merges among them
    for i, sep in enumerate((1.0, 2.0)):
        rng = np.random.default_rng(40 + i)
        vox = np.unique(rng.integers(0, 6, (40, 3)), axis=0)
        c["sparse_sep%.1f" % sep] = ([(key(int(v[0]), int(v[1]), int(v[2]), bool(rng.uniform() < 0.5)), int(rng.integers(1, 7))) for v in vox],
                                     dict(md_min_cluster_size=2, md_min_separation_distance=sep))
    # more than 255 kept clusters behind a merge: saturation
    c["saturation_behind_merge"] = (PAIR + [(key(4 * i, 8, 0, True), 2) for i in range(270)], dict(md_min_cluster_size=1, md_min_separation_distance=1.0))
    # the first cluster (2 pixels) is filtered out, the ids of the merged pair behind it and of the last cluster move up
    c["filter_shifts_ids"] = ([(key(0, 0, 0, True), 2), (key(10, 0, 0, True), 3), (key(12, 0, 0, True), 3), (key(11, 0, 0), 5), (key(20, 0, 0, True), 6)],
                              dict(md_min_cluster_size=4, md_min_separation_distance=1.0))
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = tmp_path_factory.mktemp("md_host") / "md_host_selftest"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                        os.path.join(ROOT, "tests", "md_host_selftest.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def _run(exe, numbers):
    out = subprocess.run([exe], input=" ".join(str(int(x)) for x in numbers), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    res = {}
    for line in out.stdout.splitlines():
        name, *vals = line.split()
        res[name] = [int(v) for v in vals]
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_host_stages_equal_the_oracle(selftest, name):
    runs, kw = CASES[name]
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, with_tracking=1, max_blocks=64, max_frame_pixels=W * H,
                         **{"md_neighbor_connectivity": 26, **kw})
    nn, sep = int(cfg.md_neighbor_connectivity), float(cfg.md_min_separation_distance)
    img, _ = _image(W, H, runs)
    n_o, dyn_o, _ = po.OracleMap(po.config_from(cfg, 0)).detect_motion_from_keys(img)

    seeds, bnd, adj = _lists(img, nn, np.random.default_rng(len(runs)))
    comp_of, R = _components(seeds, adj)
    recs, with_rows = _records(seeds, bnd, adj, comp_of, R, sep)
    numbers = [nn, int(np.float32(sep).view(np.uint32)), cfg.md_min_cluster_size, cfg.md_max_cluster_size, len(seeds), len(bnd)]
    numbers += [k for k, _ in seeds] + [n for _, n in seeds] + [a for row in adj for a in row] + [k for k, _ in bnd] + [n for _, n in bnd]
    numbers.append(R)
    for r in recs:
        numbers += [r["px"], r["min_key"]] + [int(v) + BIAS for v in r["lo"]] + [int(v) + BIAS for v in r["hi"]] + [r["row"]]
    numbers.append(1 if with_rows else 0)
    res = _run(selftest, numbers)
    saturating = [min(i + 1, 255) for i in range(n_o)]

    # the walk
    assert res["walk"] == [n_o]
    assert res["kept"][0::2] == saturating
    assert np.array_equal(_paint(img, seeds, bnd, res["seed_final"], res["bnd_final"]), dyn_o)
    deg = [0] * len(bnd)  # seeds of KEPT clusters that list the boundary voxel
    for s, row in enumerate(adj):
        for a in row:
            if a != NONE and not a & SEED_REF and res["seed_final"][s]:
                deg[a] += 1
    assert res["bnd_deg"] == deg

    # the records: whenever motionFinish would take them -- nothing can merge, or the device's rows say what does
    assert ("records" in res) == (with_rows or res["may_merge"] == [0])
    if "records" in res:
        assert res["records"] == [n_o]
        assert res["rkept"] == res["kept"]
        seed_final = [res["comp_id"][comp_of[s]] for s in range(len(seeds))]
        bnd_final = [0] * len(bnd)  # k_md_comp_finals: the largest id among the adjacent seeds' clusters
        for s, row in enumerate(adj):
            for a in row:
                if a != NONE and not a & SEED_REF:
                    bnd_final[a] = max(bnd_final[a], seed_final[s])
        assert np.array_equal(_paint(img, seeds, bnd, seed_final, bnd_final), dyn_o)


def test_the_cases_reach_every_branch():
    """what the cases above are there for, so that a changed generator cannot quietly stop covering it"""
    seen = {}
    for name in ("pair_and_10", "pair_and_100", "300_clusters", "saturation_behind_merge", "filter_shifts_ids", "truncated_norm_3.2"):
        runs, kw = CASES[name]
        img, _ = _image(W, H, runs)
        seeds, bnd, adj = _lists(img, 26, np.random.default_rng(0))
        seen[name] = (_components(seeds, adj)[1], po.OracleMap(po.config_from(default_config(
            voxel_size=0.1, truncation_distance=0.3, with_tracking=1, max_blocks=64, max_frame_pixels=W * H, md_neighbor_connectivity=26, **kw), 0))
            .detect_motion_from_keys(img)[0])
    assert seen["pair_and_10"] == (12, 11) and seen["pair_and_100"] == (102, 101)   # components, clusters: a merge with / without rows
    assert seen["300_clusters"] == (300, 300) and seen["saturation_behind_merge"] == (272, 271)
    assert seen["filter_shifts_ids"] == (4, 2) and seen["truncated_norm_3.2"] == (2, 1)
