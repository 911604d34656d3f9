"""-m "not gpu": tests/weld_replica.py, the numpy restatement of khr_weld_mesh (ASSUMPTIONS.md A.16) that the device is compared
with in tests/test_gpu_weld_mesh.py, on the CPU oracle's meshes of the hand-built maps: equal to a plain sequential first-come
weld, the definition's invariants, and the saving the feature exists for.
Measured with the oracle's meshes (printed below; asserted with margin): the sphere at one voxel keeps 0.092 of the soup's vertices
and 0.55 of its faces at both block sizes; all_cases(8) at two voxels keeps exactly 512 vertices, one per cell of its box."""
import numpy as np
import pytest

import mesh_cases as mc
import weld_replica as wr
from test_cpu_mesh_cases import oracle_mesh

VS = mc.VOXEL_SIZE
RESOLUTIONS = {"voxel": VS, "half": VS / 2, "two": 2 * VS, "5mm": 0.005}
MAPS = {"all_cases8": lambda: (8,) + mc.all_cases(8), "dense8": lambda: (8,) + mc.dense(8), "sphere8": lambda: (8,) + wr.sphere(8),
        "sphere16": lambda: (16,) + wr.sphere(16)}
_meshes = {}


def soup_of(name):
    if name not in _meshes:
        m = oracle_mesh(*MAPS[name]())
        assert len(m["points"]) > 0 and len(m["points"]) % 3 == 0
        for a in m.values():
            a.setflags(write=False)
        _meshes[name] = m
    return _meshes[name]


def assert_same(a, b, what):
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])
    for k in wr.FIELDS + ("faces", "soup_to_vertex"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("res", list(RESOLUTIONS))
@pytest.mark.parametrize("name", list(MAPS))
def test_replica_equals_the_sequential_weld(name, res):
    soup, r = soup_of(name), RESOLUTIONS[res]
    w = wr.weld(soup, r)
    print(name, res, w["stats"])
    assert_same(w, wr.weld_sequential(soup, r), (name, res))


@pytest.mark.parametrize("res", list(RESOLUTIONS))
@pytest.mark.parametrize("name", list(MAPS))
def test_invariants(name, res):
    soup, r = soup_of(name), RESOLUTIONS[res]
    w = wr.weld(soup, r)
    st, f, s2v = w["stats"], w["faces"], w["soup_to_vertex"]
    n = len(soup["points"])
    assert st["n_soup_vertices"] == n == len(s2v) and st["n_vertices"] == len(w["points"]) and st["n_faces"] == len(f)
    assert st["n_faces"] + st["n_degenerate_faces"] == n // 3
    assert f.dtype == np.uint32 and s2v.dtype == np.uint32
    # kept faces have three distinct indices, all of them welded vertices
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all() and (f < st["n_vertices"]).all()
    # every soup vertex lies in the cell of the welded vertex it maps to
    assert (wr.cells(w["points"][s2v], r) == wr.cells(soup["points"], r)).all()
    # no two welded vertices share a cell
    assert len(np.unique(wr.keys(w["points"], r))) == st["n_vertices"]
    # the representatives ascend: welded vertex j is the first soup vertex that maps to j, and those first indices ascend
    first = np.full(st["n_vertices"], n, np.int64)
    np.minimum.at(first, s2v, np.arange(n))
    assert (np.diff(first) > 0).all()
    for k in wr.FIELDS:
        assert w[k].tobytes() == soup[k][first].tobytes(), k
    # the kept faces are the soup's non-degenerate ones in soup order, with their winding
    tri = s2v.reshape(-1, 3)
    assert f.tobytes() == tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])].tobytes()


@pytest.mark.parametrize("vps", [8, 16])
def test_the_sphere_shrinks_to_a_fifth(vps):
    st = wr.weld(soup_of("sphere%d" % vps), VS)["stats"]
    print(vps, st, st["n_vertices"] / st["n_soup_vertices"], st["n_faces"] / (st["n_soup_vertices"] // 3))
    assert st["n_vertices"] <= st["n_soup_vertices"] / 5
    assert st["n_faces"] >= 0.4 * (st["n_soup_vertices"] // 3)


def test_two_voxels_leave_one_vertex_per_cell_of_the_box():
    st = wr.weld(soup_of("all_cases8"), 2 * VS)["stats"]
    print(st)
    assert st["n_vertices"] <= 512


def test_out_of_range_is_reported():
    with pytest.raises(wr.OutOfRange):
        wr.weld(soup_of("all_cases8"), 0.001)   # cell index about -1.6 M against the limit of 2^20
    bad = {k: np.array(v[:3]) for k, v in soup_of("all_cases8").items()}
    bad["points"][1, 2] = np.nan
    with pytest.raises(wr.OutOfRange):
        wr.weld(bad, VS)


def test_empty_soup():
    empty = {"points": np.zeros((0, 3), np.float32), "colors": np.zeros((0, 4), np.uint8), "labels": np.zeros(0, np.uint32),
             "first_seen": np.zeros(0, np.uint64), "stamps": np.zeros(0, np.uint64)}
    w = wr.weld(empty, VS)
    assert w["stats"] == {"n_soup_vertices": 0, "n_vertices": 0, "n_faces": 0, "n_degenerate_faces": 0}
    assert w["faces"].shape == (0, 3) and w["soup_to_vertex"].shape == (0,)
