"""-m "not gpu": tests/travel_replica.py -- the restatement of khr_travel_field (ASSUMPTIONS.md A.22) the device is held to -- held
itself to the hand numbers of tests/travel_cases.py, to a second, independent restatement (whole-grid Bellman-Ford sweeps over 64-bit
keys) and to the invariants of its paths; hydra::TravelConfig on its yaml keys."""
import os
import subprocess

import numpy as np
import pytest

import travel_cases as tc
import travel_replica as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "khronos_amd", "lib", "host_selftest")
NAMES = sorted(tc.BUILDERS)


@pytest.mark.parametrize("connectivity", tc.CONNECTIVITIES)
@pytest.mark.parametrize("name", NAMES)
def test_the_replica_gives_the_hand_numbers_and_agrees_with_bellman_ford(name, connectivity):
    c = tc.built(name)
    res = tc.expected(name, connectivity)
    tc.check_hand_numbers(name, connectivity, res)
    cost, goal = tr.bellman_ford(c["origin"], c["distance"], c["status"], c["goals"], **dict(c["kw"], connectivity=connectivity))
    assert np.array_equal(cost, res["cost"]) and np.array_equal(goal, res["goal"])
    reached = res["cost"] != tr.UNREACHED
    assert ((res["parent"] == 255) == ~reached).all() and ((res["parent"] == 13) == (res["cost"] == 0)).all()
    assert (res["goal"][~reached] == -1).all() and not reached[~res["traversable"]].any()


def test_the_long_serpentine_needs_three_waits_by_its_shape():
    nx, ny = tc.long_serpentine_dims(8, 8)
    assert (nx, ny) == (17, 21)
    c = tc.serpentine(nx, ny)
    res = tr.travel_field(c["origin"], c["distance"], c["status"], c["goals"], **c["kw"])
    assert res["stats"]["n_reached"] == res["stats"]["n_traversable"] == int(tc.serpentine_mask(nx, ny).sum())
    # the far end's path walks every full row: (rows - 1) crossings of the two tile faces inside a row
    path = tr.travel_paths(c["origin"], res, [(0 if ((ny - 1) // 2) % 2 == 0 else nx - 1, ny - 1, 0)])["cells"]
    faces = int((np.diff(path[:, 0] // 8) != 0).sum())
    assert faces > 2 * 8


@pytest.mark.parametrize("connectivity", tc.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["wall", "random", "serpentine", "pocket_own_goal", "wall_negative_origin"])
def test_paths_step_to_adjacent_cells_and_lose_exactly_the_moves_weight(name, connectivity):
    c = tc.built(name)
    res = tc.expected(name, connectivity)
    o = np.asarray(c["origin"])
    nx, ny, nz = c["dims"]
    rng = np.random.default_rng(3)
    starts = np.stack([rng.integers(0, nx, 24), rng.integers(0, ny, 24), rng.integers(0, nz, 24)], 1) + o
    starts = np.concatenate([starts, c["goals"][:1], o[None] + (nx, 0, 0), o[None] - (1, 0, 0)])
    p = tr.travel_paths(c["origin"], res, starts)
    weights = {(dx, dy, dz): w for dx, dy, dz, w, _ in tr.moves(connectivity)}
    some = 0
    for i, s in enumerate(starts):
        cells = p["cells"][p["offsets"][i]:p["offsets"][i + 1]]
        x, y, z = s - o
        inside = 0 <= x < nx and 0 <= y < ny and 0 <= z < nz
        if not inside or res["cost"][z, y, x] == tr.UNREACHED:
            assert len(cells) == 0 and p["path_cost"][i] == tr.UNREACHED and p["path_goal"][i] == -1
            continue
        some += 1
        assert tuple(cells[0]) == tuple(s) and p["path_cost"][i] == res["cost"][z, y, x] and p["path_goal"][i] == res["goal"][z, y, x]
        local = cells - o
        costs = [int(res["cost"][q[2], q[1], q[0]]) for q in local]
        for a, b, ca, cb in zip(local[:-1], local[1:], costs[:-1], costs[1:]):
            assert ca - cb == weights[tuple(int(v) for v in b - a)]   # (a KeyError: not a move of this connectivity)
        assert costs[-1] == 0 and tuple(cells[-1]) == tuple(c["goals"][p["path_goal"][i]])
    assert some >= 2
    if name == "wall" and connectivity == 26:
        q = tr.travel_paths(c["origin"], res, [tc.WALL_PATH_START])
        assert len(q["cells"]) == tc.WALL_PATH_CELLS


def test_allow_unknown_nan_and_the_obstacle_class():
    distance = np.array([[[1.0, 1.0, np.nan, 1.0, 1.0, 0.4, 1.0]]], np.float32)
    status = np.array([[[1, 0, 1, 1, 3, 1, 1]]], np.uint8)
    assert tr.traversable(distance, status, 0.5).tolist() == [[[True, False, False, True, False, False, True]]]
    assert tr.traversable(distance, status, 0.5, True).tolist() == [[[True, True, False, True, False, False, True]]]
    res = tr.travel_field((0, 0, 0), distance, status, [(0, 0, 0)], 0.5, 6, allow_unknown=True)
    assert res["cost"][0, 0].tolist() == [0, 10] + [tr.UNREACHED] * 5


def test_travel_config_reads_its_yaml_keys():
    """hydra::TravelConfig (khronos_amd/host/hydra_compat.h) through host_selftest --travel-config"""
    out = subprocess.run([SELFTEST, "--travel-config"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    kv = dict(t.split("=") for t in out.stdout.split())
    assert np.float32(kv.pop("clearance")) == np.float32(0.35)
    # 50 m over cells of 0.2 m: 250 cells of 10 each
    assert kv == {"connectivity": "18", "allow_unknown": "1", "max_cost": "2500", "default_connectivity": "26", "default_max_cost": "0", "bad_connectivity": "rejected"}
