"""Hand-built fields for khr_travel_field (ASSUMPTIONS.md A.22) with the numbers worked out on the CPU when the call was specified;
tests/test_cpu_travel_replica.py holds tests/travel_replica.py to them, tests/test_gpu_travel_field.py the device.  A field is a
traversable mask [z, y, x]: distance 1.0 on its cells and 0.0 on the others, status OBSERVED, clearance 0.5."""
import functools

import numpy as np

import travel_replica as tr

CLEARANCE = 0.5
CONNECTIVITIES = (6, 18, 26)
NEGATIVE_ORIGIN = (-37, 5, -3)


def field_of(mask):
    mask = np.asarray(mask, bool)
    return np.where(mask, np.float32(1.0), np.float32(0.0)).astype(np.float32), np.full(mask.shape, tr.OBSERVED, np.uint8)


def case(mask, goals, origin=(0, 0, 0), **kw):
    """goals are given box-local and moved by the origin"""
    distance, status = field_of(mask)
    nz, ny, nx = distance.shape
    goals = np.asarray(goals, np.int32).reshape(-1, 3) + np.asarray(origin, np.int32)
    return dict(origin=tuple(origin), dims=(nx, ny, nz), distance=distance, status=status, goals=goals, kw=dict(clearance=CLEARANCE, **kw))


def open_box(origin=(0, 0, 0)):
    return case(np.ones((12, 12, 12), bool), [(0, 0, 0)], origin)


def wall(origin=(0, 0, 0), **kw):
    mask = np.ones((1, 17, 24), bool)
    mask[0, 0:16, 12] = False
    return case(mask, [(0, 0, 0)], origin, **kw)


def serpentine_mask(nx, ny):
    """rows y = 0, 2, .. full; row 2r + 1 has the one cell x = nx - 1 (r even) or x = 0 (r odd)"""
    mask = np.zeros((1, ny, nx), bool)
    mask[0, 0::2, :] = True
    for r in range((ny - 1) // 2):
        mask[0, 2 * r + 1, nx - 1 if r % 2 == 0 else 0] = True
    return mask


def serpentine(nx=33, ny=33, origin=(0, 0, 0)):
    return case(serpentine_mask(nx, ny), [(0, 0, 0)], origin)


def long_serpentine_dims(tile_edge, rounds_per_wait):
    """A key crosses at most one tile face per round.  Every full row of a serpentine 2 * edge + 1 cells wide is walked from end to
    end and crosses 2 faces; rounds_per_wait + 2 such rows need more than 2 * rounds_per_wait rounds, that is at least 3 waits."""
    return 2 * tile_edge + 1, 2 * (rounds_per_wait + 2) + 1


def tie(duplicate=False):
    goals = [(8, 0, 0), (0, 0, 0)] + ([(8, 0, 0)] if duplicate else [])
    return case(np.ones((1, 1, 9), bool), goals)


TIE_COST = [0, 10, 20, 30, 40, 30, 20, 10, 0]
TIE_GOAL = [1, 1, 1, 1, 0, 0, 0, 0, 0]


def pocket(own_goal=False):
    """the cell (2, 2, 2) of a 5^3 box, walled in on all 26 sides"""
    mask = np.ones((5, 5, 5), bool)
    mask[1:4, 1:4, 1:4] = False
    mask[2, 2, 2] = True
    return case(mask, [(0, 0, 0)] + ([(2, 2, 2)] if own_goal else []), NEGATIVE_ORIGIN)


def random(origin=NEGATIVE_ORIGIN, **kw):
    mask = np.random.default_rng(7).random((20, 33, 40)) >= 0.35
    return case(mask, [(0, 0, 0), (39, 32, 19), (20, 16, 10), (5, 30, 3)], origin, **kw)


# the counts of the random field as the issue states them: traversable cells, then per connectivity reached cells, greatest cost and
# cells per goal.  They belong to the field numpy's default_rng(7) draws (PCG64, unchanged since numpy 1.17); were an installed numpy
# to draw another field, the replica's own counts hold and the comparison with the replica stays what it is.
RANDOM_TRAVERSABLE = 17175
RANDOM_COUNTS = {6: (17124, 460, [2269, 1999, 12856]), 26: (17175, 291, [1901, 1760, 13514])}

# (case, connectivity) -> {local cell: cost}
HAND_COSTS = {
    ("open", 26): {(11, 11, 11): 187, (11, 0, 0): 110, (11, 5, 0): 130},
    ("wall", 6): {(23, 0, 0): 550, (12, 16, 0): 280}, ("wall", 18): {(23, 0, 0): 412, (12, 16, 0): 208}, ("wall", 26): {(23, 0, 0): 412, (12, 16, 0): 208},
    ("serpentine", 6): {(32, 32, 0): 5760, (0, 32, 0): 5440}, ("serpentine", 18): {(32, 32, 0): 5568, (0, 32, 0): 5254},
    ("serpentine", 26): {(32, 32, 0): 5568, (0, 32, 0): 5254},
}
WALL_PATH_START, WALL_PATH_CELLS = (23, 0, 0), 33
SERPENTINE_TRAVERSABLE = 577

BUILDERS = {"open": open_box, "wall": wall, "serpentine": serpentine, "tie": tie, "tie_duplicate": lambda: tie(True), "pocket": pocket,
            "pocket_own_goal": lambda: pocket(True), "random": random, "wall_max_cost_100": lambda: wall(max_cost=100),
            "wall_negative_origin": lambda: wall(NEGATIVE_ORIGIN), "open_negative_origin": lambda: open_box(NEGATIVE_ORIGIN)}


@functools.lru_cache(maxsize=None)
def built(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name, connectivity):
    """the replica's result of a case, computed once and shared; nobody writes into it"""
    c = built(name)
    kw = dict(c["kw"], connectivity=connectivity)
    out = tr.travel_field(c["origin"], c["distance"], c["status"], c["goals"], **kw)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def check_hand_numbers(name, connectivity, res):
    """the issue's numbers for case `name` on a result dict (cost / goal / parent [z, y, x], stats)"""
    cost, goal, parent, stats = res["cost"], res["goal"], res["parent"], res["stats"]
    base = name.replace("_negative_origin", "")
    for (x, y, z), want in HAND_COSTS.get((base, connectivity), {}).items():
        assert int(cost[z, y, x]) == want, (name, connectivity, (x, y, z), int(cost[z, y, x]), want)
    if name == "serpentine":
        assert stats["n_traversable"] == SERPENTINE_TRAVERSABLE
        blocked = ~serpentine_mask(33, 33)
        assert (cost[blocked] == tr.UNREACHED).all() and (goal[blocked] == -1).all() and (parent[blocked] == 255).all()
    if name in ("tie", "tie_duplicate"):
        assert cost[0, 0].tolist() == TIE_COST and goal[0, 0].tolist() == TIE_GOAL
    if name == "pocket":
        assert cost[2, 2, 2] == tr.UNREACHED and goal[2, 2, 2] == -1 and parent[2, 2, 2] == 255
        assert stats["n_reached"] == stats["n_traversable"] - 1
    if name == "pocket_own_goal":
        assert cost[2, 2, 2] == 0 and goal[2, 2, 2] == 1 and parent[2, 2, 2] == 13 and stats["n_goals_used"] == 2
    if name == "random" and int(built("random")["distance"].sum()) == RANDOM_TRAVERSABLE:
        assert stats["n_traversable"] == RANDOM_TRAVERSABLE and stats["n_goals_used"] == 3
        if connectivity in RANDOM_COUNTS:
            reached, top, per_goal = RANDOM_COUNTS[connectivity]
            assert (stats["n_reached"], stats["max_cost"]) == (reached, top), stats
            assert [int((goal == g).sum()) for g in range(3)] == per_goal and not (goal == 3).any()
    if name == "wall_max_cost_100":
        full = expected("wall", connectivity)["cost"]
        assert ((cost != tr.UNREACHED) == (full <= 100)).all() and (cost[cost != tr.UNREACHED] == full[full <= 100]).all()
