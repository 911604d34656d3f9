"""A plain restatement of khr_travel_field and khr_travel_paths (ASSUMPTIONS.md A.22): a heap Dijkstra over (cost, goal) pairs, the
parent rule, and the path walk, in numpy and Python.  Arrays are indexed [z, y, x]; cells and goals are global (x, y, z)."""
import heapq

import numpy as np

UNREACHED = 0xFFFFFFFF
OBSERVED, OBSTACLE = 1, 2
WEIGHT = {1: 10, 2: 14, 3: 17}


def moves(connectivity):
    """(dx, dy, dz, weight, code) of the connectivity's moves in the order dz outer, dy middle, dx inner"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nz = (dx != 0) + (dy != 0) + (dz != 0)
                if 1 <= nz <= most:
                    out.append((dx, dy, dz, WEIGHT[nz], (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)))
    return out


def traversable(distance, status, clearance, allow_unknown=False):
    distance, status = np.asarray(distance, np.float32), np.asarray(status, np.uint8)
    observed = (status & OBSERVED) != 0
    cls = np.where(observed, (status & OBSTACLE) == 0, bool(allow_unknown))
    with np.errstate(invalid="ignore"):
        return cls & (distance >= np.float32(clearance))


def usable_goals(trav, origin, goals):
    """[(goal index, local x, y, z)] of the goals inside the box on traversable cells"""
    nz, ny, nx = trav.shape
    out = []
    for g, cell in enumerate(np.asarray(goals, np.int64).reshape(-1, 3)):
        x, y, z = (int(cell[k]) - int(origin[k]) for k in range(3))
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and trav[z, y, x]:
            out.append((g, x, y, z))
    return out


def parents(trav, cost, goal, connectivity):
    nz, ny, nx = trav.shape
    mv = moves(connectivity)
    parent = np.full(trav.shape, 255, np.uint8)
    for z, y, x in zip(*np.nonzero(cost != UNREACHED)):
        c = int(cost[z, y, x])
        if c == 0:
            parent[z, y, x] = 13
            continue
        for dx, dy, dz, w, code in mv:
            X, Y, Z = x + dx, y + dy, z + dz
            if 0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz and cost[Z, Y, X] != UNREACHED and int(cost[Z, Y, X]) + w == c and goal[Z, Y, X] == goal[z, y, x]:
                parent[z, y, x] = code
                break
        assert parent[z, y, x] != 255, "a reached cell without a parent"
    return parent


def travel_field(origin, distance, status, goals, clearance, connectivity=26, allow_unknown=False, max_cost=0):
    """cost uint32, goal int32, parent uint8 [z, y, x], and stats (the four words that describe the result)"""
    trav = traversable(distance, status, clearance, allow_unknown)
    nz, ny, nx = trav.shape
    mv = moves(connectivity)
    cost = np.full(trav.shape, UNREACHED, np.uint32)
    goal = np.full(trav.shape, -1, np.int32)
    best = {}
    heap = []
    used = usable_goals(trav, origin, goals)
    for g, x, y, z in used:
        if (x, y, z) not in best or (0, g) < best[(x, y, z)]:
            best[(x, y, z)] = (0, g)
            heapq.heappush(heap, (0, g, x, y, z))
    done = np.zeros(trav.shape, bool)
    while heap:
        c, g, x, y, z = heapq.heappop(heap)
        if done[z, y, x] or best[(x, y, z)] != (c, g):
            continue
        done[z, y, x] = True
        cost[z, y, x], goal[z, y, x] = c, g
        for dx, dy, dz, w, _ in mv:
            X, Y, Z = x + dx, y + dy, z + dz
            if not (0 <= X < nx and 0 <= Y < ny and 0 <= Z < nz) or not trav[Z, Y, X] or done[Z, Y, X]:
                continue
            cand = (c + w, g)
            if max_cost and cand[0] > max_cost:
                continue
            if (X, Y, Z) not in best or cand < best[(X, Y, Z)]:
                best[(X, Y, Z)] = cand
                heapq.heappush(heap, (cand[0], g, X, Y, Z))
    reached = cost != UNREACHED
    stats = {"n_traversable": int(trav.sum()), "n_goals_used": len(used), "n_reached": int(reached.sum()),
             "max_cost": int(cost[reached].max()) if reached.any() else 0}
    return {"cost": cost, "goal": goal, "parent": parents(trav, cost, goal, connectivity), "stats": stats, "traversable": trav}


RESULT_STATS = ("n_traversable", "n_goals_used", "n_reached", "max_cost")


def travel_paths(origin, field, starts):
    """offsets int64, cells (total, 3) int32 global, path_cost uint32, path_goal int32 of the walks along `parent`"""
    parent, cost, goal = field["parent"], field["cost"], field["goal"]
    nz, ny, nx = parent.shape
    starts = np.asarray(starts, np.int64).reshape(-1, 3)
    offsets, cells = [0], []
    path_cost, path_goal = np.full(len(starts), UNREACHED, np.uint32), np.full(len(starts), -1, np.int32)
    for i, s in enumerate(starts):
        x, y, z = (int(s[k]) - int(origin[k]) for k in range(3))
        if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz and parent[z, y, x] != 255:
            path_cost[i], path_goal[i] = cost[z, y, x], goal[z, y, x]
            for _ in range(parent.size):
                cells.append((origin[0] + x, origin[1] + y, origin[2] + z))
                code = int(parent[z, y, x])
                if code == 13:
                    break
                x, y, z = x + code % 3 - 1, y + (code // 3) % 3 - 1, z + code // 9 - 1
            else:
                raise AssertionError("a walk that does not end")
        offsets.append(len(cells))
    return {"offsets": np.asarray(offsets, np.int64), "cells": np.asarray(cells, np.int32).reshape(-1, 3), "path_cost": path_cost, "path_goal": path_goal}


def bellman_ford(origin, distance, status, goals, clearance, connectivity=26, allow_unknown=False, max_cost=0):
    """the same (cost, goal), independently: whole-grid sweeps over 64-bit keys cost << 32 | goal until nothing changes"""
    trav = traversable(distance, status, clearance, allow_unknown)
    nz, ny, nx = trav.shape
    far = np.uint64(0xFFFFFFFFFFFFFFFF)
    key = np.full((nz + 2, ny + 2, nx + 2), far, np.uint64)  # (a frame of unreached cells around the box)
    inner = key[1:-1, 1:-1, 1:-1]
    for g, x, y, z in reversed(usable_goals(trav, origin, goals)):
        inner[z, y, x] = min(int(inner[z, y, x]), g)
    mv = moves(connectivity)
    limit = max_cost if max_cost else UNREACHED - 1
    while True:
        new = inner.copy()
        for dx, dy, dz, w, _ in mv:
            nb = key[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
            ok = (nb != far) & trav
            cand = np.where(ok, nb + (np.uint64(w) << np.uint64(32)), far)
            cand = np.where((cand >> np.uint64(32)) <= np.uint64(limit), cand, far)
            new = np.minimum(new, cand)
        if (new == inner).all():
            break
        inner[...] = new
    reached = inner != far
    cost = np.where(reached, inner >> np.uint64(32), UNREACHED).astype(np.uint32)
    goal = np.where(reached, (inner & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return cost, goal
