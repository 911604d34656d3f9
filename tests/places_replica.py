"""Plain restatement of khr_places_graph (ASSUMPTIONS.md A.21) over a field of distance / d2 / basis / site arrays [z, y, x]: a
breadth-first flood fill over a dictionary of members, the edges from a dictionary of pairs, the components by a second flood fill
over the places.  It shares nothing with the device's form (union-find per bucket, sort and reduce of pair keys).  `labels_minprop`
is a second closure -- repeated min-propagation over a dense array, restricted to buckets -- for tests/test_cpu_places_replica.py to
hold the flood fill against."""
from collections import deque

import numpy as np

f32 = np.float32
D2_LIMIT = 1 << 30
# the 26 neighbours; the 13 that raise lin = x + nx * (y + ny * z) see every unordered pair once, from its lower cell
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
FORWARD = [o for o in OFFSETS if (o[2], o[1], o[0]) > (0, 0, 0)]
STATS = ("n_members", "n_places_all", "n_edges_all", "n_components_all", "n_places", "n_edges", "n_components")
PLACE_FIELDS = ("centre", "centre_d2", "radius", "basis", "site", "n_cells", "sum", "degree", "component")
EDGE_FIELDS = ("edge_a", "edge_b", "edge_clearance_d2", "edge_n_contacts")


def members_of(distance, d2, basis, min_basis=0, min_node_distance=0.0):
    """bool [z, y, x]: basis >= min_basis (0 means 2), distance >= min_node_distance as float32, 0 <= d2 < 2^30"""
    mb = 2 if min_basis == 0 else min_basis
    return (basis.astype(np.int64) >= mb) & (distance.astype(f32) >= f32(min_node_distance)) & (d2 >= 0) & (d2 < D2_LIMIT)


def bucket_of(c, compression, floor=True):
    """the bucket of the global cell coordinate c: rounded towards minus infinity -- or, WRONG for negative cells, towards zero"""
    return c // compression if floor else int(c / compression)


def labels_flood(member, origin, compression, floor=True):
    """(place of each member cell {(x, y, z) local: place}, the members of each place in the order found): places in ascending lin
    of their representatives, which are the first cells found"""
    nz, ny, nx = member.shape
    cells = [(int(x), int(y), int(z)) for z, y, x in np.argwhere(member)]   # ascending lin
    bucket = {c: tuple(bucket_of(origin[a] + c[a], compression, floor) for a in range(3)) for c in cells}
    place_of, places = {}, []
    for c in cells:
        if c in place_of:
            continue
        place_of[c] = len(places)
        found, queue = [c], deque([c])
        while queue:
            x, y, z = queue.popleft()
            for dx, dy, dz in OFFSETS:
                q = (x + dx, y + dy, z + dz)
                if q in bucket and q not in place_of and bucket[q] == bucket[c]:
                    place_of[q] = len(places)
                    found.append(q)
                    queue.append(q)
        places.append(found)
    return place_of, places


def labels_minprop(member, origin, compression):
    """int64 [z, y, x]: the least lin of the cell's place, -1 for no member; by min-propagation sweeps until nothing changes"""
    nz, ny, nx = member.shape
    big = np.int64(1) << 40
    lab = np.where(member, np.arange(member.size, dtype=np.int64).reshape(member.shape), big)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    b = [(origin[0] + x) // compression, (origin[1] + y) // compression, (origin[2] + z) // compression]
    while True:
        before = lab.copy()
        for dx, dy, dz in OFFSETS:
            src = [slice(max(0, -d), n - max(0, d)) for d, n in ((dz, nz), (dy, ny), (dx, nx))]
            dst = [slice(max(0, d), n - max(0, -d)) for d, n in ((dz, nz), (dy, ny), (dx, nx))]
            src, dst = tuple(src), tuple(dst)
            ok = member[src] & member[dst] & (b[0][src] == b[0][dst]) & (b[1][src] == b[1][dst]) & (b[2][src] == b[2][dst])
            lab[dst] = np.where(ok, np.minimum(lab[dst], lab[src]), lab[dst])
        if np.array_equal(lab, before):
            return np.where(member, lab, -1)


def places_graph(origin, dims, distance, d2, basis, site, min_basis=0, min_node_distance=0.0, compression=4, min_component_size=1, floor=True):
    """the outputs of FusionContext.places_graph_from (without `centroid`); the arrays [z, y, x] or flat"""
    nx, ny, nz = (int(v) for v in dims)
    shape = (nz, ny, nx)
    distance, d2, basis, site = (np.asarray(a).reshape(shape) for a in (distance, d2, basis, site))
    member = members_of(distance, d2, basis, min_basis, min_node_distance)
    place_of, places = labels_flood(member, origin, compression, floor)
    lin = lambda c: c[0] + nx * (c[1] + ny * c[2])
    # the edges: every unordered adjacent pair once
    pairs = {}
    for c, p in place_of.items():
        for dx, dy, dz in FORWARD:
            q = (c[0] + dx, c[1] + dy, c[2] + dz)
            pq = place_of.get(q)
            if pq is None or pq == p:
                continue
            key = (min(p, pq), max(p, pq))
            v = min(int(d2[c[2], c[1], c[0]]), int(d2[q[2], q[1], q[0]]))
            e = pairs.setdefault(key, [v, 0])
            e[0], e[1] = max(e[0], v), e[1] + 1
    # the components: a flood fill over the places
    adj = [[] for _ in places]
    for a, b in pairs:
        adj[a].append(b)
        adj[b].append(a)
    comp_of, comps = [-1] * len(places), []
    for p in range(len(places)):
        if comp_of[p] >= 0:
            continue
        comp_of[p] = len(comps)
        found, queue = [p], deque([p])
        while queue:
            for q in adj[queue.popleft()]:
                if comp_of[q] < 0:
                    comp_of[q] = len(comps)
                    found.append(q)
                    queue.append(q)
        comps.append(found)
    need = max(int(min_component_size), 1)
    kept_comp = [len(c) >= need for c in comps]
    comp_new, k = [], 0
    for keep in kept_comp:    # (a component's least place is its first: the order of the least places)
        comp_new.append(k if keep else -1)
        k += keep
    place_new, k = [], 0
    for p in range(len(places)):
        keep = kept_comp[comp_of[p]]
        place_new.append(k if keep else -1)
        k += keep
    n_places = k
    edges = sorted((place_new[a], place_new[b], v, n) for (a, b), (v, n) in pairs.items() if place_new[a] >= 0)
    out = {"place": np.full(shape, -1, np.int32), "centre": np.zeros((n_places, 3), np.int32), "centre_d2": np.zeros(n_places, np.int32),
           "radius": np.zeros(n_places, f32), "basis": np.zeros(n_places, np.uint8), "site": np.zeros((n_places, 3), np.int32),
           "n_cells": np.zeros(n_places, np.uint32), "sum": np.zeros((n_places, 3), np.int64), "degree": np.zeros(n_places, np.uint32),
           "component": np.zeros(n_places, np.uint32)}
    o = [int(v) for v in origin]
    for p, found in enumerate(places):
        q = place_new[p]
        if q < 0:
            continue
        for c in found:
            out["place"][c[2], c[1], c[0]] = q
        centre = min(found, key=lambda c: (-int(d2[c[2], c[1], c[0]]), lin(c)))
        at = (centre[2], centre[1], centre[0])
        out["centre"][q] = [o[a] + centre[a] for a in range(3)]
        out["centre_d2"][q] = d2[at]
        out["radius"][q] = distance[at]
        out["basis"][q] = basis[at]
        s = int(site[at])
        if 0 <= s < nx * ny * nz:
            out["site"][q] = [o[0] + s % nx, o[1] + (s // nx) % ny, o[2] + s // (nx * ny)]
        out["n_cells"][q] = len(found)
        out["sum"][q] = [sum(o[a] + c[a] for c in found) for a in range(3)]
        out["component"][q] = comp_new[comp_of[p]]
    out["edge_a"] = np.array([e[0] for e in edges], np.uint32)
    out["edge_b"] = np.array([e[1] for e in edges], np.uint32)
    out["edge_clearance_d2"] = np.array([e[2] for e in edges], np.int32)
    out["edge_n_contacts"] = np.array([e[3] for e in edges], np.uint32)
    for a, b, _, _ in edges:
        out["degree"][a] += 1
        out["degree"][b] += 1
    out["stats"] = {"n_members": len(place_of), "n_places_all": len(places), "n_edges_all": len(pairs), "n_components_all": len(comps),
                    "n_places": n_places, "n_edges": len(edges), "n_components": int(sum(kept_comp))}
    return out


def of_voronoi(field, origin, **kw):
    """places_graph over the dict voronoi_replica.field_of / FusionContext.voronoi_field returns"""
    nz, ny, nx = field["basis"].shape
    return places_graph(origin, (nx, ny, nz), field["distance"], field["d2"], field["basis"], field["site"], **kw)
