"""Hand-built maps for khr_voronoi_field (tests/test_cpu_voronoi_replica.py, tests/test_gpu_voronoi_field.py).  distance_cases.wall
and distance_cases.random are used as they are; the cases here are one block of mesh_cases.Group style each -- everything observed
and free, the obstacle voxels negative -- with the box that goes with them:

  corridor(lo, hi)  two walls, the planes x = lo and x = hi of the box; free columns between and outside them
  posts()           four posts, single cells at the corners of an 8-cell square in the plane z = 3; the centre cell is
                    equidistant to all four

Each returns (indices, layers, origin, dims, in_set): the map as khronos_amd.checkpoint.pack takes it, the box in cells of one
voxel, and the obstacle set the construction means, bool [z, y, x]."""
import numpy as np

import distance_cases as dc
import mesh_cases as mc

VPS = 16
BLOCK = (-1, 2, -3)   # the block's index: the box is negative on x and z
BOX_FIRST = (1, 3, 2)  # the box's first voxel inside the block
CORRIDOR_EVEN, CORRIDOR_ODD = (2, 11), (2, 12)
POSTS = [(2, 2), (10, 2), (2, 10), (10, 10)]   # (x, y) in the box, z = 3
POSTS_DIMS, POSTS_CENTRE = (13, 13, 7), (6, 6, 3)
MIN_DISTANCE_CELLS = 2
# (mode, parent_l1_separation, parent_cos_angle_separation, max_distance) of the GPU tests; max_distance None = 5.5 cells
PARAMS = [(0, 4, 0.0, 100.0), (2, 20, 0.2, None), (1, 1, 0.2, 100.0)]


def _case(dims, obstacle_xyz, seed):
    g = mc.Group(np.random.default_rng(seed), VPS, BLOCK, dims=(1, 1, 1), signs=1.0)
    in_set = np.zeros((dims[2], dims[1], dims[0]), bool)
    for x, y, z in obstacle_xyz:
        in_set[z, y, x] = True
        g.d[BOX_FIRST[0] + x, BOX_FIRST[1] + y, BOX_FIRST[2] + z] *= -1.0
    indices, layers = mc.to_map([g])
    origin = tuple(b * VPS + f for b, f in zip(BLOCK, BOX_FIRST))
    assert all(f + d <= VPS for f, d in zip(BOX_FIRST, dims))
    return indices, layers, origin, dims, in_set


def corridor(walls, seed=31):
    lo, hi = walls
    dims = (hi + 3, 6, 6)
    return _case(dims, [(x, y, z) for x in (lo, hi) for y in range(dims[1]) for z in range(dims[2])], seed)


def posts(seed=37):
    return _case(POSTS_DIMS, [(x, y, 3) for x, y in POSTS], seed)


def params(cell):
    """PARAMS with the five-and-a-half-cell range filled in"""
    return [(m, l1, cs, 5.5 * float(cell) if md is None else md) for m, l1, cs, md in PARAMS]


# the stream box of tests/test_cpu_voronoi_replica.py and tests/test_gpu_voronoi_field.py: distance_cases.stream_box with
STREAM = dict(ratio=dc.STREAM_RATIO, max_distance=dc.STREAM_MAX_DISTANCE, mode=0, parent_l1_separation=4, unknown_is_obstacle=False)
