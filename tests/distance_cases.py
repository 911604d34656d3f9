"""Hand-built maps for khr_distance_field (tests/test_cpu_distance_field.py, tests/test_gpu_distance_field.py), in the style of
tests/mesh_cases.py whose Group / to_map they reuse: seeded, pure numpy, (indices, layers) as khronos_amd.checkpoint.pack takes
them -- FusionContext.load_map(pack(...)) on the device side, OracleMap.put_blocks(indices, layers) on the oracle side.

  wall    a 3 x 3 x 2 group of blocks at a negative origin.  Along x (group voxel column g): observed free space (positive
          distances) for g < S, an obstacle slab (negative distances) for S <= g < S + T, nothing observed (weight 0) behind it.
          S = vps + 3 is no multiple of 2 or 4: the slab's first column shares a ratio-2 and a ratio-4 cell with free columns.
  random  a 3 x 2 x 2 group at mesh_cases.ORIGIN, every voxel's sign independent and uniform, about 20 % of the voxels with
          weight 0, two blocks absent.
"""
import numpy as np

import mesh_cases as mc
import query_cases as qc

f32 = np.float32

WALL_ORIGIN = (-2, -1, -1)       # blocks
WALL_DIMS = (3, 3, 2)
WALL_THICKNESS = 5               # voxel columns
RANDOM_DIMS = (3, 2, 2)
RANDOM_ABSENT = [(1, 0, 1), (2, 1, 0)]
BOX_DIMS = (37, 21, 45)          # the GPU tests' box: no multiple of anything, longer than the groups along z
BOX_OFFSET = (-3, 2, -5)         # cells, from the group's first cell


def wall_start(vps):
    return vps + 3


def wall(vps, seed=21, with_group=False):
    g = mc.Group(np.random.default_rng(seed), vps, WALL_ORIGIN, dims=WALL_DIMS, signs=1.0)
    s = wall_start(vps)
    g.d[s:s + WALL_THICKNESS] = -g.d[s:s + WALL_THICKNESS]
    g.w[s + WALL_THICKNESS:] = 0.0
    out = mc.to_map([g])
    return out + (g,) if with_group else out


def random(vps, seed=23, with_group=False):
    rng = np.random.default_rng(seed)
    present = [p for p in np.ndindex(*RANDOM_DIMS) if p not in RANDOM_ABSENT]
    g = mc.Group(rng, vps, mc.ORIGIN, dims=RANDOM_DIMS, present=present)
    g.w[rng.random(g.w.shape) < 0.2] = 0.0
    out = mc.to_map([g])
    return out + (g,) if with_group else out


CASES = {"wall": wall, "random": random}


def group_first_cell(group_origin, vps, ratio):
    """the cell that holds the group's first voxel"""
    return tuple((int(o) * vps) // ratio for o in group_origin)


def box_of(name, vps, ratio):
    """(origin, dims) of the GPU tests' box: not block-aligned, negative on x and z, reaching past the blocks"""
    first = group_first_cell(WALL_ORIGIN if name == "wall" else mc.ORIGIN, vps, ratio)
    return tuple(f + o for f, o in zip(first, BOX_OFFSET)), BOX_DIMS


# the stream box of tests/test_cpu_distance_field.py and tests/test_gpu_distance_field.py: cells of 2 voxels around the last camera position
STREAM_RATIO, STREAM_DIMS, STREAM_MAX_DISTANCE = 2, (40, 40, 24), 1.2


def stream_box(pose, voxel_size, ratio=STREAM_RATIO, dims=STREAM_DIMS):
    """the box of `dims` cells centred on the cell that holds the pose's translation"""
    cell = float(f32(voxel_size) * f32(ratio))
    t = np.asarray(pose, np.float64).reshape(4, 4)[:3, 3]
    return tuple(int(np.floor(t[a] / cell)) - dims[a] // 2 for a in range(3)), dims


def surface_cells(frame, sensor, dyn, cell_size, origin, dims):
    """the cells (x, y, z relative to the box) that hold the back-projected surface points of the frame's non-dynamic pixels, those
    inside the box"""
    (at, _, _), sel = qc.surface_points(frame, sensor, 0.0)
    at = at[np.asarray(dyn).ravel()[sel] == 0]
    c = np.floor(at / f32(cell_size)).astype(np.int64) - np.asarray(origin, np.int64)
    return c[((c >= 0) & (c < np.asarray(dims))).all(axis=1)]
