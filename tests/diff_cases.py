"""Hand-built map pairs for khr_diff_map (ASSUMPTIONS.md A.18), on merge_cases.rich_map / ragged_map: `now` and `then` as
(indices, layers) pairs in the form of khronos_amd.checkpoint, fixed seeds, at most a few tens of blocks.  The distances of the
`rich` pairs are drawn from a short list around the two thresholds (each threshold, the float next to it on either side, a value
in the gap, clear values on either side), the weights from merge_cases' list (min_weight and the float below it), so every class
of A.18 meets each side of each comparison many times per block.  Needs no device."""
import numpy as np

import merge_cases as mc
from khronos_amd import checkpoint as ck

f32 = np.float32
MIN_WEIGHT = mc.MIN_WEIGHT
OCC, FREE = f32(0.01), f32(0.04)  # (inside the band of both configurations)
INF = f32(np.inf)


def distances(occ, free):
    occ, free = f32(occ), f32(free)
    return np.array([occ, np.nextafter(occ, -INF), np.nextafter(occ, INF), free, np.nextafter(free, -INF), np.nextafter(free, INF),
                     (occ + free) / f32(2), -0.1, 0.1, -0.03, 0.07], f32)


def rich_pair_map(cfg, blocks, seed, occ, free):
    idx, L = mc.rich_map(cfg, blocks, seed)
    rng = np.random.default_rng(seed + 5000)
    L["distance"][:] = rng.choice(distances(occ, free), L["distance"].shape)
    return idx, L


def solid_map(cfg, blocks, seed, distance):
    """every voxel observed (weight 2.5) at one distance; the other layers rich"""
    idx, L = mc.rich_map(cfg, [(b, "solid") for b in blocks], seed)
    L["distance"][:] = f32(distance)
    return idx, L


def case(name, cfg, now, then, mode=0, voxel_offset=(0, 0, 0), pose=None, occ=OCC, free=FREE, min_weight=float(MIN_WEIGHT)):
    return dict(name=name, cfg=cfg, now=now, then=then, mode=mode, voxel_offset=voxel_offset, pose=pose, min_weight=min_weight,
                occupied_distance=None if occ is None else float(occ), free_distance=None if free is None else float(free))


def _rich(name, cfg, offset, now_blocks, then_blocks, seed, occ=OCC, free=FREE):
    o, f = (0.0, ck.config_fields(cfg)["voxel_size"]) if occ is None else (occ, free)
    return case(name, cfg, rich_pair_map(cfg, now_blocks, seed, o, f), rich_pair_map(cfg, then_blocks, seed + 1, o, f), voxel_offset=offset,
                occ=occ, free=free)


def _singles():
    """two blocks with one change each: linear index 0 of (0, 0, 0) appeared, the last linear index of (2, -1, 0) disappeared"""
    blocks = [(0, 0, 0), (2, -1, 0)]
    now, then = solid_map(mc.CFG16, blocks, 31, -0.1), solid_map(mc.CFG16, blocks, 32, -0.1)
    then[1]["distance"][0, 0] = f32(0.1)
    now[1]["distance"][1, 16 ** 3 - 1] = f32(0.1)
    return case("singles", mc.CFG16, now, then)


def _four_waves():
    """one block at 16^3 and one at 8^3 whose changes lie in groups of all four waves (group g belongs to wave g % 4)"""
    out = []
    for cfg, tag, lins in ((mc.CFG16, "16", [5, 64 + 7, 128 + 63, 192, 256 + 1, 16 ** 3 - 64 * 3 + 9, 16 ** 3 - 1]),
                           (mc.CFG8, "8", [0, 3, 64 + 63, 128 + 31, 192 + 1, 256, 320 + 5, 384 + 17, 511])):
        now, then = solid_map(cfg, [(1, 1, 1)], 41, 0.1), solid_map(cfg, [(1, 1, 1)], 42, 0.1)
        for i, l in enumerate(lins):  # alternately appeared and disappeared
            if i % 2 == 0:
                now[1]["distance"][0, l] = f32(-0.1)
            else:
                then[1]["distance"][0, l], now[1]["distance"][0, l] = f32(-0.1), f32(0.1)
        out.append(case("four_waves_vps" + tag, cfg, now, then))
    return out


def _resample():
    """`then` a ragged linear field, `now` another linear field over the same stretch: the classes flip across a plane"""
    then = mc.ragged_map(mc.CFG16, [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (-1, 0, 0)], 601)
    now = mc.ragged_map(mc.CFG16, [(0, 0, 0), (1, 0, 0), (0, 1, 0), (-4, 4, 4)], 701)
    vps, vs = 16, f32(0.1)
    lin = np.arange(vps ** 3)
    for i, b in enumerate(now[0]):
        c = [((int(b[a]) * vps + (lin // vps ** a) % vps).astype(f32) + f32(0.5)) * vs for a in range(3)]
        now[1]["distance"][i] = (f32(-0.06) * c[0] + f32(0.02) * c[1] + f32(0.05) * c[2] + f32(0.03)).astype(f32)
    return case("resample", mc.CFG16, now, then, mode=1, pose=mc.pose((1.0, 2.0, -0.5), 30.0, (0.137, -0.291, 0.053)), occ=-0.01, free=0.01)


R = "rich"
ORDER_BLOCKS = [(-1, 2, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (-2, -1, -1)]
_SAME = rich_pair_map(mc.CFG16, [((0, 0, 0), R), ((0, 1, 0), R), ((4, 0, -1), R)], 50, OCC, FREE)
CASES = [
    # block-set edges: (0, 0, 1) of `then` is a candidate `now` lacks, (3, 3, 3) of `now` is reached by nothing, (-5, 2, 2) of
    # `then` has zero weights (present, nothing compared), (0, 1, 0) of `now` has zero weights (only_then)
    _rich("zero_offset", mc.CFG16, (0, 0, 0), [((0, 0, 0), R), ((1, 0, 0), R), ((3, 3, 3), R), ((0, 1, 0), "zero"), ((-5, 2, 2), R)],
          [((0, 0, 0), R), ((1, 0, 0), R), ((0, 0, 1), R), ((0, 1, 0), R), ((-5, 2, 2), "zero")], 100),
    _rich("block_offset", mc.CFG16, (16, 0, -16), [((1, 0, -1), R), ((2, 0, 0), R), ((7, 7, 7), R)],
          [((0, 0, 0), R), ((1, 0, 0), R), ((1, 0, 1), R), ((9, 9, 9), "zero")], 200),
    _rich("odd_offset", mc.CFG16, (5, -3, 17), [((0, -1, 1), R), ((-1, -1, 0), R), ((0, 0, 1), R), ((1, 0, 2), R), ((0, -2, 1), "zero"), ((6, 6, 6), R)],
          [((-1, -1, -1), R), ((0, 0, 0), R), ((-2, 0, -1), R), ((4, -4, 4), "zero")], 300),
    _rich("vps8_zero_offset", mc.CFG8, (0, 0, 0), [((0, 0, 0), R), ((0, 0, -1), R), ((5, 5, 5), R)],
          [((0, 0, 0), R), ((0, 0, -1), R), ((-1, 0, 0), R), ((8, 8, 8), "zero")], 400),
    _rich("vps8_block_offset", mc.CFG8, (8, 0, -8), [((1, 0, -1), R), ((1, 0, 0), R), ((5, 5, 5), R)],
          [((0, 0, 0), R), ((0, 0, 1), R), ((-1, 0, 0), R)], 410),
    _rich("vps8_odd_offset", mc.CFG8, (5, -3, 17), [((0, 0, 2), R), ((0, -1, 2), R), ((1, 0, 2), R), ((1, -1, 3), R), ((0, 0, 3), R), ((-1, 0, 1), R), ((5, 5, 5), R)],
          [((-1, -1, -1), R), ((0, 0, 0), R), ((0, 0, 1), R), ((-1, 0, 0), R)], 420),
    # five changed blocks whose (x, y, z) order is neither the order of their packed keys (x in the low bits) nor the order given
    _rich("order", mc.CFG16, (0, 0, 0), [(b, R) for b in ORDER_BLOCKS], [(b, R) for b in ORDER_BLOCKS], 500),
    # changed-block counts 0 (a map against itself), 1 and 3; the default thresholds (0 and voxel_size) in the last
    case("no_change", mc.CFG16, _SAME, _SAME),
    _rich("one_block", mc.CFG16, (0, 0, 0), [((0, 0, 0), R), ((2, 2, 2), R)], [((0, 0, 0), R), ((-2, 2, 2), R)], 600),
    _rich("three_blocks_default_thresholds", mc.CFG16, (0, 0, 0), [((0, 0, 0), R), ((0, 0, 1), R), ((-1, 0, 0), R), ((2, 2, 2), R)],
          [((0, 0, 0), R), ((0, 0, 1), R), ((-1, 0, 0), R)], 700, occ=None, free=None),
    # every voxel of the block changed: the in-block prefix reaches its maximum
    case("all_changed", mc.CFG16, solid_map(mc.CFG16, [(0, -1, 0)], 21, -0.1), solid_map(mc.CFG16, [(0, -1, 0)], 22, 0.1)),
    case("all_changed_vps8", mc.CFG8, solid_map(mc.CFG8, [(0, -1, 0)], 23, 0.1), solid_map(mc.CFG8, [(0, -1, 0)], 24, -0.1)),
    _singles(),
    *_four_waves(),
    _resample(),
]
BY_NAME = {c["name"]: c for c in CASES}


def request_of(case):
    return dict(mode=case["mode"], voxel_offset=case["voxel_offset"], pose=case["pose"], min_weight=case["min_weight"],
                occupied_distance=0.0 if case["occupied_distance"] is None else case["occupied_distance"], free_distance=case["free_distance"])


def replica_of(case):
    import diff_replica as dr
    return dr.diff(ck.config_fields(case["cfg"]), case["now"][0], case["now"][1], case["then"][0], case["then"][1], **request_of(case))
