"""Hand-picked life cycles of the object mini-map (tests/test_cpu_object_map_cases.py, tests/test_gpu_object_map_cases.py): the one
8^3 context MeshObjectExtractor keeps alive and sends every object through -- khr_reset_map at the object's voxel size,
khr_allocate_blocks, khr_integrate_shared_batch (k_multi_cull, k_multi_order, k_fuse_obj or k_fuse2<8, 4, ..>), khr_object_prune,
khr_generate_mesh.  Helper module, no tests.

A case is a list of frames and a list of objects.  A frame is a pose of SyntheticStream's scene (room 8 x 6 x 3 m; the mover sphere is
placed per frame, parked under the floor unless the frame says otherwise), optionally a range window of its own and a part of its
depth image made invalid.  An object is a voxel size and a list of steps on the context; only the LAST object of a case is compared:
  ("alloc", indices)            khr_allocate_blocks
  ("frame_alloc", k)            an allocating khr_integrate_shared of frame k
  ("frame_alloc_ckpt", k)       the same in a context of its own, saved and loaded into the (empty) batch context
  ("batch", [k, ...])           the batch context: one khr_integrate_shared_batch; its twin: one khr_integrate_shared per frame
  ("prune_mesh",)               khr_object_prune, khr_generate_mesh and a download (earlier objects only; the last object always gets it)
`run_three` (device) runs context A through every object of the case, context B -- fresh, frame by frame -- and a fresh OracleMap
through the last object only, and compares the three; `run_oracle` is the oracle's third alone with its per-frame statistics, on which
the CPU test shows that every case is what it claims to be.

Groups: R -- reuse through khr_reset_map, the voxel size changed across every reset so that the same integer block indices denote other
places; M -- blocks of an allocating integration or of a loaded checkpoint beside explicitly allocated ones (the item list of
k_multi_order has to hold them all); C -- one branch of k_multi_cull per case, the special frame(s) between ordinary ones; B -- the
row form of the band update (fuseBandRows) inside the multi-frame kernel."""
import math

import numpy as np

import common
from general_camera import GENERAL_INTRINSICS, general_stream, pose_rpy
from khronos_amd import FusionContext, default_config
from khronos_amd.synth import SyntheticStream
from oracle import pyoracle as po

OBJECT_MAP = dict(with_tracking=0, semantic_mode=1, num_labels=2)  # the extractor's configuration: the batch takes k_fuse_obj
LABEL_MAP = dict(with_tracking=1, semantic_mode=0, num_labels=4)   # any other 8^3 map: the batch takes k_fuse2<8, 4, ..>
LABEL_MAP_20 = dict(LABEL_MAP, num_labels=20)                      # the benchmark's label count: padded likelihood rows
LAYOUTS = {"object": OBJECT_MAP, "label": LABEL_MAP, "label20": LABEL_MAP_20}
OBJECT_ID = 3                       # the value the object image carries where the frame's label is the case's target
WALL, CEILING, MOVER = 3, 5, 19     # labels of the scene: the plane y = 3 m, the plane z = 3 m, the mover sphere
PARKED = ((0.0, 0.0, -10.0), 0.3)   # the mover under the floor: no ray reaches it
VPS = 8
FINE, COARSE = (0.03, 0.06), (0.04, 0.08)   # (voxel size, truncation distance) on the two sides of a reset
LAYERS = ("distance", "weight", "color", "flags", "sem_label", "likelihoods", "last_observed", "last_occupied")
K_MULTI_CHUNK, ORDER_WG = 7, 1024   # frames per launch of the multi-frame update; items per workgroup of k_multi_order


def box(xr, yr, zr):
    return np.array([[x, y, z] for x in range(xr[0], xr[1] + 1) for y in range(yr[0], yr[1] + 1) for z in range(zr[0], zr[1] + 1)], np.int32)


# the surface point the wall boxes sit on: (1.5, 3.0, 1.5), seen from around (1.3, 0.2, 1.4) looking along +y
WALL_BOX = box((3, 5), (8, 10), (3, 5))          # 27 blocks of 32 cm
WALL_BOX_FINE = box((5, 7), (11, 13), (5, 7))    # 27 blocks of 24 cm around the same point
BIG_BOX = box((-2, 9), (8, 10), (0, 8))          # 324 blocks of 32 cm of the same wall
# a mover of radius 0.3 m at (1.56, 2.28, 1.2) in blocks of 24 cm: every index lies inside BIG_BOX's index range
MOVER_NEAR_WALL = ((1.56, 2.28, 1.2), 0.3)
MOVER_BOX_FINE = box((5, 7), (8, 10), (3, 6))    # 36 blocks
# a mover at (1.44, 0.16, 1.44) in blocks of 32 cm, seen from 1.5 m in front of it (y = -1.34): without it the box is free space
# in front of the wall
MOVER_FREE = ((1.44, 0.16, 1.44), 0.3)
MOVER_BOX = box((3, 5), (-1, 1), (3, 5))
# the ceiling above (1.44, 0.16): one layer of blocks that contains z = 3 m
SLAB = box((2, 6), (-2, 2), (9, 9))


def look(pos, yaw, pitch=0.0, roll=0.0):
    return pose_rpy(pos, yaw, pitch, roll)


def ordinary(k, n=8):
    """poses that see the wall boxes whole: around (1.3, 0.2, 1.4), yaw within a few degrees of +y"""
    t = k / max(1, n - 1)
    return look((1.1 + 0.5 * t, 0.25 - 0.15 * t, 1.35 + 0.2 * t), math.pi / 2 + 0.12 * (t - 0.5))


def fr(pose, target=WALL, mover=PARKED, ranges=None, invalid=None):
    """a frame: ranges = (min_range, max_range) of its sensor, invalid = "all" | "half": the depth under the footprint of the case's
    `footprint_box` (and a margin of 4 pixels) set to 0 in even and NaN in odd rows, over all of it or over its left half"""
    return dict(pose=pose, target=target, mover=mover, ranges=ranges or (0.1, 5.0), invalid=invalid)


def intrinsics(case):
    W, H = case["size"]
    return GENERAL_INTRINSICS(W, H) if case.get("general") else (W / 2.0, W / 2.0, W / 2.0, H / 2.0)


def project(case, pose, pts):
    """pixel coordinates (float64) and camera z of world points"""
    fx, fy, cx, cy = intrinsics(case)
    T = np.linalg.inv(np.asarray(pose, np.float64))
    pc = np.asarray(pts, np.float64) @ T[:3, :3].T + T[:3, 3]
    return np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], axis=1), pc[:, 2]


def box_corners(indices, block_size):
    lo, hi = indices.min(0) * block_size, (indices.max(0) + 1) * block_size
    return np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], np.float64)


def footprint(case, pose, indices, block_size, margin=4):
    """(u0, v0, u1, v1), inclusive, clipped to the image: the pixel box around the projected corners of the block box"""
    W, H = case["size"]
    uv, z = project(case, pose, box_corners(indices, block_size))
    assert (z > 0).all()
    return (max(0, int(math.floor(uv[:, 0].min())) - margin), max(0, int(math.floor(uv[:, 1].min())) - margin),
            min(W - 1, int(math.ceil(uv[:, 0].max())) + margin), min(H - 1, int(math.ceil(uv[:, 1].max())) + margin))


def aim(case, pos, target, u, v, yaw0=math.pi / 2):
    """the (yaw, pitch) at which the camera at `pos` sees the world point `target` at pixel (u, v): Newton on the two angles"""
    a = np.array([yaw0, 0.0])
    f = lambda q: project(case, look(pos, q[0], q[1]), [target])[0][0] - (u, v)
    for _ in range(12):
        e, J = f(a), np.zeros((2, 2))
        for j in range(2):
            d = np.zeros(2)
            d[j] = 1e-6
            J[:, j] = (f(a + d) - e) / 1e-6
        a = a - np.linalg.solve(J, e)
    assert np.abs(f(a)).max() < 1e-3
    return float(a[0]), float(a[1])


def tiles_under(case, pose, block, block_size, item_z):
    """k_multi_cull's tile count of the wave item (the 8 x 8 voxels of one z layer, voxel centres) `item_z` of `block`: tiles of
    16 x 16 pixels under its projected corners, widened by 2 / 3 pixels as the kernel does and clipped to the image"""
    W, H = case["size"]
    vs = block_size / VPS
    lo = np.asarray(block, np.float64) * block_size + (0.5 * vs, 0.5 * vs, (item_z + 0.5) * vs)
    pts = np.array([lo + ((k & 1) * (block_size - vs), (k >> 1) * (block_size - vs), 0.0) for k in range(4)])
    uv, z = project(case, pose, pts)
    assert z.min() > 0.05
    tw, th = (W + 15) // 16, (H + 15) // 16
    tx0, ty0 = max(0, (int(math.floor(uv[:, 0].min())) - 2) // 16), max(0, (int(math.floor(uv[:, 1].min())) - 2) // 16)
    tx1, ty1 = min(tw - 1, (int(math.ceil(uv[:, 0].max())) + 3) // 16), min(th - 1, (int(math.ceil(uv[:, 1].max())) + 3) // 16)
    return (tx1 - tx0 + 1) * (ty1 - ty0 + 1)


def padded_row(cfg):
    """floats per likelihood row of the device's pool (khr_device.h: likStride, khr_config.packed_likelihood_rows)"""
    K = int(cfg.num_labels)
    return K if (cfg.packed_likelihood_rows or K <= 4) else (K + 31) & ~31


def band_rows_ok(cfg, frame_has_label=True, frame_has_color=True):
    """khr_kernels_fuse.h: fuseBandRowsOk, from the configuration of a mini context and what its frames carry"""
    KS = padded_row(cfg)
    do_sem = bool(cfg.with_semantics) and cfg.semantic_mode != 1 and frame_has_label
    return bool(do_sem and frame_has_color and cfg.semantic_mode != 1 and KS % 32 == 0 and KS <= 256)


def band_mode(cfg):
    """khronos_amd.hip: fillFuseMap -- rows (1) above 640 x 480 pixels of frame capacity where the lanes of a row divide a wave
    (fuseBandRowLanesOk), records (0) otherwise"""
    return 0 if cfg.max_frame_pixels <= 640 * 480 or padded_row(cfg) not in (32, 64, 128, 256) else 1


# ------------------------------------------------------------------------------------------------------------------------- cases
def _case(name, frames, objects, size=(160, 120), layout="object", general=False, mini=None, untouched=(), partial=(), ordinary_frame=0,
          footprint_box=None):
    """untouched / partial: frames of the last object's batch whose n_updated_voxels is 0 / strictly between 0 and that of
    `ordinary_frame`; every other frame of the last object updates at least one voxel"""
    return dict(name=name, frames=frames, objects=objects, size=size, layout=layout, general=general, untouched=tuple(untouched),
                partial=tuple(partial), ordinary_frame=ordinary_frame, footprint_box=footprint_box,
                mini=dict(dict(max_blocks=512, max_frame_pixels=size[0] * size[1]), **(mini or {})))


def _obj(steps, scale=COARSE):
    return dict(scale=scale, steps=steps)


def _simple(indices, ks, scale=COARSE):
    return _obj([("alloc", indices), ("batch", list(ks))], scale)


def _c_case(name, frames, untouched=(), partial=(), indices=WALL_BOX, **kw):
    kw.setdefault("footprint_box", (indices, COARSE[0] * VPS))
    return _case(name, frames, [_simple(indices, range(len(frames)))], untouched=untouched, partial=partial, **kw)


def _cull_cases():
    o = [ordinary(k, 4) for k in range(4)]
    pos, yaw = (1.3, 0.2, 1.4), math.pi / 2
    c = {}
    c["C1"] = _c_case("C1", [fr(o[0]), fr(look(pos, -yaw)), fr(o[1]), fr(o[2])], untouched=[1])
    c["C2"] = _c_case("C2", [fr(o[0]), fr(o[1], ranges=(0.1, 2.0)), fr(o[2])], untouched=[1])
    c["C2b"] = _c_case("C2b", [fr(o[0]), fr(o[1], ranges=(4.0, 5.0)), fr(o[2])], untouched=[1])
    c["C3"] = _c_case("C3", [fr(o[0]), fr(look((1.44, 2.8, 1.44), yaw)), fr(o[1])])
    c["C4"] = _c_case("C4", [fr(o[0]), fr(look(pos, yaw + 1.2)), fr(look(pos, yaw - 1.2)), fr(look(pos, yaw, 1.0)), fr(look(pos, yaw, -1.0)),
                             fr(o[1])], untouched=[1, 2, 3, 4])
    c["C4b"] = _c_case("C4b", [fr(o[0]), fr(look(pos, yaw + 0.75)), fr(look(pos, yaw - 0.75)), fr(look(pos, yaw, 0.62)),
                               fr(look(pos, yaw, -0.62)), fr(o[1])], partial=[1, 2, 3, 4])
    g = [look((1.2 + 0.1 * k, 0.2, 1.45), yaw + 0.1, (0.19, -0.19, 0.12)[k], (0.28, -0.09, 0.2)[k]) for k in range(3)]
    c["C5"] = _c_case("C5", [fr(g[0]), fr(g[1]), fr(look((1.3, 0.2, 1.45), yaw + 0.6, 0.1, 0.25)), fr(g[2])], partial=[2], general=True)
    screen = ((1.3, 1.05, 1.4), 0.45)   # the mover between the camera and the box: every voxel of the box far behind its surface
    c["C6"] = _c_case("C6", [fr(o[0]), fr(look(pos, yaw), mover=screen), fr(o[1]), fr(o[2])], untouched=[1])
    m = [look((1.29 + 0.1 * k, -1.34, 1.34 + 0.05 * k), yaw + 0.05 * (k - 1)) for k in range(4)]
    c["C6b"] = _c_case("C6b", [fr(m[0], MOVER, MOVER_FREE), fr(m[1], MOVER), fr(m[2], MOVER, MOVER_FREE), fr(m[3], MOVER, MOVER_FREE)],
                       indices=MOVER_BOX)
    c["C7"] = _c_case("C7", [fr(o[0]), fr(o[1], invalid="all"), fr(o[2])], untouched=[1])
    c["C7b"] = _c_case("C7b", [fr(o[0]), fr(o[1]), fr(o[1], invalid="half"), fr(o[2])], partial=[2], ordinary_frame=1)
    up = math.pi / 2
    below = [fr(look((1.3 + 0.1 * k, 0.1 + 0.05 * k, 1.9), yaw + 0.2 * k, 1.4 + 0.05 * k), CEILING) for k in range(3)]
    c["C8"] = _c_case("C8", [below[0], fr(look((1.44, 0.16, 2.63), yaw, up), CEILING), below[1], below[2]], indices=SLAB, size=(320, 240))
    c9 = dict(size=(161, 119))
    ya, pa = aim(c9, pos, (1.44, 3.0, 1.44), 156.0, 113.0)
    c["C9"] = _c_case("C9", [fr(o[0]), fr(look(pos, ya, pa)), fr(o[1])], partial=[1], size=(161, 119))
    return c


def _reuse_cases():
    n40 = [fr(ordinary(k, 40)) for k in range(40)]
    c = {}
    # R1: 324 blocks and 9 frames (two launches), then 36 blocks whose indices all lie inside the first box's index range
    f = [fr(ordinary(k, 9)) for k in range(9)] + [fr(ordinary(k, 3), MOVER, MOVER_NEAR_WALL) for k in range(3)]
    c["R1"] = _case("R1", f, [_simple(BIG_BOX, range(9)), _simple(MOVER_BOX_FINE, [9, 10, 11], FINE)])
    # R2 / R3: one word of frame bits per item, then two (the buffer is regrown, the item list kept), and the other way round
    c["R2"] = _case("R2", n40, [_simple(WALL_BOX, [0, 20, 39]), _simple(WALL_BOX_FINE, range(40), FINE)])
    c["R3"] = _case("R3", n40, [_simple(WALL_BOX, range(40)), _simple(WALL_BOX_FINE, [3, 11, 19, 27, 35], FINE)])
    f = [fr(ordinary(k, 5)) for k in range(5)]
    # R4: a batch of one frame (declined by the multi-frame path: frame by frame) and a batch of none, before the reset
    c["R4"] = _case("R4", f, [_obj([("alloc", WALL_BOX), ("batch", [0]), ("batch", [])]), _simple(WALL_BOX_FINE, [1, 2, 3, 4], FINE)])
    f = [fr(ordinary(k, 8)) for k in range(8)]
    c["R5"] = _case("R5", f, [_simple(WALL_BOX, range(8)), _simple(WALL_BOX_FINE, [1, 3, 4, 6, 7], FINE)], layout="label")
    c["R6"] = _case("R6", f, [_obj([("alloc", WALL_BOX), ("batch", [0, 1, 2, 3]), ("prune_mesh",)]), _simple(WALL_BOX_FINE, [4, 5, 6, 7], FINE)])
    return c


M_SCALE = (0.05, 0.1)                       # blocks of 40 cm
M_PRESENT = [(3, 7, 3), (4, 7, 3)]          # blocks around (1.5, 3.0, 1.5): allocated by the allocating frame
M_OUTSIDE = [(3, -9, 3), (4, -9, 3), (3, -9, 4), (4, -9, 4)]   # behind every camera of the case
M_E = np.array(M_OUTSIDE[:2] + M_PRESENT + M_OUTSIDE[2:], np.int32)
M_E200 = box((-5, 4), (7, 8), (0, 9))       # 200 blocks of the wall


def _mixed_cases():
    f = [fr(ordinary(k, 9)) for k in range(9)]
    mini = dict(max_blocks=8192)
    batch = ("batch", list(range(1, 9)))
    c = {}
    c["M1"] = _case("M1", f, [_obj([("frame_alloc", 0), ("alloc", M_E), batch], M_SCALE)], mini=mini)
    c["M2"] = _case("M2", f, [_obj([("frame_alloc_ckpt", 0), ("alloc", M_E), batch], M_SCALE)], mini=mini)
    c["M3"] = _case("M3", f, [_obj([("alloc", M_E200), ("frame_alloc", 0), batch], M_SCALE)], mini=mini)
    return c


def explicit_count(case):
    """E of the last object: the blocks khr_allocate_blocks was given (the host counts them whether present or not)"""
    return sum(len(s[1]) for s in case["objects"][-1]["steps"] if s[0] == "alloc")


def order_reach(case):
    """slots the grid of k_multi_order covers with one thread per item: 128 * ceil(8 E / 1024)"""
    return (ORDER_WG // VPS) * -(-VPS * explicit_count(case) // ORDER_WG)


def _band_cases():
    f = [fr(ordinary(k, 15)) for k in range(15)]
    obj = [_simple(BIG_BOX, range(15))]
    return {"B_rows": _case("B_rows", f, obj, size=(320, 240), layout="label20", mini=dict(max_frame_pixels=641 * 480)),
            "B_records": _case("B_records", f, obj, size=(320, 240), layout="label20")}


CASES = {}
CASES.update(_reuse_cases())
CASES.update(_mixed_cases())
CASES.update(_cull_cases())
CASES.update(_band_cases())
R_CASES, M_CASES = ["R1", "R2", "R3", "R4", "R5", "R6"], ["M1", "M2", "M3"]
C_CASES = ["C1", "C2", "C2b", "C3", "C4", "C4b", "C5", "C6", "C6b", "C7", "C7b", "C8", "C9"]
C_AGAIN = ["C3", "C5", "C9"]    # once more in relaxed arithmetic and with LABEL_MAP


def variant(name, layout=None):
    case = CASES[name]
    return case if layout is None else dict(case, layout=layout)


def mini_config(case, scale, exact=1):
    return default_config(voxels_per_side=VPS, voxel_size=scale[0], truncation_distance=scale[1], with_semantics=1, exact_arithmetic=exact,
                          **dict(LAYOUTS[case["layout"]], **case["mini"]))


def uses_object_image(case):
    return LAYOUTS[case["layout"]]["semantic_mode"] == 1


# ------------------------------------------------------------------------------------------------------------------------ frames
_rendered = {}


def render(case):
    """the frames of a case: stamp, pose, depth, rgb, label, obj (the object image) and ranges; rendered once per case and size"""
    key = (case["name"], case["size"])
    if key in _rendered:
        return _rendered[key]
    W, H = case["size"]
    s = general_stream(W, H) if case["general"] else SyntheticStream(W, H)
    assert (s.fx, s.fy, s.cx, s.cy) == intrinsics(case)
    out = []
    for k, f in enumerate(case["frames"]):
        s.set_mover(f["mover"][0], (0.0, 0.0, 0.0), f["mover"][1])
        r = s.render(k, pose=f["pose"])
        if f["invalid"]:
            u0, v0, u1, v1 = footprint(case, f["pose"], *case["footprint_box"])
            if f["invalid"] == "half":
                u1 = (u0 + u1) // 2
            r["depth"][v0:v1 + 1:2, u0:u1 + 1] = 0.0
            r["depth"][v0 + 1:v1 + 1:2, u0:u1 + 1] = np.nan
        r["obj"] = (r["label"] == f["target"]).astype(np.int32) * OBJECT_ID
        r["ranges"] = f["ranges"]
        out.append(r)
    _rendered[key] = out
    return out


# ------------------------------------------------------------------------------------------------------------------------ oracle
def run_oracle(case, exact=1, keep=False, finish=True):
    """the last object of a case on a fresh OracleMap.  Returns dict(ora, per_frame: [(step, frame, statistics of integrate)],
    updated: number of blocks whose weight a ("batch", ..) step changed, and -- with finish -- mesh, pruned (the prune count), mesh_pruned);
    ora is closed unless keep"""
    frames, obj = render(case), case["objects"][-1]
    cfg = mini_config(case, obj["scale"], exact)
    ora = po.OracleMap(po.config_from(cfg, 0))
    W, H = case["size"]
    with_obj = uses_object_image(case)

    def integrate(k, allocate):
        f = frames[k]
        sen = ora.make_sensor(W, H, *intrinsics(case), *f["ranges"])
        if with_obj:
            return ora.integrate(sen, f["stamp"], f["pose"], f["depth"], f["rgb"], None, object_image=f["obj"], object_id=OBJECT_ID,
                                 allocate_blocks=allocate)
        return ora.integrate(sen, f["stamp"], f["pose"], f["depth"], f["rgb"], f["label"], allocate_blocks=allocate)
    weights = lambda: {tuple(b): ora.get_block(b, likelihoods=False)["weight"] for b in ora.block_indices().tolist()}
    out = dict(per_frame=[], updated=0, after_alloc_frame=None)
    for si, step in enumerate(obj["steps"]):
        if step[0] == "alloc":
            ora.allocate_blocks(step[1])
        elif step[0] in ("frame_alloc", "frame_alloc_ckpt"):
            out["per_frame"].append((si, step[1], integrate(step[1], True)))
            out["after_alloc_frame"] = {tuple(b) for b in ora.block_indices().tolist()}
        elif step[0] == "batch":
            before = weights()
            for k in step[1]:
                out["per_frame"].append((si, k, integrate(k, False)))
            after = weights()
            out["updated"] += sum(1 for b in after if not np.array_equal(after[b], before[b]))
    out["ora"] = ora
    if finish:
        ora.generate_mesh(True, False)
        out["mesh"] = ora.mesh()
        out["pruned"] = ora.object_prune(0.5, 2.0) if with_obj else None
        ora.generate_mesh(True, False)
        out["mesh_pruned"] = ora.mesh()
    if not keep:
        out["n_blocks"] = ora.num_blocks()
        ora.close()
        out["ora"] = None
    return out


# ------------------------------------------------------------------------------------------------------------------------ device
def _window(case):
    """a window context that only holds the frames of the case in retained slots, and the slots"""
    W, H = case["size"]
    frames = render(case)
    n_slots = len(frames) + 2
    win = FusionContext(default_config(voxel_size=0.1, truncation_distance=0.3, with_semantics=1, with_tracking=1, max_blocks=64,
                                       max_frame_pixels=W * H, num_frame_slots=n_slots, exact_arithmetic=1))
    slots = []
    for f in frames:
        sen = win.make_sensor(W, H, *intrinsics(case), *f["ranges"])
        slot = win.upload_frame(sen, f["stamp"], f["pose"], f["depth"], f["rgb"], f["label"])
        win._chk(win.lib.khr_retain_slot(win.h, slot))
        win.set_frame_image(slot, 1, f["obj"])
        slots.append(slot)
    assert len(set(slots)) == len(frames)
    win.sync()
    return win, slots


def _layers(ctx):
    order = ctx.block_indices()
    order = order[np.lexsort(order.T)]
    bl = [ctx.download_block(idx) for idx in order]
    return order, {k: np.stack([b[k] for b in bl]) for k in LAYERS}


def _mesh(ctx):
    ctx.generate_mesh(True, False)
    return ctx.download_mesh()


def _device_object(ctx, case, obj, win, slots, batched, exact):
    """the steps of one object on a context whose map is empty at the object's scale; returns the mesh of a ("prune_mesh",) step"""
    with_obj = uses_object_image(case)
    oid = OBJECT_ID if with_obj else -1
    mesh = None
    for step in obj["steps"]:
        if step[0] == "alloc":
            ctx.allocate_blocks(step[1])
        elif step[0] == "frame_alloc" or (step[0] == "frame_alloc_ckpt" and not batched):
            ctx.integrate_shared(win, slots[step[1]], allocate_blocks=True, object_id=oid)
        elif step[0] == "frame_alloc_ckpt":
            tmp = FusionContext(mini_config(case, obj["scale"], exact))
            try:
                tmp.integrate_shared(win, slots[step[1]], allocate_blocks=True, object_id=oid)
                assert ctx.load_map(tmp.save_map()) == tmp.num_blocks() > 0
            finally:
                tmp.close()
        elif step[0] == "batch" and batched:
            ks = step[1]
            ctx.integrate_shared_batch(win, [slots[k] for k in ks], [oid] * len(ks) if with_obj else None)
        elif step[0] == "batch":
            for k in step[1]:
                ctx.integrate_shared(win, slots[k], object_id=oid)
        elif step[0] == "prune_mesh":
            ctx.object_prune(0.5, 2.0)
            mesh = _mesh(ctx)
    return mesh


MESH_KEYS = ("points", "colors", "labels", "stamps")


def run_three(case, exact=1, max_oracle_blocks=None):
    """context A: every object of the case in turn, khr_reset_map between them, batches as batches.  Context B: fresh, the last
    object only, frame by frame.  A fresh OracleMap: the last object.  A == B bit for bit (digest, every layer of every block, block
    indices, statistics, prune count, meshes before and after the prune); A against the oracle by common.compare_maps (exact in exact
    arithmetic, TOL and its borderline bound in relaxed arithmetic) and, for the mesh points, common.TOL.  Returns A's digest."""
    win, slots = _window(case)
    objects = case["objects"]
    last = objects[-1]
    a = FusionContext(mini_config(case, objects[0]["scale"], exact))
    b = FusionContext(mini_config(case, last["scale"], exact))
    ref = run_oracle(case, exact, keep=True, finish=False)
    ora = ref["ora"]
    try:
        earlier = []
        for i, obj in enumerate(objects):
            if i:
                a.reset_map(*obj["scale"])
                assert a.num_blocks() == 0 and len(a.block_indices()) == 0
            m = _device_object(a, case, obj, win, slots, True, exact)
            if m is not None:
                earlier.append(m)
        _device_object(b, case, last, win, slots, False, exact)
        da, db = [int(x) for x in a.map_digest()], [int(x) for x in b.map_digest()]
        print(case["name"], "digests", "equal" if da == db else "DIFFER", "blocks", a.num_blocks(), b.num_blocks(), ora.num_blocks())
        assert da == db, ("batch and frame-by-frame digests differ", [n for n, x, y in zip(common.DIGEST_LAYERS, da, db) if x != y])
        ia, la = _layers(a)
        ib, lb = _layers(b)
        assert np.array_equal(ia, ib) and np.array_equal(a.block_indices(), b.block_indices())
        assert a.num_blocks() == b.num_blocks() == ora.num_blocks() == len(ia)
        for k in LAYERS:
            assert la[k].tobytes() == lb[k].tobytes(), k
        # the counters of everything the context itself integrated (the frame a checkpoint brought in was another context's)
        sa, sb = a.stats(), b.stats()
        own = [si for si, s in enumerate(last["steps"]) if s[0] != "frame_alloc_ckpt"]
        for ctx_stats, steps in ((sa, own), (sb, range(len(last["steps"])))):
            assert ctx_stats["pool_exhausted"] == 0
            for k in ("updated_voxels", "band_voxels"):
                want = sum(st["n_" + k] for si, _, st in ref["per_frame"] if si in steps)
                assert ctx_stats["cum_" + k] == want, (k, ctx_stats["cum_" + k], want)
        assert sa["cum_updated_voxels"] > 0
        common.compare_maps(a, ora, exact=bool(exact), max_blocks=max_oracle_blocks)
        with_obj = uses_object_image(case)
        for pruned in (False, True):
            if pruned and with_obj:
                pa, pb, po_ = a.object_prune(0.5, 2.0), b.object_prune(0.5, 2.0), ora.object_prune(0.5, 2.0)
                assert pa == pb == po_, (pa, pb, po_)
            ora.generate_mesh(True, False)
            ma, mb, mo = _mesh(a), _mesh(b), ora.mesh()
            for k in MESH_KEYS[:4 if LAYOUTS[case["layout"]]["with_tracking"] else 3]:   # (stamps where the layout has them)
                assert ma[k].tobytes() == mb[k].tobytes(), (k, pruned)
            assert ma["points"].shape == mo["points"].shape, (pruned, ma["points"].shape, mo["points"].shape)
            assert pruned or len(mo["points"]) > 0
            if len(mo["points"]):
                assert np.abs(ma["points"] - mo["points"]).max() <= common.TOL
            assert np.array_equal(ma["labels"], mo["labels"])
            if exact:
                assert ma["points"].tobytes() == mo["points"].tobytes() and ma["colors"].tobytes() == mo["colors"].tobytes()
            for m in earlier:   # no vertex of an earlier object's mesh survives the reset
                if len(m["points"]) and len(ma["points"]):
                    old = {p.tobytes() for p in m["points"]}
                    assert not any(p.tobytes() in old for p in ma["points"])
        if with_obj:
            common.compare_maps(a, ora, exact=bool(exact), max_blocks=max_oracle_blocks)
        return da
    finally:
        a.close()
        b.close()
        ora.close()
        win.close()
