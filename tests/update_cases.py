"""Hand-built frames for the update kernels (tests/test_cpu_update_cases.py, tests/test_gpu_update_cases.py): k_fuse, k_fuse2 and
k_fuse_obj of khr_kernels_fuse.h and the arithmetic they share through khr_fuse_math.h.  Helper module, no tests, no device.

Geometry.  voxel_size 1/8 m, truncation distance 1/4 m, an unrotated camera (world_T_sensor = identity rotation, a translation) over
the voxel box [0, 16)^3: one block of 16^3 voxels or eight of 8^3.  The translation puts the voxel layer `L` at camera depth exactly
1 (layer_tz); with fx = fy = 8 the voxel (ix, iy, L) projects to the pixel (ix + ou, iy + ov), ou = 0.5 - 8 tx + cx, so integer or
half-integer cx, cy and translations in steps of 1/64 m place the voxel centres of that layer on integer, half or quarter pixels.
Every quantity of a NAMED voxel (camera-frame position, pixel, interpolation weights, surface range, signed distance) is dyadic and
therefore exact in float32: the voxel sits ON the edge it is named for, not near it.  The other voxels of the box -- other depths,
non-dyadic pixels -- are ordinary voxels that every implementation has to agree on as well.

A case is a dict: size (W, H), intr (fx, fy, cx, cy), ranges (min_range, max_range) of its sensor, region (voxel box), K
(num_labels), cfg (khr_config overrides the case needs: its switches), use_mask, frames (dicts laid out as SyntheticStream.render
returns them, plus `dyn`: the dynamic image, where the case paints one), checks: [(frame, (ix, iy, iz), {decision: value})] -- what
the case claims about its named voxels, shown on the numpy restatement of the decisions in the CPU test --, both: the decisions of
which the named voxels must show both outcomes.  One ulp: the neighbouring float32 of the SURFACE RANGE the case writes into the
depth image (up / dn); the signed distance is the exact difference of two floats, a few ulps of the bound away.  The cases
sdf_neighbours* put the signed distance on the float32 neighbours of -truncation itself.  Every case holds two frames or more: a
batch of one frame and a tick of one camera never reach the multi-frame kernels.

Groups: EDGE_CASES (one decision edge or more each), SWITCH_CASES (the same frames under every integrator switch, with the map
layers that must differ from the default run), LABEL_CASES (label counts, the in-band record counts per wave item that the band
phase's shapes depend on, ties of the arg-max), GENERIC (non-dyadic everything: the one case of the relaxed-arithmetic runs)."""
import numpy as np

from oracle import pyoracle as po

F32 = np.float32
VS, TRUNC = 0.125, 0.25
OBJECT_ID = 1
# layouts of a map (khr_config), as the batch entry point tells them apart: the extractor's binary object layer takes k_fuse_obj
OBJECT_LAYOUT = dict(with_tracking=0, semantic_mode=1, num_labels=2)
SWITCH_DEFAULTS = dict(use_constant_weight=0, use_weight_dropoff=1, weight_dropoff_epsilon=-1.0, interpolation_method=2, range_mode=0,
                       adaptive_max_range_difference=0.2, label_confidence=0.9, max_weight=1e5, color_blend_weight=0)
# the switches k_fuse2 and k_fuse_obj hard-code (multiApplies, tickUnion): any other value has to send a tick or a batch to k_fuse
# (the GPU test asks default_switches which runs are meant to reach the multi-frame kernels, and holds those to their entry conditions)
HARD_CODED = ("use_constant_weight", "use_weight_dropoff", "interpolation_method", "range_mode")


def up(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def dn(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def pose(tx, ty, tz):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T


def layer_tz(L, depth=1.0):
    """camera z at which the voxel layer L lies at camera depth `depth`"""
    return (L + 0.5) * VS - depth


def rgb_image(W, H, k=0):
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([(u * 37 + v * 11 + k * 53) % 256, (u * 5 + v * 71 + k * 19 + 128) % 256, (u * 13 + v * 29 + k * 7 + 64) % 256], axis=-1).astype(np.uint8)


def label_image(W, H, K, k=0):
    """the four pixels of every 2 x 2 neighbourhood carry different labels (K >= 4)"""
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    return (((u % 2) + 2 * (v % 2) + k) % K).astype(np.int32)


def frame(k, T, depth, rgb=None, label=None, dyn=None, K=4):
    H, W = depth.shape
    return dict(stamp=(k + 1) * 100_000_000, pose=np.asarray(T, np.float64), depth=np.ascontiguousarray(depth, np.float32),
                rgb=rgb_image(W, H, k) if rgb is None else np.ascontiguousarray(rgb, np.uint8),
                label=label_image(W, H, K, k) if label is None else np.ascontiguousarray(label, np.int32),
                dyn=None if dyn is None else np.ascontiguousarray(dyn, np.int32))


def plane(W, H, d):
    return np.full((H, W), d, np.float32)


def _case(name, size, intr, frames, checks=(), both=(), ranges=(0.125, 2.0), cfg=None, K=4, use_mask=False, region=((0, 0, 0), (16, 16, 16)),
          track=False, only_vps=None):
    return dict(name=name, size=size, intr=intr, ranges=ranges, region=region, K=K, cfg=dict(cfg or {}), use_mask=use_mask, frames=frames,
                checks=list(checks), both=tuple(both), track=track, only_vps=only_vps)


def blocks(case, vps):
    lo, hi = case["region"]
    return np.array([[x, y, z] for x in range(lo[0] // vps, (hi[0] - 1) // vps + 1) for y in range(lo[1] // vps, (hi[1] - 1) // vps + 1)
                     for z in range(lo[2] // vps, (hi[2] - 1) // vps + 1)], np.int32)


def vps_of(case):
    return [case["only_vps"]] if case["only_vps"] else [16, 8]


def config(case, vps, layout=None, **extra):
    """keyword arguments of default_config for a map of the case"""
    W, H = case["size"]
    kw = dict(voxel_size=VS, truncation_distance=TRUNC, voxels_per_side=vps, with_semantics=1, with_tracking=1, num_labels=case["K"], semantic_mode=0,
              max_blocks=64, max_frame_pixels=W * H, num_frame_slots=10, max_mesh_vertices=1 << 16, exact_arithmetic=1)
    kw.update(case["cfg"])
    kw.update(layout or {})
    kw.update(extra)
    return kw


def default_switches(kw):
    """would multiApplies / tickUnion let this configuration into k_fuse2 / k_fuse_obj?"""
    return all(kw.get(k, SWITCH_DEFAULTS[k]) == SWITCH_DEFAULTS[k] for k in HARD_CODED)


MIN_MULTI_FRAMES, MAX_MULTI_FRAMES = 2, 1024    # khronos_amd.hip: multiApplies declines a batch of one frame (and of more than kMaxMultiFrames)
TICK_CAMERAS = 3


def tick_chunks(case):
    """the frames of a case as the cameras of ticks: [(first frame, one past the last)], three cameras a tick and never one alone
    (4 frames: 2 + 2, 7 frames: 3 + 2 + 2)"""
    n = len(case["frames"])
    sizes = [TICK_CAMERAS] * (n // TICK_CAMERAS)
    if n % TICK_CAMERAS == 2 or not sizes:
        sizes.append(n % TICK_CAMERAS)
    elif n % TICK_CAMERAS == 1:
        sizes[-1:] = [2, 2]
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    return [(a, a + m) for a, m in zip(starts, sizes)]


def tick_stamps(case):
    """every camera of a tick carries the stamp of the tick's first frame"""
    return [case["frames"][a]["stamp"] for a, b in tick_chunks(case) for _ in range(a, b)]


# ---- the small image (14 x 12): a 16 x 16 voxel layer reaches one pixel beyond every border --------------------------------------
SMALL, SMALL_INTR = (14, 12), (8.0, 8.0, 6.5, 6.5)      # u = ix - 1, v = iy - 1 from tx = ty = 1
# ---- the ordinary image (32 x 24): the layer covers the window u in [8, 23], v in [4, 19] ----------------------------------------
IMG, INT_INTR, HALF_INTR = (32, 24), (8.0, 8.0, 15.5, 11.5), (8.0, 8.0, 15.0, 11.0)   # u = ix + 8, v = iy + 4  /  u = ix + 7.5, v = iy + 3.5
L = 10  # the depth-1 layer of most cases: camera depth (iz - 10) / 8 + 1, so iz = 2 lies at depth 0 and iz < 2 behind the camera


def _image_edges():
    W, H = SMALL
    T = pose(1.0, 1.0, layer_tz(L))
    checks = [(0, (1, 3, L), dict(u=0.0, in_image=True, updated=True)), (0, (0, 3, L), dict(u=-1.0, in_image=False, updated=False)),
              (0, (14, 3, L), dict(u=13.0, in_image=True, updated=True)), (0, (15, 3, L), dict(u=14.0, in_image=False)),
              (0, (3, 1, L), dict(v=0.0, in_image=True, updated=True)), (0, (3, 0, L), dict(v=-1.0, in_image=False)),
              (0, (3, 12, L), dict(v=11.0, in_image=True, updated=True)), (0, (3, 13, L), dict(v=12.0, in_image=False)),
              (0, (14, 12, L), dict(u=13.0, v=11.0, in_image=True, updated=True, in_band=True)), (0, (15, 13, L), dict(in_image=False)),
              (0, (5, 5, 2), dict(depth=0.0, front=False, updated=False)), (0, (5, 5, 1), dict(depth=-0.125, front=False)),
              (0, (5, 5, 3), dict(depth=0.125, front=True))]
    return _case("image_edges", SMALL, SMALL_INTR, [frame(0, T, plane(W, H, 1.0)), frame(1, T, plane(W, H, 1.0625))], checks, both=("in_image", "front"))


def _last_column():
    """u == W - 1 with dv == 0.5: the pair gather's second pixel is the first pixel of the NEXT image row (0.7 m behind here), which the
    last-column select has to keep out of the adaptive range test; rows differ by 1/64 m, so nearest and bilinear differ"""
    W, H = SMALL
    T = pose(1.0, 1.0, layer_tz(L))
    d = (1.0 + np.arange(H)[:, None] / 64.0) * np.ones((1, W))
    d[:, 0] = 1.75
    checks = [(0, (14, 5, L), dict(u=13.0, v=3.5, dv=0.5, use_nearest=False, best=0, sdf=float(F32(1.0 + 3.5 / 64) - F32(1.0)), in_band=True)),
              (0, (14, 12, L), dict(u=13.0, v=10.5, in_image=True, use_nearest=False)), (0, (14, 13, L), dict(v=11.5, in_image=False))]
    return _case("last_column", SMALL, (8.0, 8.0, 6.5, 6.0), [frame(0, T, d), frame(1, T, d)], checks, both=("in_image",))


def _tilted(W, H, k=0):
    """every pixel its own range, neighbours within 1/64 m (bilinear under the adaptive rule)"""
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    return (1.0 + ((u + 2 * v + k) % 8) / 512.0).astype(np.float32)


def _nearest_half():
    W, H = IMG
    tz = layer_tz(L)
    fr = [frame(0, pose(1.0, 1.0, tz), _tilted(W, H)), frame(1, pose(1.0 + 1 / 32, 1.0, tz), _tilted(W, H, 1)), frame(2, pose(1.0, 1.0 - 1 / 32, tz), _tilted(W, H, 2))]
    checks = [(0, (5, 5, L), dict(du=0.5, dv=0.5, use_nearest=True, best=3)), (1, (5, 5, L), dict(du=0.25, dv=0.5, best=1)),
              (2, (5, 5, L), dict(du=0.5, dv=0.75, best=3)), (1, (6, 6, L), dict(du=0.25, hi_u=False)), (0, (6, 6, L), dict(hi_u=True, hi_v=True))]
    return _case("nearest_half", IMG, HALF_INTR, fr, checks, both=("hi_u",), cfg=dict(interpolation_method=0))


def _first_max():
    """four equal bilinear weights: the FIRST pixel (u0, v0) is the mask pixel and the label pixel.  Voxel A's first pixel is painted
    in the dynamic image (masked: not updated), voxel B's last one (not masked); the four pixels carry four labels."""
    W, H = IMG
    T = pose(1.0, 1.0, layer_tz(L))
    dyn = np.zeros((H, W), np.int32)
    dyn[7, 11] = 1      # A = (4, 4, L): u = 11.5, v = 7.5 -> pixels (11..12, 7..8), first (11, 7)
    dyn[12, 18] = 1     # B = (10, 8, L): u = 17.5, v = 11.5 -> pixels (17..18, 11..12), last (18, 12)
    fr = [frame(k, T, plane(W, H, 1.0), dyn=dyn) for k in range(2)]
    checks = [(0, (4, 4, L), dict(du=0.5, dv=0.5, use_nearest=False, best=0, best_px=7 * W + 11, masked=True, updated=False)),
              (0, (10, 8, L), dict(du=0.5, dv=0.5, best=0, best_px=11 * W + 17, masked=False, updated=True, in_band=True))]
    return [_case("first_max_" + n, IMG, HALF_INTR, fr, checks, both=("masked",), cfg=dict(interpolation_method=m), use_mask=True)
            for n, m in (("bilinear", 1), ("adaptive", 2))]


def _adaptive_threshold():
    """mx - mn == the threshold (bilinear: the mean, 1.0) and above it by one ulp of the farthest range (nearest: the last pixel)"""
    W, H = IMG
    T = pose(1.0, 1.0, layer_tz(L))
    d = plane(W, H, 1.0)
    d[7:9, 11:13] = [[0.875, 1.0], [1.0, 1.125]]            # A = (4, 4, L)
    d[11:13, 17:19] = [[0.875, 1.0], [1.0, up(1.125)]]      # B = (10, 8, L)
    checks = [(0, (4, 4, L), dict(spread=0.25, use_nearest=False, sdf=0.0)), (0, (10, 8, L), dict(spread=float(F32(up(1.125)) - F32(0.875)), use_nearest=True, sdf=float(F32(up(1.125)) - F32(1.0))))]
    return _case("adaptive_threshold", IMG, HALF_INTR, [frame(0, T, d), frame(1, T, d)], checks, both=("use_nearest",), cfg=dict(adaptive_max_range_difference=0.25))


def _invalid_pixel():
    """one invalid pixel among the four -- depth 0, NaN, inf; as the first and as the last pixel -- under each interpolation method"""
    W, H = IMG
    T = pose(1.0, 1.0, layer_tz(L))
    d = plane(W, H, 1.0)
    sites = {}
    for n, (bad, (ix, iy)) in enumerate(zip((0.0, np.nan, np.inf, 0.0, np.nan, np.inf), ((2, 2), (6, 2), (10, 2), (2, 8), (6, 8), (10, 8)))):
        u0, v0 = ix + 7, iy + 3
        last = n >= 3
        d[v0 + (1 if last else 0), u0 + (1 if last else 0)] = bad
        sites[(ix, iy, L)] = last
    out = []
    for m in (0, 1, 2):
        checks = []
        for vox, last in sites.items():
            if m == 1:      # bilinear: the mean of (0, 1, 1, 1) is 0.75: sdf == -truncation, weight 0 under the drop-off
                checks.append((0, vox, dict(dist_surface=0.75, sdf=-0.25, w_zero=True, updated=False)))
            else:           # nearest (method 0, and the adaptive rule at a spread of 1 m): the last pixel
                checks.append((0, vox, dict(use_nearest=True, best=3, dist_surface=0.0 if last else 1.0, updated=not last)))
        checks.append((0, (13, 13, L), dict(dist_surface=1.0, updated=True)))
        out.append(_case("invalid_pixel_i%d" % m, IMG, HALF_INTR, [frame(0, T, d), frame(1, T, d)], checks, both=("updated",), cfg=dict(interpolation_method=m)))
    return out


SDF_SITES = [(0.75, "at -trunc"), (dn(0.75), "below -trunc"), (up(0.75), "above -trunc"), (1.25, "at +trunc"), (dn(1.25), "below +trunc"),
             (up(1.25), "above +trunc"), (1.0, "surface"), (0.875, "at -eps"), (dn(0.875), "below -eps"), (up(0.875), "above -eps"),
             (0.9375, "at -eps/2"), (dn(0.9375), "below -eps/2"), (up(0.9375), "above -eps/2")]


def _sdf_bounds():
    """integer pixels: the voxel (ix, iy, L) reads exactly pixel (ix + 8, iy + 4), whose range is SDF_SITES[(ix + 3 iy) % 13]"""
    W, H = IMG
    T = pose(1.0, 1.0, layer_tz(L))
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    vals = np.array([s[0] for s in SDF_SITES], np.float32)
    d = vals[((u - 8) + 3 * (v - 4)) % len(vals)]
    fr = [frame(k, T, d) for k in range(2)]

    def checks(dropoff, eps):
        out = []
        for n, (r, what) in enumerate(SDF_SITES):
            vox = (n, 0, L)      # (ix + 3 * 0) % 13 == n
            sdf = float(F32(r) - F32(1.0))
            ok = not sdf < -TRUNC
            zero = dropoff and sdf < -eps and float(F32(TRUNC) + F32(sdf)) <= 0.0
            out.append((0, vox, dict(du=0.0, dv=0.0, dist_surface=float(F32(r)), sdf=sdf, sdf_ok=ok, in_band=ok and abs(sdf) < TRUNC and not zero,
                                     w_zero=bool(zero and ok), updated=ok and not zero, below_eps=sdf < -eps)))
        return out
    c = []
    c.append(_case("sdf_bounds", IMG, INT_INTR, fr, checks(True, 0.125), both=("sdf_ok", "in_band", "w_zero", "updated", "below_eps")))
    c.append(_case("sdf_bounds_no_dropoff", IMG, INT_INTR, fr, checks(False, 0.125), both=("sdf_ok", "in_band", "updated"), cfg=dict(use_weight_dropoff=0)))
    c.append(_case("dropoff_eps_positive", IMG, INT_INTR, fr, checks(True, 0.125), both=("below_eps",), cfg=dict(weight_dropoff_epsilon=0.125)))
    c.append(_case("dropoff_eps_negative", IMG, INT_INTR, fr, checks(True, 0.0625), both=("below_eps",), cfg=dict(weight_dropoff_epsilon=-0.5)))
    return c


def _range_gates():
    """the voxels (7, 7, iz) lie on the optical axis: their range is their depth in both range modes, they read exactly the principal
    pixel, and that pixel's range is its depth in both modes.  min_range 0.5 (iz = 1), max_range 2 (iz = 13)."""
    W, H = IMG
    T = pose(0.9375, 0.9375, layer_tz(5))
    fr = []
    for k, r in enumerate((0.5, dn(0.5), 2.0, up(2.0))):
        d = plane(W, H, 1.0)
        d[11, 15] = r
        fr.append(frame(k, T, d))
    checks = [(0, (7, 7, 1), dict(u=15.0, v=11.0, range=0.5, in_range=True, dist_surface=0.5, surf_ok=True, updated=True)),
              (0, (7, 7, 0), dict(range=0.375, in_range=False, updated=False)),
              (1, (7, 7, 1), dict(dist_surface=dn(0.5), surf_ok=False, updated=False)),
              (2, (7, 7, 13), dict(range=2.0, in_range=True, dist_surface=2.0, surf_ok=True, updated=True)),
              (2, (7, 7, 14), dict(range=2.125, in_range=False, updated=False)),
              (3, (7, 7, 13), dict(dist_surface=up(2.0), surf_ok=False, updated=False))]
    return [_case("range_gates_mode%d" % m, IMG, (8.0, 8.0, 15.0, 11.0), fr, checks, both=("in_range", "surf_ok"), ranges=(0.5, 2.0), cfg=dict(range_mode=m))
            for m in (0, 1)]


def _sdf_neighbours():
    """the float32 neighbours of the bound itself: the voxel (7, 7, 0) on the optical axis has range 0.375 and reads the principal
    pixel; a surface at 0.125, 0.125 - 2^-25 and 0.125 + 2^-26 puts its signed distance ON -truncation, on the next float below
    (outside) and on the next float above (inside) -- each difference is exact.  (+truncation has no such pair in this geometry:
    a range of at least 0.25 steps by 2^-25 or more, twice the spacing of the floats below 0.25.)"""
    W, H = IMG
    T = pose(0.9375, 0.9375, layer_tz(5))
    fr = []
    for k, r in enumerate((0.125, 0.125 - 2.0 ** -25, 0.125 + 2.0 ** -26, 0.375)):
        d = plane(W, H, 1.0)
        d[11, 15] = r
        fr.append(frame(k, T, d))
    below, above = float(np.nextafter(F32(-0.25), F32(-1))), float(np.nextafter(F32(-0.25), F32(0)))
    out = []
    for name, dropoff in (("sdf_neighbours", 1), ("sdf_neighbours_no_dropoff", 0)):
        checks = [(0, (7, 7, 0), dict(u=15.0, v=11.0, range=0.375, sdf=-0.25, sdf_ok=True, w_zero=bool(dropoff), updated=not dropoff)),
                  (1, (7, 7, 0), dict(sdf=below, surf_ok=True, sdf_ok=False, updated=False)),
                  (2, (7, 7, 0), dict(sdf=above, sdf_ok=True, w_zero=False, updated=True, in_band=True)),
                  (3, (7, 7, 0), dict(sdf=0.0, updated=True))]
        out.append(_case(name, IMG, (8.0, 8.0, 15.0, 11.0), fr, checks, both=("sdf_ok", "updated"), ranges=(0.0625, 2.0), cfg=dict(use_weight_dropoff=dropoff)))
    return out


def _max_weight():
    """a measurement at depth 1 weighs exactly 1: with max_weight 2.5 the voxels of layer L saturate at the third of five frames"""
    W, H = IMG
    T = pose(1.0, 1.0, layer_tz(L))
    fr = [frame(k, T, plane(W, H, (1.0, 1.0625, 0.9375, 1.125, 1.0)[k])) for k in range(5)]
    return _case("max_weight", IMG, INT_INTR, fr, [(0, (5, 5, L), dict(depth=1.0, updated=True))], cfg=dict(max_weight=2.5))


def _colour_rounding():
    """u on a pixel, v half way: weights (1/2, 1/2, 0, 0).  Frame 0: colours 10 and 11 -> 10.5 -> 11; every channel of every pixel.
    Frame 1: colour 12 everywhere: (11 w_v + 12) / (w_v + 1) = 11.5 with the weight before the update (1), 11.33 with the weight after."""
    W, H = IMG
    T = pose(1.0, 1.0, layer_tz(L))
    c0 = np.zeros((H, W, 3), np.uint8)
    c0[:] = (10 + (np.arange(H) % 2))[:, None, None]
    c1 = np.full((H, W, 3), 12, np.uint8)
    fr = [frame(0, T, plane(W, H, 1.0), rgb=c0), frame(1, T, plane(W, H, 1.0), rgb=c1)]
    checks = [(0, (5, 5, L), dict(du=0.0, dv=0.5, use_nearest=False, in_band=True))]
    return [_case("colour_rounding_blend%d" % b, IMG, (8.0, 8.0, 15.5, 11.0), fr, checks, cfg=dict(color_blend_weight=b)) for b in (0, 1)]


def _generic_frames(n=3, K=4):
    W, H = IMG
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    fr = []
    for k in range(n):
        d = 1.03 + 0.011 * u + 0.007 * v + 0.013 * k
        d[(u > 20) & (v < 8)] += 0.37          # a step: the adaptive rule turns to the nearest pixel along it
        d[3, 5], d[17, 9] = 0.0, np.nan
        fr.append(frame(k, pose(1.013 + 0.021 * k, 0.987 - 0.017 * k, 0.29 + 0.009 * k), d, K=K))
    return fr


GENERIC_INTR = (17.3, 16.1, 15.7, 11.2)


def _generic():
    return _case("generic", IMG, GENERIC_INTR, _generic_frames(), track=True)


# ---- switch cases: the generic frames under every setting, and the layers of the map digest that differ from the default run ------
# A switch of the measurement WEIGHT moves values only (distance, weight, colour: the same voxels are updated, the frames hold no voxel
# at sdf == -truncation exactly).  A switch of the INTERPOLATION or of the range mode moves the surface range along the step and the
# invalid pixels of the frames, and with it voxels across the -truncation bound and the band: which voxels are observed (stamps), which
# hold likelihoods (flags), and what they hold.  The label confidence only scales the likelihoods; the arg-max stays.
VALUES = ("distance", "weight", "color")
DECISIONS = VALUES + ("last_observed", "flags", "sem_label", "likelihoods")
SWITCHES = {
    "default": (dict(), ()),
    "constant_weight": (dict(use_constant_weight=1), VALUES),
    "no_dropoff": (dict(use_weight_dropoff=0), VALUES),
    "eps_positive": (dict(weight_dropoff_epsilon=0.03), VALUES),
    "eps_negative": (dict(weight_dropoff_epsilon=-0.4), VALUES),
    "interp0_range0": (dict(interpolation_method=0, range_mode=0), DECISIONS),
    "interp1_range0": (dict(interpolation_method=1, range_mode=0), DECISIONS),
    "interp0_range1": (dict(interpolation_method=0, range_mode=1), DECISIONS),
    "interp1_range1": (dict(interpolation_method=1, range_mode=1), DECISIONS),
    "interp2_range1": (dict(interpolation_method=2, range_mode=1), DECISIONS),
    "adaptive_diff": (dict(adaptive_max_range_difference=0.005), DECISIONS),
    "label_confidence": (dict(label_confidence=0.6), ("likelihoods",)),
}


def _switch_cases():
    return {n: dict(_case("switch_" + n, IMG, GENERIC_INTR, _generic_frames(), cfg=cfg), differs=set(differs)) for n, (cfg, differs) in SWITCHES.items()}


# ---- label cases -------------------------------------------------------------------------------------------------------------------
LABEL_COUNTS = (1, 2, 3, 4, 5, 7, 8, 20, 32, 33, 64, 65, 128, 129, 161, 193, 256, 257)   # (161, 193: rows of 192 and 224 floats)
LL = 7   # the depth-1 layer of the label frames: the layers 6, 7 end a wave item (of 4 layers in 16^3 blocks, of 2 in 8^3 blocks), 8 starts one


def label_values(K):
    """every valid label, and -1, K, K + 5"""
    return np.array([-1] + list(range(K)) + [K, K + 5], np.int32)


def _label_frames(K):
    """frames 0 / 1 / 6: the plane at depth 1 (layers 6, 7, 8 in the band: full items, and items of exactly 64); frame 2: one pixel of
    surface in front of a far wall (an item with ONE in-band voxel, one with two); frame 3: the plane with one pixel a layer further
    (64 + 1; the label cases lower the adaptive threshold to 1/16 m, so that pixel is taken or left whole); frames 4 / 5: the plane
    at 1.3125 (layers 8 .. 11 in the band: a whole item of a 16^3 block, 256 records).  The label image is shifted between the
    frames: the layers 9 .. 11 see two labels once each -- an exact tie at the top of the row, the smaller label wins -- and every
    label a voxel does not see ties with all the others it does not see."""
    W, H = IMG
    T = pose(1.0, 1.0, layer_tz(LL))
    seq = label_values(K)
    u, v = np.meshgrid(np.arange(W), np.arange(H))

    def lab(shift):
        return seq[(u * 7 + v * 13 + shift) % len(seq)]
    single = plane(W, H, 3.0)
    single[12, 16] = 1.0
    bump = plane(W, H, 1.0)
    bump[12, 16] = 1.125
    depths = [plane(W, H, 1.0), plane(W, H, 1.0), single, bump, plane(W, H, 1.3125), plane(W, H, 1.3125), plane(W, H, 1.0)]
    return [frame(k, T, d, label=lab(s)) for k, (d, s) in enumerate(zip(depths, (0, 1, 3, 0, 2, 4, 1)))]


LABEL_CFG = dict(adaptive_max_range_difference=0.0625)


def _label_cases():
    c = {}
    for K in LABEL_COUNTS:
        big = K >= 161      # one 8^3 block: the likelihood pool stays small
        c["labels_%d" % K] = _case("labels_%d" % K, IMG, INT_INTR, _label_frames(K), K=K, ranges=(0.125, 4.0), cfg=LABEL_CFG,
                                   region=((8, 8, 8), (16, 16, 16)) if big else ((0, 0, 0), (16, 16, 16)), only_vps=8 if big else None)
    # the binary object layer: two counters per voxel, the label is "the object image carries OBJECT_ID here"
    c["labels_2_binary"] = _case("labels_2_binary", IMG, INT_INTR, _label_frames(2), K=2, ranges=(0.125, 4.0), cfg=dict(LABEL_CFG, semantic_mode=1))
    return c


EDGE_CASES = {}
for _c in ([_image_edges(), _last_column(), _nearest_half(), _adaptive_threshold(), _max_weight()] + _first_max() + _invalid_pixel() + _sdf_bounds()
           + _sdf_neighbours() + _range_gates() + _colour_rounding()):
    EDGE_CASES[_c["name"]] = _c
GENERIC = _generic()
SWITCH_CASES = _switch_cases()
LABEL_CASES = _label_cases()


def object_image(fr):
    """the object layer's image of a frame: the label image itself, OBJECT_ID marks the object"""
    return fr["label"]


# ---- the oracle's run of a case ----------------------------------------------------------------------------------------------------
def run_oracle(case, kw, allocate=False, vps=None, stamps=None, keep_each=False, track=None):
    """the frames of the case on a fresh OracleMap configured by kw (config()); explicit blocks unless `allocate`; stamps: one per
    frame in place of the frames' own (the cameras of a tick share one); track: run the tracking pass after every frame (default:
    the case's choice).  Returns (ora, [statistics per frame], [snapshot after each frame] if keep_each)"""
    from khronos_amd import default_config
    cfg = default_config(**kw)
    ora = po.OracleMap(po.config_from(cfg, 1))
    W, H = case["size"]
    sen = ora.make_sensor(W, H, *case["intr"], *case["ranges"])
    if not allocate:
        ora.allocate_blocks(blocks(case, vps or kw["voxels_per_side"]))
    stats, each = [], []
    binary = kw.get("semantic_mode", 0) == 1
    track = case["track"] if track is None else track
    for k, f in enumerate(case["frames"]):
        stamp = f["stamp"] if stamps is None else stamps[k]
        mask = f["dyn"] if case["use_mask"] else None
        if binary:
            st = ora.integrate(sen, stamp, f["pose"], f["depth"], f["rgb"], None, mask=mask, object_image=object_image(f), object_id=OBJECT_ID,
                               allocate_blocks=allocate)
        else:
            st = ora.integrate(sen, stamp, f["pose"], f["depth"], f["rgb"], f["label"], mask=mask, allocate_blocks=allocate)
        stats.append(st)
        if track:
            ora.update_tracking(stamp)
        if keep_each:
            each.append(snapshot(ora))
    return ora, stats, each


def snapshot(m, likelihoods=True):
    """{block index: layers} of an OracleMap or a FusionContext"""
    get = m.get_block if hasattr(m, "get_block") else m.download_block
    return {tuple(int(x) for x in b): get(b, likelihoods) for b in m.block_indices()}


def voxel_of(snap, vps, vox):
    """the layers of one voxel (global voxel coordinates) of a snapshot"""
    b = tuple(c // vps for c in vox)
    lin = (vox[0] % vps) + vps * ((vox[1] % vps) + vps * (vox[2] % vps))
    blk = snap[b]
    return {k: (blk[k][:, lin] if k == "likelihoods" else blk[k][lin]) for k in ("distance", "weight", "color", "sem_label", "likelihoods", "flags", "last_observed")
            if blk.get(k) is not None}
