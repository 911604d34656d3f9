"""Shows on the CPU that every case of tests/update_cases.py is what it claims to be, so that tests/test_gpu_update_cases.py can stay
a thin comparison of the update kernels with the oracle over the same table.

`decide` is a float32 numpy restatement of the DECISIONS of oracle.cpp's integrateBlock -- projection, in the image, range gates,
interpolation mode, signed-distance bounds, band, mask pixel and label pixel, weight > 0 -- operation for operation, in its order.  It
is a third implementation beside the oracle and the kernels and replaces neither: it says WHERE a voxel sits (u == W - 1 exactly,
truncation + sdf == 0 exactly), which neither of the two can be asked.  Its updated / in-band counts must equal the oracle's
statistics for every frame of every case; the values (distance, weight, colour, likelihoods) stay the oracle's business, except the
likelihood rows, which are simple enough to accumulate directly."""
import math
import os

import numpy as np
import pytest

import common
import update_cases as uc
from khronos_amd import default_config

F32 = np.float32


def decide(case, k, kw):
    """the decisions of frame k of a case for every voxel of its region, arrays [iz, iy, ix] (oracle.cpp: integrateBlock, computeInterp,
    makeRange, makePose)"""
    cfg = default_config(**kw)
    f = case["frames"][k]
    W, H = case["size"]
    fx, fy, cx, cy = (F32(x) for x in case["intr"])
    mn, mx = (F32(x) for x in case["ranges"])
    vs, trunc = F32(cfg.voxel_size), F32(cfg.truncation_distance)
    T = f["pose"]
    R = T[:3, :3].T.astype(F32)
    t = np.array([-(T[0, r] * T[0, 3] + T[1, r] * T[1, 3] + T[2, r] * T[2, 3]) for r in range(3)]).astype(F32)
    d = f["depth"]
    ok = (d > 0) & np.isfinite(d)
    with np.errstate(all="ignore"):
        if cfg.range_mode == 0:
            rng = np.where(ok, d, F32(0))
        else:
            pu, pv = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32))
            x, y = (pu - cx) / fx, (pv - cy) / fy
            rng = np.where(ok, d * np.sqrt((x * x + y * y) + F32(1)), F32(0))
        rng = rng.astype(F32).reshape(-1)
        lo, hi = case["region"]
        iz, iy, ix = np.meshgrid(*(np.arange(lo[a], hi[a]) for a in (2, 1, 0)), indexing="ij")
        px, py, pz = ((i.astype(F32) + F32(0.5)) * vs for i in (ix, iy, iz))
        pc = [((R[c, 0] * px + R[c, 1] * py) + R[c, 2] * pz) + t[c] for c in range(3)]
        o = dict(depth=pc[2], front=pc[2] > 0)
        o["range"] = pc[2] if cfg.range_mode == 0 else np.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2])
        o["in_range"] = ~((o["range"] < mn) | (o["range"] > mx))
        u, v = (pc[0] * fx) / pc[2] + cx, (pc[1] * fy) / pc[2] + cy
        o["u"], o["v"] = u, v
        o["in_image"] = ~((np.ceil(u) >= F32(W)) | (np.floor(u) < 0)) & ~((np.ceil(v) >= F32(H)) | (np.floor(v) < 0))
        valid = o["front"] & o["in_range"] & o["in_image"]
        us, vs_ = np.where(valid, u, F32(0)), np.where(valid, v, F32(0))
        u0, v0 = np.floor(us).astype(np.int64), np.floor(vs_).astype(np.int64)
        u1, v1 = np.minimum(u0 + 1, W - 1), np.minimum(v0 + 1, H - 1)
        du, dv = us - u0.astype(F32), vs_ - v0.astype(F32)
        o["du"], o["dv"], o["hi_u"], o["hi_v"] = du, dv, du >= F32(0.5), dv >= F32(0.5)
        pix = np.stack([v0 * W + u0, v1 * W + u0, v0 * W + u1, v1 * W + u1])
        r4 = rng[pix]
        nearest = np.where(o["hi_u"], 2, 0) + np.where(o["hi_v"], 1, 0)
        o["spread"] = r4.max(0) - r4.min(0)
        use_nearest = np.full(u.shape, cfg.interpolation_method == 0)
        if cfg.interpolation_method == 2:
            use_nearest = o["spread"] > F32(cfg.adaptive_max_range_difference)
        o["use_nearest"] = use_nearest
        one = F32(1)
        wb = np.stack([(one - du) * (one - dv), (one - du) * dv, du * (one - dv), du * dv])
        wn = (np.arange(4)[:, None, None, None] == nearest[None]).astype(F32)
        w4 = np.where(use_nearest[None], wn, wb)
        o["best"] = np.where(use_nearest, nearest, np.argmax(wb, axis=0))      # argmax: the first maximum
        o["best_px"] = np.take_along_axis(pix, o["best"][None], 0)[0]
        dist = ((w4[0] * r4[0] + w4[1] * r4[1]) + w4[2] * r4[2]) + w4[3] * r4[3]
        o["dist_surface"] = dist
        o["surf_ok"] = (dist >= mn) & ~(dist > mx)
        sdf = dist - o["range"]
        o["sdf"] = sdf
        o["sdf_ok"] = ~(sdf < -trunc)
        reach = valid & o["surf_ok"] & o["sdf_ok"]
        band = reach & (np.abs(sdf) < trunc)
        masked = np.zeros(u.shape, bool)
        if case["use_mask"] and f["dyn"] is not None:
            masked = band & (f["dyn"].reshape(-1)[o["best_px"]] != 0)
        o["masked"] = masked
        e = F32(cfg.weight_dropoff_epsilon)
        eps = e if e > 0 else e * -vs
        o["below_eps"] = sdf < -eps
        # computeWeight: positive factors times (trunc + sdf) / (trunc - eps): not positive exactly where that ratio is not
        o["w_zero"] = reach & ~masked & bool(cfg.use_weight_dropoff) & o["below_eps"] & (((trunc + sdf) / (trunc - eps)) <= 0)
        o["updated"] = reach & ~masked & ~o["w_zero"]
        o["in_band"] = band & o["updated"]
    o["origin"] = lo
    return o


def at(o, vox, field):
    lo = o["origin"]
    return o[field][vox[2] - lo[2], vox[1] - lo[1], vox[0] - lo[0]]


ALL_CASES = dict(uc.EDGE_CASES, generic=uc.GENERIC, **{c["name"]: c for c in uc.SWITCH_CASES.values()}, **uc.LABEL_CASES)
EDGE_NAMES = sorted(uc.EDGE_CASES)


def test_every_case_can_reach_the_multi_frame_kernels():
    """multiApplies declines a batch of one frame, and a tick of one camera is no rig: every case holds two frames or more"""
    for name, case in ALL_CASES.items():
        assert uc.MIN_MULTI_FRAMES <= len(case["frames"]) <= 8, name
        chunks = uc.tick_chunks(case)
        assert all(2 <= b - a <= uc.TICK_CAMERAS for a, b in chunks), (name, chunks)     # every tick is a rig of two or three cameras
        assert [k for a, b in chunks for k in range(a, b)] == list(range(len(case["frames"]))) and len(uc.tick_stamps(case)) == len(case["frames"])
    # the bounds are those of the source
    hip = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "khronos_amd", "csrc", "khronos_amd.hip")).read()
    assert "n_frames < %d || n_frames > kMaxMultiFrames" % uc.MIN_MULTI_FRAMES in hip and "constexpr int kMaxMultiFrames = %d;" % uc.MAX_MULTI_FRAMES in hip


def test_every_edge_class_has_a_case():
    """the classes of the issue, by the decision fields their cases pin"""
    pinned = {}
    for c in uc.EDGE_CASES.values():
        for _, _, want in c["checks"]:
            for k in want:
                pinned.setdefault(k, set()).add(c["name"])
    for field in ("u", "v", "in_image", "du", "dv", "hi_u", "best", "best_px", "masked", "spread", "use_nearest", "dist_surface", "sdf", "sdf_ok",
                  "in_band", "w_zero", "below_eps", "range", "in_range", "surf_ok", "depth", "front", "updated"):
        assert pinned.get(field), field
    assert len(uc.EDGE_CASES) >= 18 and len(uc.LABEL_CASES) == len(uc.LABEL_COUNTS) + 1 and len(uc.SWITCH_CASES) == 12


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_named_voxels_sit_on_their_edges(name):
    case = uc.EDGE_CASES[name]
    kw = uc.config(case, 16)
    dec = {k: decide(case, k, kw) for k in {c[0] for c in case["checks"]}}
    assert case["checks"], name
    seen = {}
    for k, vox, want in case["checks"]:
        for field, value in want.items():
            got = at(dec[k], vox, field)
            assert got == value and type(value)(got) == value, (name, k, vox, field, got, value)   # exactly: == on float32, no tolerance
            seen.setdefault(field, set()).add(bool(got) if isinstance(value, bool) else None)
    for field in case["both"]:
        assert seen.get(field) == {True, False}, (name, "both sides of", field, seen.get(field))


@pytest.mark.parametrize("name,vps", [(n, v) for n in sorted(ALL_CASES) for v in uc.vps_of(ALL_CASES[n])])
def test_oracle_counts_equal_the_restatement(name, vps):
    """updated and in-band voxels of every frame: the oracle's statistics against the restatement's decisions, and the voxels themselves
    by their stamps (last_observed == the frame's stamp exactly where the restatement updates)"""
    case = ALL_CASES[name]
    kw = uc.config(case, vps)
    ora, stats, each = uc.run_oracle(case, kw, keep_each=True)
    try:
        total = 0
        for k, (st, snap) in enumerate(zip(stats, each)):
            o = decide(case, k, kw)
            assert st["n_updated_voxels"] == int(o["updated"].sum()), (name, k, st["n_updated_voxels"], int(o["updated"].sum()))
            assert st["n_band_voxels"] == int(o["in_band"].sum()), (name, k, st["n_band_voxels"], int(o["in_band"].sum()))
            total += st["n_updated_voxels"]
            lo, hi = case["region"]
            for b, blk in snap.items():
                sl = tuple(slice(b[a] * vps - lo[a], (b[a] + 1) * vps - lo[a]) for a in (2, 1, 0))
                stamped = blk["last_observed"].reshape(vps, vps, vps) == case["frames"][k]["stamp"]
                assert np.array_equal(stamped, o["updated"][sl]), (name, k, b)
        assert total > 0
    finally:
        ora.close()


def _digest(case, **extra):
    ora, _, _ = uc.run_oracle(case, uc.config(case, 16, **extra))
    try:
        return [int(x) for x in ora.map_digest()]
    finally:
        ora.close()


def test_switches_change_the_stated_layers_and_no_other():
    base = _digest(uc.SWITCH_CASES["default"])
    for name, case in uc.SWITCH_CASES.items():
        dg = _digest(case)
        differs = {n for n, a, b in zip(common.DIGEST_LAYERS, base, dg) if a != b}
        assert differs == case["differs"], (name, sorted(differs), sorted(case["differs"]))


def test_first_touch_is_the_measurement_itself():
    """the running average at w_old == 0: (0 * 0 + sdf w) / (0 + w) = sdf, for the clamped sdf of the voxel on the surface and at both bounds"""
    case = uc.EDGE_CASES["sdf_bounds_no_dropoff"]
    ora, _, each = uc.run_oracle(case, uc.config(case, 16), keep_each=True)
    ora.close()
    o = decide(case, 0, uc.config(case, 16))
    for n, (r, what) in enumerate(uc.SDF_SITES):
        vox = (n, 0, uc.L)
        got = uc.voxel_of(each[0], 16, vox)
        if at(o, vox, "updated"):
            assert got["weight"] == 1.0 and got["distance"] == min(F32(uc.TRUNC), at(o, vox, "sdf")), (what, got["distance"], got["weight"])
        else:
            assert got["weight"] == 0.0 and got["distance"] == 0.0, what


def test_max_weight_saturates_before_the_last_frame():
    case = uc.EDGE_CASES["max_weight"]
    ora, _, each = uc.run_oracle(case, uc.config(case, 16), keep_each=True)
    ora.close()
    w = [float(uc.voxel_of(s, 16, (5, 5, uc.L))["weight"]) for s in each]
    assert w == [1.0, 2.0, 2.5, 2.5, 2.5], w
    d = [float(uc.voxel_of(s, 16, (5, 5, uc.L))["distance"]) for s in each]
    assert d[3] != d[2] and d[4] != d[3], "a saturated voxel still averages"


@pytest.mark.parametrize("blend,colours", [(0, (6, 8)), (1, (11, 12))])
def test_colour_rounds_half_up(blend, colours):
    """10.5 -> 11 from the image; then (0 + 11) / 2 = 5.5 -> 6 with the weight after the update, 11 with the weight before it; frame 1:
    (6 * 2 + 12) / 3 = 8, and (11 + 12) / 2 = 11.5 -> 12"""
    case = uc.EDGE_CASES["colour_rounding_blend%d" % blend]
    ora, _, each = uc.run_oracle(case, uc.config(case, 16), keep_each=True)
    ora.close()
    for s, want in zip(each, colours):
        assert uc.voxel_of(s, 16, (5, 5, uc.L))["color"].tolist() == [want] * 3 + [255]


def test_generic_case_keeps_clear_of_the_value_decisions():
    """no updated voxel of the generic case within TOL of distance 0 or of the occupancy threshold (after any frame): what the relaxed
    arithmetic may move (~1e-6 relative) cannot flip a decision on a value there, so compare_maps' borderline bound holds by construction"""
    case = uc.GENERIC
    # the explicitly allocated blocks (slot, batch), and every block of the frusta with the tick's stamps (the tick allocates)
    for vps, how in ((16, dict()), (8, dict()), (16, dict(allocate=True, stamps=uc.tick_stamps(case), track=False)),
                     (8, dict(allocate=True, stamps=uc.tick_stamps(case), track=False))):
        kw = uc.config(case, vps)
        thr = common.occupancy_threshold(default_config(**kw))
        ora, _, each = uc.run_oracle(case, kw, keep_each=True, **how)
        ora.close()
        n = 0
        for snap in each:
            for blk in snap.values():
                upd = blk["weight"] > 0
                n += int(upd.sum())
                dist = blk["distance"][upd]
                if not dist.size:       # (a block of the frustum that no ray reaches)
                    continue
                assert np.abs(dist).min() > common.TOL and np.abs(dist - F32(thr)).min() > common.TOL, (np.abs(dist).min(), np.abs(dist - F32(thr)).min())
        assert n > 1000


# ---- label cases -------------------------------------------------------------------------------------------------------------------
def _accumulate(case, kw, vps):
    """likelihood rows and labels of the case by direct accumulation over the restatement's in-band voxels"""
    cfg = default_config(**kw)
    K = cfg.num_labels
    lo, hi = case["region"]
    shape = tuple(hi[a] - lo[a] for a in (2, 1, 0))
    lik = np.zeros((K,) + shape, F32)
    empty = np.ones(shape, bool)
    label = np.zeros(shape, np.uint32)
    conf = F32(cfg.label_confidence)
    # (std::log of a float, correctly rounded: the double logarithm rounded once more)
    hit = F32(math.log(float(conf)))
    miss = F32(math.log(float((F32(1) - conf) / F32(K - 1)))) if K > 1 else F32(0)
    for k, f in enumerate(case["frames"]):
        o = decide(case, k, kw)
        seen = f["label"].reshape(-1)[o["best_px"]]
        if cfg.semantic_mode == 1:      # counters of "is the object" / "is not"
            seen, hit, miss = (uc.object_image(f).reshape(-1)[o["best_px"]] == uc.OBJECT_ID).astype(np.int32), F32(1), F32(0)
        upd = o["in_band"] & (seen >= 0) & (seen < K)
        lik[:, upd & empty] = 0
        empty &= ~upd
        add = np.where(np.arange(K)[:, None, None, None] == seen[None], hit, miss).astype(F32)
        lik = np.where(upd[None], lik + add, lik)
        label = np.where(upd, np.argmax(lik, axis=0).astype(np.uint32), label)
    return lik, label, empty


@pytest.mark.parametrize("name", sorted(uc.LABEL_CASES))
def test_label_rows_equal_a_direct_accumulation(name):
    case = uc.LABEL_CASES[name]
    vps = uc.vps_of(case)[-1]
    kw = uc.config(case, vps)
    ora, _, _ = uc.run_oracle(case, kw)
    snap = uc.snapshot(ora)
    ora.close()
    lik, label, empty = _accumulate(case, kw, vps)
    lo = case["region"][0]
    ties = 0
    for b, blk in snap.items():
        sl = tuple(slice(b[a] * vps - lo[a], (b[a] + 1) * vps - lo[a]) for a in (2, 1, 0))
        want = lik[(slice(None),) + sl].reshape(lik.shape[0], -1)
        assert np.array_equal(blk["likelihoods"], want), name
        assert np.array_equal(blk["sem_label"], label[sl].reshape(-1)), name
        assert np.array_equal((blk["flags"] & 8) == 0, empty[sl].reshape(-1)), name
        top = want.max(0)
        ties += int((((want == top[None]).sum(0) > 1) & ~empty[sl].reshape(-1)).sum())
    if case["K"] > 2 and case["frames"][0]["label"].min() < 0:
        assert ties > 0, "no voxel with a tie at the top of its row"
        assert (~empty).sum() > 0 and empty.sum() > 0


def item_counts(case, vps, kw=None):
    """in-band voxels per wave item (64 voxels of an x-y patch times 4 z layers of a 16^3 block, an 8 x 8 slice times 2 layers of an 8^3
    block) and frame: what the band phase of the update kernels works off per call"""
    kw = kw or uc.config(case, vps)
    zr = 4 if vps == 16 else 2
    out = []
    for k in range(len(case["frames"])):
        band = decide(case, k, kw)["in_band"]
        nz, ny, nx = band.shape
        for z0 in range(0, nz, zr):
            for by in range(0, ny, vps):
                for bx in range(0, nx, vps):
                    cell = band[z0:z0 + zr, by:by + vps, bx:bx + vps].reshape(zr, -1)
                    out += [int(cell[:, p:p + 64].sum()) for p in range(0, vps * vps, 64)]
    return out


def test_label_frames_cover_the_record_counts():
    """one record, fewer than the eight records of a pass of 32-float rows, exactly 64, 65, and a whole item (256 records in a 16^3
    block -- kRecCap, which no item can exceed: an item holds 64 voxels times at most 4 layers --, 128 in an 8^3 block)"""
    case = uc.LABEL_CASES["labels_20"]
    c16, c8 = item_counts(case, 16), item_counts(case, 8)
    for counts, full in ((c16, 256), (c8, 128)):
        assert 1 in counts and any(1 < n < 8 for n in counts) and 64 in counts and 65 in counts and full in counts, sorted(set(counts))
    one = uc.LABEL_CASES["labels_256"]
    c1 = item_counts(one, 8)
    assert 1 in c1 and 64 in c1 and 65 in c1 and 128 in c1, sorted(set(c1))
