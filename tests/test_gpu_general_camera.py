"""-m gpu: the device paths on a GENERAL camera (tests/general_camera.py: rolled, pitched poses at varying height, fx != fy, principal
point off centre by a non-integer amount), through the C ABI, against the CPU oracle, the numpy restatements and -- for the
integrator -- the analytic scene of tests/general_scene.py.  With the yaw-only poses of the rest of the suite one product of every
three-term dot product is an exact zero and fx, fy are interchangeable; here every term rounds and every parameter matters."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import common
import general_scene as gs
import render_replica as rr
from common import DeviceArray, assert_digests_equal, compare_maps, step_both
from general_camera import GENERAL_INTRINSICS, general_angles, make_general_pair, pose_rpy
from khronos_amd import FusionContext, default_config
from oracle import np_oracle as npo
from oracle import pyoracle as po
from test_gpu_render_view import assert_same_images

pytestmark = pytest.mark.gpu
OBJS = list(range(7, 20))


def general_sensor(width=160, height=120, min_range=0.1, max_range=5.0):
    return FusionContext.make_sensor(width, height, *GENERAL_INTRINSICS(width, height), min_range, max_range)


# ------------------------------------------------------------------------------------------------------------------ window parity
def run_window(n_frames=30, archive_every=5, **cfg_kw):
    """the run_stream shape of tests/test_gpu_map_slice.py on the general camera, compared after EVERY frame"""
    cfg, ctx, ora, s, sen, osen = make_general_pair(**cfg_kw)
    exact = bool(common.EXACT)
    seen = dict(seed_frames=0, archived=0, clusters=0, ever=set())
    last = None
    for i in range(n_frames):
        last = s.render(i)
        out = step_both(ctx, ora, sen, osen, last, motion=True, track=True)
        last["step"] = out
        assert out["n_gpu"] == out["n_ora"], (i, "cluster count", out["n_gpu"], out["n_ora"])
        assert np.array_equal(np.asarray(out["dyn_gpu"]).reshape(out["dyn_ora"].shape), out["dyn_ora"]), (i, "dynamic image")
        st = ctx.stats()
        assert st["n_updated_voxels"] == out["ostats"]["n_updated_voxels"], (i, st["n_updated_voxels"], out["ostats"]["n_updated_voxels"])
        assert st["n_band_voxels"] == out["ostats"]["n_band_voxels"], (i, st["n_band_voxels"], out["ostats"]["n_band_voxels"])
        assert_digests_equal(ctx.map_digest(), ora.map_digest(), exact=exact, what="frame %d" % i)
        seen["seed_frames"] += int(out["seeds_ora"] > 0)
        seen["clusters"] += out["n_ora"]
        seen["ever"] |= {tuple(b) for b in ora.block_indices().tolist()}
        if archive_every and i % archive_every == archive_every - 1:
            rg, ro = np.asarray(ctx.reset_inactive()), np.asarray(ora.reset_inactive())
            assert np.array_equal(rg, ro), (i, "archived blocks")
            seen["archived"] += len(ro.reshape(-1, 3))
    return SimpleNamespace(cfg=cfg, ctx=ctx, ora=ora, s=s, sen=sen, osen=osen, last=last, seen=seen, cache={}, exact=exact)


def check_window(st):
    ctx, ora = st.ctx, st.ora
    compare_maps(ctx, ora, max_blocks=120)
    ctx.generate_mesh(False, False)
    ora.generate_mesh(False, False)
    gm, om = ctx.download_mesh(), ora.mesh()
    assert gm["points"].shape == om["points"].shape and len(om["points"]) > 0
    assert np.array_equal(gm["labels"], om["labels"]) and np.array_equal(gm["stamps"], om["stamps"])
    if st.exact:
        assert gm["points"].tobytes() == om["points"].tobytes(), "mesh vertices"
        assert gm["colors"].tobytes() == om["colors"].tobytes(), "mesh colours"
    else:
        assert np.abs(gm["points"] - om["points"]).max() <= common.TOL
    # non-vacuity, on the oracle's side only; the blocks are those the window held on some frame (the stream ends on an archival
    # pass, which leaves only what a shaking camera saw in the last 0.6 s)
    idx = np.array(sorted(st.seen["ever"]))
    assert len(idx) > 100 and len(ora.block_indices()) > 0, (len(idx), len(ora.block_indices()))
    assert st.seen["seed_frames"] >= 1 and st.seen["archived"] >= 1, (st.seen["seed_frames"], st.seen["archived"])
    for axis in range(3):
        assert idx[:, axis].min() < 0 < idx[:, axis].max(), (axis, idx[:, axis].min(), idx[:, axis].max())


@pytest.mark.parametrize("vps", [16, 8])
def test_window_parity_general_camera(arith, vps):
    kw = dict(width=160, height=120, temporal_window=0.6)
    if vps == 8:
        kw.update(voxels_per_side=8, voxel_size=0.1, truncation_distance=0.3, max_blocks=16384)
    st = run_window(**kw)
    check_window(st)
    st.ctx.close()
    st.ora.close()


# --------------------------------------------------------------------------------------------------- range image and vertex map
@pytest.mark.parametrize("W,H", [(161, 119), (33, 17)])
@pytest.mark.parametrize("range_mode", [0, 1])
def test_range_image_and_vertex_map_general_intrinsics(W, H, range_mode):
    """range = z * |(x, y, 1)| (range_mode 1) depends on fx and fy separately; ragged sizes leave a partial tile on both axes"""
    cfg, ctx, ora, s, sen, osen = make_general_pair(width=W, height=H, range_mode=range_mode)
    for i in (3, 6):
        fr = s.render(i)
        fr["depth"][2:5, 7:30] = 0.0
        fr["depth"][H // 2, W // 2] = np.nan
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        r, v, _ = ctx.download_frame(slot, fr["depth"].shape, range_image=True, vertex_map=True)
        ro, vo = ora.parse_input(osen, fr["pose"], fr["depth"])
        assert r.tobytes() == ro.tobytes(), (i, "range image")
        assert v.tobytes() == vo.tobytes(), (i, "vertex map")
        assert (ro > 0).sum() > W * H // 2
        if range_mode == 1:
            # the definition, in float64, z * sqrt(x^2 + y^2 + 1) with the sensor's own fx, fy, cx, cy.  float32 (u = 2^-24): fx cast,
            # u - cx and the division make x relative 3u, x^2 7u, the two sums 2u more, the root halves that and adds u, the
            # product adds u: 6.5u relative, asserted as 8u (a swap of fx and fy moves the range by centimetres)
            vv, uu = np.nonzero(ro > 0)
            x, y = (uu - s.cx) / s.fx, (vv - s.cy) / s.fy
            want = fr["depth"][vv, uu].astype(np.float64) * np.sqrt(x * x + y * y + 1)
            assert (np.abs(ro[vv, uu] - want) <= 8 * 2.0 ** -24 * want).all()
    ctx.close()
    ora.close()


# ------------------------------------------------------------------------------------------- the analytic scene on the device
def test_analytic_scene_digest_and_mesh_on_the_surface(arith):
    """tests/general_scene.py's depth images through upload_frame / integrate: the map's digest equals the oracle's after every
    frame, and check (b) of tests/test_cpu_general_camera.py -- every mesh vertex within 0.5 * voxel_size of the analytic plane or
    sphere, at least 3 000 of them -- holds for the DEVICE's mesh.  Measured on the oracle: 41 736 vertices, maximum 0.0285 m."""
    fx, fy, cx, cy = GENERAL_INTRINSICS(gs.W, gs.H)
    cfg = default_config(voxel_size=0.1, truncation_distance=0.2, with_semantics=0, with_tracking=0, max_blocks=8192,
                         max_frame_pixels=gs.W * gs.H, exact_arithmetic=common.EXACT)
    ctx = FusionContext(cfg)
    ora = po.OracleMap(po.config_from(cfg, 0))
    sen = ctx.make_sensor(gs.W, gs.H, fx, fy, cx, cy, gs.MIN_RANGE, gs.MAX_RANGE)
    osen = ora.make_sensor(gs.W, gs.H, fx, fy, cx, cy, gs.MIN_RANGE, gs.MAX_RANGE)
    for stamp, pose, depth in gs.frames():
        slot = ctx.upload_frame(sen, stamp, pose, depth, None, None)
        ctx.integrate(slot)
        so = ora.integrate(osen, stamp, pose, depth, None, None)
        st = ctx.stats()
        assert st["n_updated_voxels"] == so["n_updated_voxels"] and st["n_visible_blocks"] == so["n_visible_blocks"]
        assert_digests_equal(ctx.map_digest(), ora.map_digest(), exact=bool(common.EXACT), what="analytic scene")
    ctx.generate_mesh(False, False)
    pts = ctx.download_mesh()["points"]
    dist = gs.surface_distance(pts)
    print("device mesh: %d vertices, max distance to the analytic surface %.4f m (bound 0.05 m)" % (len(dist), dist.max()))
    assert len(dist) >= 3000
    assert dist.max() <= 0.5 * 0.1
    ctx.close()
    ora.close()


# --------------------------------------------------------------------------------------------------------------------- rig tick
def test_tick_with_a_rig_of_pitched_and_rolled_cameras():
    """khr_tick_ingest / khr_tick_integrate with three cameras that differ in pitch and roll (and height), not in yaw only; the tick
    takes one sensor per call, so two intrinsics sets alternate between ticks.  == the oracle fed frame by frame
    (test_gpu_edge_cases.test_tick_with_blind_cameras)."""
    W, H = 160, 120
    cfg, ctx, ora, s, sen, osen = make_general_pair(width=W, height=H, num_frame_slots=6)
    other = (0.47 * W, 0.58 * W, W / 2.0 - 4.5, H / 2.0 + 1.25)  # fy > fx, the principal point off the other way
    sens = [(sen, osen, (s.fx, s.fy, s.cx, s.cy)), (ctx.make_sensor(W, H, *other), ora.make_sensor(W, H, *other), other)]
    # per camera: yaw offset, factors on the trajectory's pitch and roll (factors keep their common sign, general_camera.py), height offset
    rig = [(0.0, 1.0, 1.0, 0.0), (0.25, 1.5, 0.8, 0.2), (0.4, 0.8, 1.2, -0.25)]
    for tick in range(5):
        dsen, osen_t, intr = sens[tick % 2]
        s.s.fx, s.s.fy, s.s.cx, s.s.cy = intr  # (the renderer reads the stream's attributes)
        pos, yaw, pitch, roll = general_angles(tick)
        frs = [s.render(tick, pose=pose_rpy(pos + np.array([0.0, 0.0, dh]), yaw + dy, pitch * kp, roll * kr)) for dy, kp, kr, dh in rig]
        for f in frs:
            assert np.abs(f["pose"][:3, :3]).min() > 0.05
        stamp = frs[0]["stamp"]
        tens = [(DeviceArray(f["depth"]), DeviceArray(f["rgb"]), DeviceArray(f["label"])) for f in frs]
        frames = [ctx.make_frame(stamp, f["pose"], d.data_ptr(), c.data_ptr(), l.data_ptr()) for f, (d, c, l) in zip(frs, tens)]
        slots, _ = ctx.tick_ingest(dsen, frames, count_seeds=False)
        ctx.tick_integrate(slots, phases=3)
        ctx.update_tracking(stamp)
        ctx.sync()
        ou = ob = 0
        for f in frs:
            so = ora.integrate(osen_t, stamp, f["pose"], f["depth"], f["rgb"], f["label"])
            ou, ob = ou + so["n_updated_voxels"], ob + so["n_band_voxels"]
        ora.update_tracking(stamp)
        st = ctx.stats()
        assert st["n_updated_voxels"] == ou and st["n_band_voxels"] == ob, (tick, st["n_updated_voxels"], ou)
        assert ou > 10000
        assert_digests_equal(ctx.map_digest(), ora.map_digest(), exact=bool(common.EXACT), what="tick %d" % tick)
        for t3 in tens:
            for t in t3:
                t.free()
    assert np.array_equal(ctx.block_indices(), ora.block_indices())
    compare_maps(ctx, ora, max_blocks=80)
    ctx.close()
    ora.close()


# ------------------------------------------------------------------------------------------------------------ objects and tracker
def _compare_objects(ctx, ora, sen, osen, fr, **kw):
    """tests/test_gpu_objects._compare"""
    slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
    ctx.configure_object_detector(OBJS, **kw)
    n = ctx.detect_objects(slot)
    no, img_o, cl_o = ora.detect_objects(osen, fr["stamp"], fr["pose"], fr["depth"], fr["label"], OBJS, **kw)
    img_g = ctx.download_frame(slot, fr["depth"].shape, range_image=False, object_image=True)[3]
    assert n == no
    assert (img_g == img_o).all()
    cl_g = ctx.semantic_clusters(slot)
    assert len(cl_g) == len(cl_o) == n
    for g, o in zip(cl_g, cl_o):
        assert g["id"] == o["id"] and g["semantic_id"] == o["semantic_id"] and g["num_pixels"] == o["num_pixels"]
        assert (g["bbox_min"] == o["bbox_min"]).all() and (g["bbox_max"] == o["bbox_max"]).all()
        assert np.allclose(g["centroid"], o["centroid"], rtol=1e-4, atol=1e-4)
    return slot, n, img_o


def test_object_clusters_and_voxel_sets_general_camera():
    """test_gpu_objects.test_connected_semantics_parity and test_cluster_voxel_sets_parity once on the general camera: the 3D
    grid a pixel falls in comes from a vertex built with fx, fy, cx, cy and the full rotation"""
    cfg, ctx, ora, s, sen, osen = make_general_pair(320, 240, seed=77)
    total = 0
    for i in range(26, 40):
        _, n, _ = _compare_objects(ctx, ora, sen, osen, s.render(i), use_3d=True, use_full_connectivity=True, grid_size=0.1, max_range=4.5,
                                   min_cluster_size=0)
        total += n
    assert total >= 10
    fr = s.render(31)
    slot, n, img_o = _compare_objects(ctx, ora, sen, osen, fr, use_3d=True, grid_size=0.1, max_range=4.5, min_cluster_size=20)
    assert n >= 3
    for vs in (0.2, 0.05):
        gi, gv = ctx.cluster_voxels(slot, 1, vs)
        oi, ov = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], img_o, vs)
        assert len(gi) == len(oi) > n
        assert (gi == oi).all() and (gv == ov).all()
    found = False
    for i in range(0, 30):
        fr = s.render(i)
        out = step_both(ctx, ora, sen, osen, fr, motion=True)
        assert out["n_gpu"] == out["n_ora"]
        if out["n_gpu"] > 0:
            gi, gv = ctx.cluster_voxels(out["slot"], 0, 0.2)
            oi, ov = ora.cluster_voxels(osen, fr["stamp"], fr["pose"], fr["depth"], out["dyn_ora"], 0.2)
            assert len(gi) == len(oi) > 0 and (gi == oi).all() and (gv == ov).all()
            found = True
    assert found
    ctx.close()
    ora.close()


def test_pixel_iou_general_camera():
    """test_gpu_tracking_pixels.test_pixel_iou_matches_numpy_restatement with the real fx, fy, cx, cy of the general sensor and a
    pose that is a small FULL rotation (computeIoUPixels applies world_T_sensor as it is, so only a pose near the identity puts
    re-projected points into the image; every entry of this one is non-zero)."""
    W, H = 320, 240
    cfg, ctx, ora, s, sen, osen = make_general_pair(width=W, height=H, num_frame_slots=4)
    kw = dict(use_3d=True, grid_size=0.1, max_range=5.0, min_cluster_size=50, use_full_connectivity=True)
    ctx.configure_object_detector(OBJS, **kw)
    a, b, c = 0.021, -0.017, 0.026
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
    pose = np.eye(4)
    pose[:3, :3] = Rz @ Ry @ Rx
    pose[:3, 3] = (0.01, -0.02, 0.015)
    assert (pose[:3, :3] != 0).all()

    def frame(i):
        fr = s.render(i)
        fr["pose"] = pose
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        assert ctx.detect_objects(slot) >= 0
        vm = ora.parse_input(osen, fr["pose"], fr["depth"])[1]
        _, oimg, cl = ora.detect_objects(osen, fr["stamp"], fr["pose"], fr["depth"], fr["label"], OBJS, **kw)
        return fr, slot, vm, oimg, cl
    fr0, slot0, vm0, oimg0, cl0 = frame(30)
    fr1, slot1, vm1, oimg1, cl1 = frame(31)
    assert len(cl0) >= 1 and len(cl1) >= 1
    refs = [(slot0, 1, c_["id"]) for c_ in cl0][:8] + [(slot1, 1, cl1[0]["id"])]
    max_id = max(c_["id"] for c_ in cl1)
    n_points, inter = ctx.pixel_iou(slot1, refs, max_id)
    for r, (sl, _, cid) in enumerate(refs):
        img, vm = (oimg0, vm0) if sl == slot0 else (oimg1, vm1)
        vs, us = np.nonzero(img == cid)
        pts = vm[vs, us]
        assert n_points[r] == len(pts)
        for c_ in cl1:
            cv, cu = np.nonzero(oimg1 == c_["id"])
            iou, n_inter = npo.iou_pixels(list(zip(cu.tolist(), cv.tolist())), pts, fr1["pose"], s.fx, s.fy, s.cx, s.cy, W, H)
            assert inter[r, c_["id"]] == n_inter, (r, c_["id"], inter[r, c_["id"]], n_inter)
    # a reference of the earlier frame meets a cluster of this frame: the association the tracker would make
    assert inter[: len(refs) - 1].sum() > 0
    ctx.close()
    ora.close()


def test_object_map_extraction_general_camera():
    """test_gpu_parity.test_no_semantics_no_color_8vps_object_map (the extractor's mini-map: explicit allocation, integration of the
    object's pixels only, pruning, meshing) against the oracle on the general camera; at least one object comes out (a mesh)."""
    cfg, ctx, ora, s, sen, osen = make_general_pair(voxels_per_side=8, voxel_size=0.04, truncation_distance=0.08,
                                                    with_tracking=0, semantic_mode=1, num_labels=2, max_blocks=8192)
    frames = [s.render(i) for i in range(4)]
    # the object: the most frequent object label of frame 0
    labs, counts = np.unique(frames[0]["label"][np.isin(frames[0]["label"], OBJS)], return_counts=True)
    target = int(labs[np.argmax(counts)])
    vm = ora.parse_input(osen, frames[0]["pose"], frames[0]["depth"])[1]
    sel = (frames[0]["label"] == target) & (frames[0]["depth"] > 0)
    lo = np.floor(vm[sel].min(0) / (8 * 0.04)).astype(int) - 1
    hi = np.floor(vm[sel].max(0) / (8 * 0.04)).astype(int) + 1
    hi = np.minimum(hi, lo + 14)
    bl = np.array([[x, y, z] for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)], np.int32)
    assert 0 < len(bl) <= 4096
    ctx.allocate_blocks(bl)
    ora.allocate_blocks(bl)
    for fr in frames:
        obj = (fr["label"] == target).astype(np.int32) * 3
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], None)
        ctx.set_frame_image(slot, 1, obj)
        ctx.integrate(slot, allocate_blocks=False, use_mask=False, object_id=3)
        ora.integrate(osen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], None, object_image=obj, object_id=3, allocate_blocks=False)
    compare_maps(ctx, ora)
    assert ctx.object_prune(0.5, 2.0) == ora.object_prune(0.5, 2.0)
    ctx.generate_mesh(True, False)
    ora.generate_mesh(True, False)
    gm, om = ctx.download_mesh(), ora.mesh()
    assert gm["points"].shape == om["points"].shape and len(om["points"]) > 0, "no object was extracted"
    assert np.abs(gm["points"] - om["points"]).max() <= common.TOL
    compare_maps(ctx, ora)
    ctx.close()
    ora.close()


# -------------------------------------------------------------------------------------------------------------------- render view
@pytest.fixture(scope="module")
def window():
    st = run_window(width=160, height=120, temporal_window=0.6)
    yield st
    st.ctx.close()
    st.ora.close()


def general_views(last_pose, last_sensor):
    """name -> (sensor, pose, step_voxels)"""
    return {
        # the last frame's own general pose and sensor
        "own": (last_sensor, last_pose, 0.0),
        # pitched down by 1 rad from above the room, rolled
        "from_above": (general_sensor(), pose_rpy([0.2, 1.0, 2.9], 1.9, -1.0, 0.25), 0.0),
        # outside the map looking in, rolled and pitched: every Rw entry non-zero while renderSkipTo skips
        "outside_in_rolled": (general_sensor(max_range=12.0), pose_rpy([9.0, 0.5, 2.6], math.pi + 0.15, -0.12, 0.3), 0.5),
        # the optical axis exactly along world +x, rolled by 0.3 rad: Rw keeps exact zeros in its first row only
        "on_axis_rolled": (general_sensor(), pose_rpy(np.asarray(last_pose)[:3, 3], 0.0, 0.0, 0.3), 1.0),
    }


def _replica(st, which, sensor, pose, step):
    if which not in st.cache:
        src = st.ctx if which == "ctx" else st.ora
        get = st.ctx.download_block if which == "ctx" else st.ora.get_block
        st.cache[which] = rr.BlockSet(src.block_indices(), get, st.cfg.voxels_per_side)
    return rr.render(None, None, st.cfg.voxels_per_side, st.cfg.voxel_size, sensor, pose, step_voxels=step,
                     min_weight=st.cfg.mesh_min_weight, with_semantics=bool(st.cfg.with_semantics), blocks=st.cache[which])


@pytest.mark.parametrize("name", ["own", "from_above", "outside_in_rolled", "on_axis_rolled"])
def test_render_views_with_full_rotations_match_the_replica(window, name):
    st = window
    sensor, pose, step = general_views(st.last["pose"], st.sen)[name]
    got = st.ctx.render_view(sensor, pose, step_voxels=step)
    mine = _replica(st, "ctx", sensor, pose, step)
    R = np.asarray(pose, np.float64)[:3, :3].astype(np.float32)
    print("%s: hit %d blocked %d none %d; samples %d of %d" % (name, mine["n_hit"], mine["n_blocked"], (mine["status"] == 0).sum(),
                                                              got["stats"]["n_samples_evaluated"], got["stats"]["n_samples_total"]))
    if name in ("own", "from_above"):
        assert mine["n_hit"] >= 1000, mine["n_hit"]
    if name != "on_axis_rolled":
        assert (R != 0).all()
    else:
        assert R[0, 2] == 1 and R[1, 2] == 0 and R[2, 2] == 0 and R[2, 0] != 0 and R[1, 1] != 0
    assert_same_images(got, mine, name + " / download_block")
    assert_same_images(got, _replica(st, "ora", sensor, pose, step), name + " / oracle")
    if name == "outside_in_rolled":
        assert mine["n_hit"] > 0
        assert got["stats"]["n_samples_evaluated"] < got["stats"]["n_samples_total"], got["stats"]
