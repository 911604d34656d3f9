"""khr_align_linearize / khr_align_frame (ASSUMPTIONS.md A.14): the 32 words of a linearisation held bit for bit to
tests/align_replica.py over this context's block downloads and over the CPU oracle's blocks, on the stream and the point sets of
the khr_query_points tests; the Gauss-Newton loop held to the replica's loop; errors, guards and the read-only contract."""
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import align_replica as ar
from common import DeviceArray, make_pair
from khronos_amd import FusionContext, default_config
from khronos_amd.capi import KHR_EINVAL, KHR_ENOTFOUND, KHR_ESTATE, KHR_ALIGN_WORDS
from test_gpu_query_points import blocks_of, point_sets, run_stream, stream  # noqa: F401  (the module-scoped 30-frame stream)
from test_gpu_render_view import YAML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "khronos_amd", "lib", "aw_demo")

f32 = np.float32
GUARD = 64
IDENTITY = np.eye(4)


def expect(st, which, pose, **kw):
    kw.setdefault("min_weight", st.cfg.mesh_min_weight)
    if kw["min_weight"] == 0:
        kw["min_weight"] = st.cfg.mesh_min_weight
    return ar.linearize(blocks_of(st, which), st.cfg.voxel_size, st.cfg.truncation_distance, pose, **kw)


def check(st, what, pose, device=False, oracle=True, **kw):
    """the kernel's words for the request == the replica's over this context's blocks and over the oracle's; returns them"""
    if device:
        dev = {k: DeviceArray(np.ascontiguousarray(kw[k], f32)) for k in ("points", "depth", "weights") if kw.get(k) is not None}
        dkw = dict(kw)
        dkw.update({k: d.data_ptr() for k, d in dev.items()})
        if "points" in dev:
            dkw["n"] = len(np.asarray(kw["points"]).reshape(-1, 3))
        got = st.ctx.align_linearize(pose, device=True, **dkw)
        for d in dev.values():
            d.free()
    else:
        got = st.ctx.align_linearize(pose, **kw)
    assert got.dtype == np.uint64 and got.shape == (KHR_ALIGN_WORDS,)
    for which in ("ctx", "ora") if oracle else ("ctx",):
        want = expect(st, which, pose, **kw)
        assert np.array_equal(got, want), (what, which, np.flatnonzero(got != want).tolist(), got[27:31].tolist(), want[27:31].tolist())
    return got


def last_frame(st):
    """(depth, sensor, true pose, perturbed pose, camera points of the valid pixels)"""
    if "align" not in st.cache:
        truth = np.asarray(st.last["pose"], np.float64).reshape(4, 4)
        pc, valid, _ = ar.depth_sources(st.last["depth"], st.sen, 1)
        st.cache["align"] = (np.asarray(st.last["depth"], f32), st.sen, truth, ar.perturbed(truth), pc[valid])
    return st.cache["align"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["surface", "lattice", "bad", "mixed"])
def test_point_sets_under_the_identity_pose(stream, name):
    st = stream
    pts = point_sets(st)[name]
    w = check(st, name, IDENTITY, points=pts)
    print("%s: %d points, gradient %d, inliers %d" % (name, len(pts), w[ar.W_GRADIENT], w[ar.W_INLIER]))
    assert w[ar.W_SOURCE] == len(pts)
    if name == "bad":
        assert not w[:30].any() and w[ar.W_WEIGHT] == 0
    else:
        assert w[ar.W_INLIER] > 0 and w[0] > 0 and int(w[ar.W_WEIGHT]) == int(w[ar.W_INLIER]) << 24  # (unit weights, no Huber factor)
    if name == "mixed":  # another shuffle: identical words
        again = st.ctx.align_linearize(IDENTITY, points=pts[np.random.default_rng(99).permutation(len(pts))])
        assert np.array_equal(again, w)


@pytest.mark.gpu
@pytest.mark.parametrize("which_pose", ["true", "perturbed"])
def test_camera_points_of_the_last_frame(stream, which_pose):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    w = check(st, which_pose, truth if which_pose == "true" else start, points=pc)
    print("%s pose: %d sources, %d inliers" % (which_pose, w[ar.W_SOURCE], w[ar.W_INLIER]))
    assert 4 * int(w[ar.W_INLIER]) >= len(pc)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 3, 4])
def test_depth_form(stream, stride):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    for pose in (truth, start):
        w = check(st, "stride %d" % stride, pose, depth=depth, sensor=sen, stride=stride)
        assert 4 * int(w[ar.W_INLIER]) >= int(w[ar.W_SOURCE]) > 0
    if stride == 4:  # a stride past the image leaves pixel (0, 0) alone, also where width + stride passes 2^31
        for huge in (320, 2 ** 31 - 1):
            assert check(st, "stride %d" % huge, truth, depth=depth, sensor=sen, stride=huge)[ar.W_SOURCE] == 1
    if stride == 1:
        # the frame's own pose: every pixel the frame path accepts and the sensor's range admits is a source, its p_W is the
        # slot's vertex map bit for bit, and the point form fed the same p_C gives the same words.  (The vertex map transformed
        # back through the float pose does not return p_C exactly -- a rotation in float32 is not invertible to the bit -- so the
        # point form is fed the replica's p_C, and the forward transform is what is compared with the vertex map.)
        w = st.ctx.align_linearize(truth, depth=depth, sensor=sen, stride=1)
        in_range = (depth > 0) & np.isfinite(depth) & (depth >= f32(sen.min_range)) & (depth <= f32(sen.max_range))
        assert int(w[ar.W_SOURCE]) == int(in_range.sum()) > 0
        vmap = np.asarray(st.ctx.download_frame(st.last["step"]["slot"], depth.shape, range_image=False, vertex_map=True)[1], f32).reshape(-1, 3)
        assert ar.transform(pc, truth)[0].tobytes() == vmap[in_range.ravel()].tobytes()
        assert np.array_equal(st.ctx.align_linearize(truth, points=pc), w)


@pytest.mark.gpu
def test_batch_sizes_cover_the_wave_and_workgroup_tails(stream):
    st = stream
    pts = point_sets(st)["surface"][::5]
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        w = check(st, "n = %d" % n, IDENTITY, points=pts[:n])
        assert int(w[ar.W_SOURCE]) == n
        if n == 0:
            assert not w.any()
    assert check(st, "n = 257", IDENTITY, points=pts[:257])[ar.W_GRADIENT] > 0


@pytest.mark.gpu
def test_weights_huber_gate_and_min_weight(stream):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    pc = pc[::3]
    rng = np.random.default_rng(8)
    wts = rng.uniform(0.01, 1.0, len(pc)).astype(f32)
    special = np.array([0.0, -0.5, np.nan, 1.0, 1.5, np.inf, 1e-30, -0.0], f32)
    wts[: 8 * (len(wts) // 8)].reshape(-1, 8)[:, 0] = np.resize(special, len(wts) // 8)
    plain = check(st, "no weights", start, points=pc)
    weighted = check(st, "weights", start, points=pc, weights=wts)
    assert 0 < weighted[ar.W_INLIER] < plain[ar.W_INLIER] and weighted[ar.W_GRADIENT] == plain[ar.W_GRADIENT]
    hub = check(st, "huber", start, points=pc, huber_delta=0.05)
    assert hub[ar.W_INLIER] == plain[ar.W_INLIER] and hub[ar.W_E] < plain[ar.W_E]
    check(st, "huber + weights", start, points=pc, weights=wts, huber_delta=0.05)
    tight = check(st, "gate", start, points=pc, gate=0.04)
    assert 0 < tight[ar.W_INLIER] < plain[ar.W_INLIER]
    heavy = check(st, "min_weight", start, points=pc, min_weight=3.0)
    assert heavy[ar.W_GRADIENT] != plain[ar.W_GRADIENT]
    # the depth form indexes the weights by pixel
    wimg = rng.uniform(0.01, 1.0, depth.shape).astype(f32)
    wimg[::5, ::3] = 0
    check(st, "depth weights", start, depth=depth, sensor=sen, stride=3, weights=wimg, huber_delta=0.05)


@pytest.mark.gpu
def test_device_form_equals_the_host_form(stream):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    wts = np.random.default_rng(2).uniform(0.0, 1.2, len(pc)).astype(f32)
    host = st.ctx.align_linearize(start, points=pc, weights=wts, huber_delta=0.05)
    assert np.array_equal(check(st, "device points", start, device=True, points=pc, weights=wts, huber_delta=0.05), host)
    host = st.ctx.align_linearize(start, depth=depth, sensor=sen, stride=3)
    assert np.array_equal(check(st, "device depth", start, device=True, depth=depth, sensor=sen, stride=3), host)
    wimg = np.random.default_rng(4).uniform(0.0, 1.0, depth.shape).astype(f32)
    check(st, "device depth weights", truth, device=True, depth=depth, sensor=sen, stride=4, weights=wimg)


@pytest.mark.gpu
def test_8vps_object_map_without_tracking():
    """the object mini-map configuration of tests/test_gpu_query_points.py (vps 8, binary labels, no tracking)"""
    cfg, ctx, ora, s, sen, osen = make_pair(voxels_per_side=8, voxel_size=0.04, truncation_distance=0.08, with_tracking=0, semantic_mode=1,
                                            num_labels=2)
    st = SimpleNamespace(cfg=cfg, ctx=ctx, ora=ora, s=s, sen=sen, osen=osen, last=None, cache={})
    fr0 = s.render(0)
    bl = np.array([[x, y, z] for x in range(2, 8) for y in range(-3, 3) for z in range(0, 6)], np.int32)
    ctx.allocate_blocks(bl)
    ora.allocate_blocks(bl)
    for i in range(4):
        fr = s.render(i)
        obj = (fr["label"] == fr0["label"][120, 160]).astype(np.int32) * 3
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], None)
        ctx.set_frame_image(slot, 1, obj)
        ctx.integrate(slot, allocate_blocks=False, use_mask=False, object_id=3)
        ora.integrate(osen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], None, object_image=obj, object_id=3, allocate_blocks=False)
        st.last = fr
    sets = point_sets(st)
    for name in ("lattice", "mixed"):
        w = check(st, "8^3 " + name, IDENTITY, points=sets[name], huber_delta=0.02)
        assert w[ar.W_INLIER] > 0
    truth = np.asarray(st.last["pose"], np.float64).reshape(4, 4)
    w = check(st, "8^3 depth", ar.perturbed(truth, 0.3, 0.01), depth=np.asarray(st.last["depth"], f32), sensor=sen, stride=3)
    print("8^3 depth: %d sources, %d gradient, %d inliers" % (w[ar.W_SOURCE], w[ar.W_GRADIENT], w[ar.W_INLIER]))
    assert w[ar.W_SOURCE] > 0  # (the box need not hold the frame's surface: the point sets above carry the inliers)
    ctx.close()


@pytest.mark.gpu
def test_without_tracking_and_semantics():
    st = run_stream(n_frames=6, archive_every=0, with_tracking=0, with_semantics=0)
    depth, sen, truth, start, pc = last_frame(st)
    w = check(st, "no tracking, no semantics", start, depth=depth, sensor=sen, stride=2)
    assert w[ar.W_INLIER] > 1000
    check(st, "no tracking, no semantics / mixed", IDENTITY, points=point_sets(st)["mixed"][::4])
    st.ctx.close()


@pytest.mark.gpu
def test_align_depth_follows_the_replica_loop(stream):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    r0, t0 = ar.pose_error(start, truth)
    ok, want, log, conv = ar.gauss_newton(lambda T: expect(st, "ctx", T, depth=depth, sensor=sen, stride=4), start)
    rr, tr = ar.pose_error(want, truth)
    pose, res = st.ctx.align_depth(depth, sen, start, stride=4)
    rg, tg = ar.pose_error(pose, truth)
    print("start %.5f rad %.5f m; replica %.5f rad %.5f m in %d linearisations; device %.5f rad %.5f m in %d (converged %s, inliers %d -> %d, "
          "rmse %.5f -> %.5f)" % (r0, t0, rr, tr, len(log), rg, tg, res["iterations"], res["converged"], res["n_inlier_first"],
                                  res["n_inlier_last"], res["rmse_first"], res["rmse_last"]))
    assert ok and res["found"] and rr < r0 and tr < t0
    assert rg <= rr * 1.1 + 1e-6 and tg <= tr * 1.1 + 1e-6
    assert abs(res["iterations"] - len(log)) <= 1
    assert res["n_inlier_first"] == log[0]["n_inlier"] and abs(res["rmse_first"] - log[0]["rmse"]) <= 1e-12
    # rmse = sqrt(e / sum of w rho): halving every weight halves both sums (up to the rounding of the fixed-point terms)
    half = np.full(depth.shape, 0.5, f32)
    rq, keep = st.ctx.align_request(start, depth=depth, sensor=sen, stride=4, weights=half, huber_delta=0.05)
    rc, res_half = st.ctx.align_frame_into(rq, np.zeros(16), max_iterations=1)
    rq, keep = st.ctx.align_request(start, depth=depth, sensor=sen, stride=4, huber_delta=0.05)
    rc1, res_one = st.ctx.align_frame_into(rq, np.zeros(16), max_iterations=1)
    w_h = expect(st, "ctx", start, depth=depth, sensor=sen, stride=4, huber_delta=0.05)
    want = np.sqrt(float(int(w_h[ar.W_E])) / float(int(w_h[ar.W_WEIGHT])))
    # (each of the n fixed-point terms of e is rounded by at most 2^-25, each term of the weight sum by a relative 2^-24)
    e_half = 0.5 * float(int(w_h[ar.W_E])) * 2.0 ** -24
    tol = 2 * int(w_h[ar.W_INLIER]) * 2.0 ** -25 / e_half + 2.0 ** -20
    print("rmse %.9f, with every weight halved %.9f, relative tolerance %.2e" % (res_one["rmse_first"], res_half["rmse_first"], tol))
    assert rc == 0 and rc1 == 0 and abs(res_one["rmse_first"] - want) <= 1e-12 and abs(res_half["rmse_first"] - want) <= tol * want
    assert int(w_h[ar.W_WEIGHT]) < int(w_h[ar.W_INLIER]) << 24  # (the Huber factor is at work)
    at = st.ctx.align_linearize(pose, depth=depth, sensor=sen, stride=4)
    assert np.array_equal(at, expect(st, "ctx", pose, depth=depth, sensor=sen, stride=4))
    assert np.array_equal(at, expect(st, "ora", pose, depth=depth, sensor=sen, stride=4))
    # the last linearisation's H and b as doubles: those of the words at the pose before the last update -- symmetric positive H
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(ar.H_PAIRS):
        H[a, b] = H[b, a] = res["H"][k]
    assert np.linalg.eigvalsh(H).min() > 0 and np.isfinite(res["b"]).all()
    # the point form of the same frame, on the device
    d_pc = DeviceArray(pc[::4])
    pose_p, res_p = st.ctx.align_points(d_pc.data_ptr(), start, device=True, n=len(pc[::4]))
    d_pc.free()
    rp, tp = ar.pose_error(pose_p, truth)
    assert res_p["found"] and rp < r0 and tp < t0


@pytest.mark.gpu
def test_nothing_to_align_against_keeps_the_prior(stream):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    away = start.copy()
    away[:3, 3] += [300.0, -200.0, 100.0]  # looking at nothing
    pose, res = st.ctx.align_depth(depth, sen, away, stride=4)
    assert not res["found"] and np.array_equal(pose, away) and res["iterations"] == 0 and res["n_inlier_first"] == 0
    rq, keep = st.ctx.align_request(away, depth=depth, sensor=sen, stride=4)
    out = np.full(16 + GUARD, 7.0)
    rc, res = st.ctx.align_frame_into(rq, out)
    assert rc == KHR_ENOTFOUND and np.array_equal(out[:16].reshape(4, 4), away) and (out[16:] == 7).all()
    # an empty map
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=320 * 240)
    empty = FusionContext(cfg)
    pose, res = empty.align_depth(depth, sen, start, stride=4)
    assert not res["found"] and np.array_equal(pose, start)
    w = empty.align_linearize(start, depth=depth, sensor=sen, stride=4)
    assert w[ar.W_SOURCE] > 0 and not w[:30].any() and w[ar.W_WEIGHT] == 0
    empty.close()


@pytest.mark.gpu
def test_error_codes_leave_the_buffers_untouched(stream):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    pc = pc[:100]
    nan_pose = truth.copy()
    nan_pose[1, 3] = np.nan
    inf_pose = truth.copy()
    inf_pose[0, 0] = np.inf
    big = np.zeros((1025, 1025), f32)  # 1025^2 > 2^20 sources at stride 1
    big_sen = st.ctx.make_sensor(1025, 1025, 500.0, 500.0, 512.0, 512.0)
    cases = {
        "nan pose": dict(pose=nan_pose, points=pc), "inf pose": dict(pose=inf_pose, points=pc),
        "stride 0": dict(pose=truth, depth=depth, sensor=sen, stride=0), "stride -1": dict(pose=truth, depth=depth, sensor=sen, stride=-1),
        "negative gate": dict(pose=truth, points=pc, gate=-0.1), "nan gate": dict(pose=truth, points=pc, gate=float("nan")),
        "inf gate": dict(pose=truth, points=pc, gate=float("inf")), "gate above 64 m": dict(pose=truth, points=pc, gate=65.0),
        "negative huber": dict(pose=truth, points=pc, huber_delta=-1.0), "nan huber": dict(pose=truth, points=pc, huber_delta=float("nan")),
        "negative min_weight": dict(pose=truth, points=pc, min_weight=-1.0), "inf min_weight": dict(pose=truth, points=pc, min_weight=float("inf")),
        "too many pixels": dict(pose=truth, depth=big, sensor=big_sen, stride=1),
        "too many points": dict(pose=truth, points=np.zeros(((1 << 20) + 1, 3), f32)),
        "negative n": dict(pose=truth, points=pc, n=-1), "no source": dict(pose=truth, n=5),
        "both sources": dict(pose=truth, points=pc, depth=depth, sensor=sen),
    }
    for what, kw in cases.items():
        rq, keep = st.ctx.align_request(kw.pop("pose"), **kw)
        words = np.full(KHR_ALIGN_WORDS + GUARD, 7, np.uint64)
        assert st.ctx.align_linearize_into(rq, words) == KHR_EINVAL, what
        assert (words == 7).all(), what
        out = np.full(16 + GUARD, 7.0)
        rc, res = st.ctx.align_frame_into(rq, out)
        assert rc == KHR_EINVAL and (out == 7).all(), what
    words = np.full(KHR_ALIGN_WORDS + GUARD, 7, np.uint64)
    assert st.ctx.align_linearize_into(None, words) == KHR_EINVAL and (words == 7).all()
    rq, keep = st.ctx.align_request(truth, points=pc)
    assert st.ctx.align_linearize_into(rq, None) == KHR_EINVAL
    # khr_align_frame: a NULL request, a NULL output pose
    out = np.full(16 + GUARD, 7.0)
    rc, res = st.ctx.align_frame_into(None, out)
    assert rc == KHR_EINVAL and (out == 7).all() and res["iterations"] == 0 and res["n_inlier_first"] == 0
    rc, res = st.ctx.align_frame_into(rq, None)
    assert rc == KHR_EINVAL and res["iterations"] == 0 and res["n_inlier_first"] == 0
    # the binding: a device point list has no length of its own
    with pytest.raises(ValueError):
        st.ctx.align_request(truth, points=0x1000, device=True)
    with pytest.raises(ValueError):
        st.ctx.align_points(0x1000, truth, device=True)
    # 2^20 pixels exactly is allowed: 1024 x 1024 at stride 1, 2048 x 2048 at stride 2 (an empty image: no source)
    ok_sen = st.ctx.make_sensor(1024, 1024, 500.0, 500.0, 512.0, 512.0)
    w = st.ctx.align_linearize(truth, depth=np.zeros((1024, 1024), f32), sensor=ok_sen, stride=1)
    assert not w.any()
    # n == 0: fine, zero words, the guard untouched
    words = np.full(KHR_ALIGN_WORDS + GUARD, 7, np.uint64)
    rq, keep = st.ctx.align_request(truth, n=0)
    assert st.ctx.align_linearize_into(rq, words) == 0 and not words[:KHR_ALIGN_WORDS].any() and (words[KHR_ALIGN_WORDS:] == 7).all()
    # a valid call writes 32 words and nothing behind them
    rq, keep = st.ctx.align_request(truth, points=pc)
    assert st.ctx.align_linearize_into(rq, words) == 0 and words[ar.W_SOURCE] == len(pc) and (words[KHR_ALIGN_WORDS:] == 7).all()
    # a shard cannot answer
    cfg = default_config(voxel_size=0.1, truncation_distance=0.3, max_blocks=256, max_frame_pixels=64 * 48, rank=0, world_size=2)
    shard = FusionContext(cfg)
    words = np.full(KHR_ALIGN_WORDS + GUARD, 7, np.uint64)
    rq, keep = shard.align_request(truth, points=pc)
    assert shard.align_linearize_into(rq, words) == KHR_ESTATE and (words == 7).all()
    out = np.full(16 + GUARD, 7.0)
    rc, res = shard.align_frame_into(rq, out)
    assert rc == KHR_ESTATE and (out == 7).all()
    shard.close()


@pytest.mark.gpu
def test_the_calls_only_read_the_map(stream):
    st = stream
    depth, sen, truth, start, pc = last_frame(st)
    digest, idx, stats = st.ctx.map_digest(), st.ctx.block_indices().copy(), st.ctx.stats()
    a = st.ctx.align_linearize(start, depth=depth, sensor=sen, stride=2, huber_delta=0.05)
    b = st.ctx.align_linearize(start, depth=depth, sensor=sen, stride=2, huber_delta=0.05)
    assert np.array_equal(a, b)
    st.ctx.align_depth(depth, sen, start, stride=4)
    st.ctx.align_points(pc[::4], start)
    assert np.array_equal(st.ctx.map_digest(), digest)
    assert np.array_equal(st.ctx.block_indices(), idx)
    assert st.ctx.stats() == stats


@pytest.mark.gpu
def test_aw_demo_align_mode_equals_the_python_path(tmp_path):
    """aw_demo --align: a Khronos sink perturbs the last frame's pose by about 1 degree and 3 cm and lets the map pull it back through
    hydra::VolumetricMap::align -- the converted frame, the raw depth image and the point list overloads, which the demo holds to one
    another bit for bit.  The same stream stepped through the C ABI as ActiveWindow::spinOnce steps it, registered from the demo's
    prior by FusionContext.align_depth, gives the same pose and counters to the bit (one library, integer sums)."""
    W, H, N = 320, 240, 14
    cfgp = tmp_path / "aw_align.yaml"
    cfgp.write_text(YAML)
    out = subprocess.run([DEMO, "--align", str(cfgp), str(W), str(H), str(N), "4"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout.strip().splitlines()[-1])
    assert res["frames"] == N and res["stride"] == 4 and res["found"] and res["depth_form_equal"] and res["point_form_equal"]
    truth, prior, got = (np.array(res[k], np.float64).reshape(4, 4) for k in ("truth", "prior", "pose"))
    r0, t0 = ar.pose_error(prior, truth)
    r1, t1 = ar.pose_error(got, truth)
    assert 0.017 < r0 < 0.018 and 0.028 < t0 < 0.030 and r1 < r0 and t1 < t0
    assert abs(res["rot_error"] - r1) <= 1e-9 and abs(res["trans_error"] - t1) <= 1e-9
    cfg, ctx, ora, s, sen, osen = make_pair(width=W, height=H, temporal_window=0.75, truncation_distance=0.3,
                                            md_min_cluster_size=20, md_min_separation_distance=2.0, md_max_range=5.0)
    last_full, mine = 0, None
    for i in range(N):
        fr = s.render(i)
        slot = ctx.upload_frame(sen, fr["stamp"], fr["pose"], fr["depth"], fr["rgb"], fr["label"])
        ctx.detect_motion(slot)
        ctx.integrate(slot, allocate_blocks=True, use_mask=True)
        ctx.update_tracking(fr["stamp"])
        if i == N - 1:  # the sinks run before the frame's output and its archival
            assert np.allclose(np.asarray(fr["pose"], np.float64).reshape(4, 4), truth, rtol=0, atol=1e-12)
            mine = ctx.align_depth(fr["depth"], sen, prior, stride=4)
            n_points = int(ar.depth_sources(fr["depth"], sen, 4)[1].sum())
        if not (last_full + int(float(np.float32(0.4)) * 1e9) > fr["stamp"]):
            ctx.generate_mesh(True, True)
            ctx.reset_inactive()
            ctx.clear_updated()
            last_full = fr["stamp"]
    pose, r = mine
    ctx.close()
    assert r["found"] and np.array_equal(pose, got)
    assert (r["iterations"], r["converged"], r["n_inlier_first"], r["n_inlier_last"]) == \
        (res["iterations"], res["converged"], res["n_inlier_first"], res["n_inlier_last"])
    assert r["rmse_first"] == res["rmse_first"] and r["rmse_last"] == res["rmse_last"] and res["n_points"] == n_points
