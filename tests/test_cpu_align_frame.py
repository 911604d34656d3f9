"""-m "not gpu": the definition of khr_align_linearize / khr_align_frame (ASSUMPTIONS.md A.14) as tests/align_replica.py restates it,
run over the CPU oracle's map of tests/test_cpu_query_points.py's stream (320x240, 10 cm, 30 frames): the properties the kernel's
reduction relies on (order and split invariance, the no-wrap bound), the consistency of H, b and e, and that the inputs the GPU
test compares on are not vacuous."""
import os

import numpy as np
import pytest

import align_replica as ar
from khronos_amd import capi
from test_cpu_query_points import world  # noqa: F401  (the module-scoped oracle stream of the query tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def scene(world):  # noqa: F811
    cfg, fr, sen = world["cfg"], world["frame"], world["sensor"]
    truth = np.asarray(fr["pose"], np.float64).reshape(4, 4)
    kw = dict(blocks=world["blocks"], voxel_size=cfg.voxel_size, truncation_distance=cfg.truncation_distance, min_weight=cfg.mesh_min_weight)

    def lin(pose, stride=4, **more):
        a = dict(kw)
        a.update(more)
        return ar.linearize(a.pop("blocks"), a.pop("voxel_size"), a.pop("truncation_distance"), pose, depth=fr["depth"], sensor=sen, stride=stride, **a)

    def tm(pose, stride=4, gate=0.0, huber_delta=0.0):
        return ar.terms(world["blocks"], cfg.voxel_size, cfg.truncation_distance, pose, ar.depth_sources(fr["depth"], sen, stride),
                        cfg.mesh_min_weight, gate, huber_delta)

    return dict(cfg=cfg, frame=fr, sensor=sen, truth=truth, start=ar.perturbed(truth), lin=lin, terms=tm, blocks=world["blocks"])


def test_words_do_not_depend_on_order_or_split(scene):
    cfg, fr, sen = scene["cfg"], scene["frame"], scene["sensor"]
    pc, valid, w = ar.depth_sources(fr["depth"], sen, 4)
    pc = pc[valid]
    rng = np.random.default_rng(3)
    wts = rng.uniform(0.05, 1.0, len(pc)).astype(f32)

    def words(p, ww):
        return ar.linearize(scene["blocks"], cfg.voxel_size, cfg.truncation_distance, scene["start"], points=p, weights=ww,
                            min_weight=cfg.mesh_min_weight, huber_delta=0.05)

    whole = words(pc, wts)
    assert whole[ar.W_INLIER] > 1000 and whole[ar.W_SOURCE] == len(pc) and 0 < whole[ar.W_WEIGHT] < int(whole[ar.W_INLIER]) << 24
    perm = rng.permutation(len(pc))
    assert np.array_equal(words(pc[perm], wts[perm]), whole)
    k = len(pc) // 3
    with np.errstate(over="ignore"):
        assert np.array_equal(words(pc[:k], wts[:k]) + words(pc[k:], wts[k:]), whole)


def test_largest_term_is_below_the_bound_of_A14(scene):
    """A.14: |term| < 2^43, so 2^20 sources cannot wrap a 64-bit sum.  On these inputs the terms are far smaller."""
    worst = 0
    for pose in (scene["truth"], scene["start"]):
        for stride in (1, 4):
            t = scene["terms"](pose, stride)
            worst = max(worst, int(np.abs(t["T"]).max()))
            assert np.abs(t["J"]).max() <= 512 and np.abs(t["d"]).max() <= scene["cfg"].truncation_distance
    print("largest |term| = %d = 2^%.1f" % (worst, np.log2(worst)))
    assert 0 < worst < 2 ** 43


def test_inputs_are_not_vacuous_at_the_true_pose(scene):
    w = scene["lin"](scene["truth"], stride=4)
    n_in, n_src = int(w[ar.W_INLIER]), int(w[ar.W_SOURCE])
    print("true pose, stride 4: %d sources, %d with gradient, %d inliers" % (n_src, int(w[ar.W_GRADIENT]), n_in))
    assert n_src > 1000 and 4 * n_in >= n_src
    assert int(w[ar.W_GRADIENT]) >= n_in
    assert int(w[ar.W_WEIGHT]) == n_in << 24  # unit weights, no Huber factor: the sum of w rho is the inlier count


def test_H_and_b_predict_the_change_of_e_under_a_small_twist(scene):
    """With the inlier set and the Huber factors held fixed, e(xi) = sum w rho (d + J xi)^2 to first order in the residual, so
    e(xi) - e(0) = 2 b.xi + xi^T H xi up to the curvature of the interpolated distance.  Checked per axis with twists of 1e-3 (rad,
    m) at the perturbed pose on the points that are inliers at both poses (the fixed-point words of that subset).  Measured on the
    replica (stride 2), the relative deviation |actual - predicted| / (|2 b.xi| + xi^T H xi), the larger of both signs, per axis
    (omega_x, omega_y, omega_z, v_x, v_y, v_z): 0.067, 0.024, 0.090, 0.013, 0.184, 0.026 -- the largest along the translation axis
    whose predicted change is the smallest (trilinear interpolation is only piecewise smooth and the gradient is a central
    difference over two 10 cm voxels).  Each axis is held to its own figure times a margin of 1.36, rounded up to three places:
    0.092, 0.033, 0.123, 0.018, 0.251, 0.036.  A sign error or a missing factor 2 in b or H gives a deviation of 1 or more on every
    axis; a scale error of 10 % in one component of b moves that axis' deviation by about 0.1, which four of the six bounds catch."""
    cfg, fr, sen = scene["cfg"], scene["frame"], scene["sensor"]
    base = scene["start"]
    pc, valid, _ = ar.depth_sources(fr["depth"], sen, 2)
    pc = pc[valid]

    def t_at(pose, pts):
        return ar.terms(scene["blocks"], cfg.voxel_size, cfg.truncation_distance, pose, ar.point_sources(pts), cfg.mesh_min_weight)

    t0 = t_at(base, pc)
    bound = [0.092, 0.033, 0.123, 0.018, 0.251, 0.036]
    worst = [0.0] * 6
    for axis in range(6):
        for sgn in (1.0, -1.0):
            xi = np.zeros(6)
            xi[axis] = sgn * 1e-3
            t1 = t_at(ar.apply_twist(base, xi), pc)
            both = t0["inlier"] & t1["inlier"]
            assert both.sum() > 1000
            H, b, e0, _ = ar.unpack(ar.words_of(t_at(base, pc[both])))
            e1 = ar.unpack(ar.words_of(t_at(ar.apply_twist(base, xi), pc[both])))[2]
            pred = 2.0 * b @ xi + xi @ H @ xi
            dev = abs((e1 - e0) - pred) / (abs(2.0 * b @ xi) + xi @ H @ xi)
            print("axis %d sign %+d: e %.6f -> %.6f, predicted change %.3e, actual %.3e, deviation %.3f" % (axis, sgn, e0, e1, pred, e1 - e0, dev))
            worst[axis] = max(worst[axis], dev)
    print("largest relative deviation per axis " + ", ".join("%.3f" % w for w in worst))
    for axis in range(6):
        assert worst[axis] < bound[axis], (axis, worst[axis], bound[axis])


def test_the_loop_reduces_the_pose_error(scene):
    """from the true pose perturbed by about 1 degree and 3 cm, gate = the truncation distance"""
    truth, start = scene["truth"], scene["start"]
    r0, t0 = ar.pose_error(start, truth)
    ok, pose, log, converged = ar.gauss_newton(lambda T: scene["lin"](T, stride=4), start)
    r1, t1 = ar.pose_error(pose, truth)
    print("start: %.4f rad %.4f m; end: %.4f rad %.4f m after %d linearisations (converged %s)" % (r0, t0, r1, t1, len(log), converged))
    for k, it in enumerate(log):
        print("  %d: inliers %d, e %.5f, rmse %.5f, cond(H) %.3g" % (k, it["n_inlier"], it["e"], it["rmse"], it["cond"]))
    assert ok and 0.015 < r0 < 0.02 and 0.029 < t0 < 0.031
    assert max(it["cond"] for it in log) < 1e6  # (every direction is constrained: the assertion is on the pose, not on e alone)
    assert r1 < r0 and t1 < t0
    assert log[-1]["rmse"] < log[0]["rmse"]


def test_cholesky_and_twist_are_what_they_claim():
    rng = np.random.default_rng(0)
    M = rng.normal(size=(6, 6))
    A, rhs = M @ M.T + 6 * np.eye(6), rng.normal(size=6)
    assert np.allclose(ar.cholesky_solve(A, rhs), np.linalg.solve(A, rhs), rtol=1e-12, atol=1e-12)
    assert ar.cholesky_solve(np.diag([1.0, 1, 1, 0, 1, 1]), rhs) is None
    T = ar.apply_twist(np.eye(4), np.array([0, 0, np.pi / 2, 1, 2, 3]))
    assert np.allclose(T[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15) and np.allclose(T[:3, 3], [1, 2, 3])
    T = ar.apply_twist(T, np.array([1e-10, 0, 0, 0, 0, 0]))
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-15)


def test_binding_and_header():
    assert "khr_align_linearize" in capi.EXPORTS and "khr_align_frame" in capi.EXPORTS
    lib = capi.load_library()
    assert len(lib.khr_align_linearize.argtypes) == 4 and len(lib.khr_align_frame.argtypes) == 6
    assert (capi.KHR_ALIGN_WORDS, capi.KHR_ALIGN_MAX_SOURCES) == (ar.N_WORDS, ar.MAX_SOURCES)
    text = open(os.path.join(ROOT, "include", "khronos_amd.h")).read()
    for word in ("khr_align_request", "khr_align_options", "khr_align_result", "#define KHR_ALIGN_WORDS 32",
                 "int khr_align_linearize(khr_ctx* ctx, const khr_align_request* request, int on_device, uint64_t* words);"):
        assert word in text, word
    for name in ("align_linearize", "align_points", "align_depth"):
        assert callable(getattr(capi.FusionContext, name))
