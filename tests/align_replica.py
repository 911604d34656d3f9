"""numpy restatement of khr_align_linearize / khr_align_frame (ASSUMPTIONS.md A.14) over query_replica.query: vectorised over the
source points, every product formed and rounded on its own and summed with numpy's integer sum, so that it has nothing in common
with the kernel but the definition.  float32 where A.14 says float32, float64 where it says double."""
import numpy as np

import query_replica as qr

f32, f64 = np.float32, np.float64
N_WORDS, W_B, W_E, W_INLIER, W_GRADIENT, W_SOURCE, W_WEIGHT = 32, 21, 27, 28, 29, 30, 31
MAX_SOURCES = 1 << 20
MAX_GRAD_SQ, MAX_ARM, MAX_GATE = f32(16), f32(64), 64.0
H_PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]


def pose_f32(pose):
    T = np.asarray(pose, f64).reshape(4, 4)
    return T[:3, :3].astype(f32), T[:3, 3].astype(f32)


def depth_sources(depth, sensor, stride, weights=None):
    """the depth form's source points: (p_C (n, 3) float32, valid (n,), w (n,) float32) over the pixels (u, v) with u % stride ==
    v % stride == 0 in row-major order; p_C is A.2's, a pixel is valid under A.2's rule and within the sensor's range"""
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    vv, uu = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    u, v = uu.ravel(), vv.ravel()
    z = depth[v, u]
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (z > 0) & np.isfinite(z) & (z >= f32(sensor.min_range)) & (z <= f32(sensor.max_range))
        x = (u.astype(f32) - f32(sensor.cx)) / f32(sensor.fx)
        y = (v.astype(f32) - f32(sensor.cy)) / f32(sensor.fy)
        pc = np.stack([x * z, y * z, z], axis=1).astype(f32)
    w = np.ones(len(z), f32) if weights is None else np.asarray(weights, f32).reshape(H, W)[v, u]
    return pc, valid, w


def point_sources(points, weights=None):
    pc = np.ascontiguousarray(points, f32).reshape(-1, 3)
    w = np.ones(len(pc), f32) if weights is None else np.asarray(weights, f32).reshape(-1)
    return pc, np.ones(len(pc), bool), w


def transform(pc, pose):
    """p_W = ((r0*x + r1*y) + r2*z) + t in float32 (A.2's order): (p_W (n, 3), t)"""
    R, t = pose_f32(pose)
    with np.errstate(invalid="ignore", over="ignore"):
        pw = np.stack([((R[a, 0] * pc[:, 0] + R[a, 1] * pc[:, 1]) + R[a, 2] * pc[:, 2]) + t[a] for a in range(3)], axis=1)
    return pw.astype(f32), t


def terms(blocks, voxel_size, truncation_distance, pose, sources, min_weight, gate=0.0, huber_delta=0.0):
    """per source point: dict with inlier, has_gradient, valid masks, J (n, 6) float32, d, wr float32 (zero where no inlier) and
    T (n, 28) int64, the rounded products (H's 21, b's 6, e), S (n,) int64, the rounded w * rho"""
    pc, valid, w = sources
    pw, t = transform(pc, pose)
    q = qr.query(blocks, pw, voxel_size, min_weight)
    has_grad = valid & ((q["status"] & qr.QP_GRADIENT) != 0)
    d, g = q["distance"], q["gradient"]
    gate = f32(truncation_distance) if gate == 0 else f32(gate)
    hub = f32(huber_delta)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        arm = (pw - t[None, :]).astype(f32)
        ad = np.abs(d)
        gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        inlier = has_grad & (ad <= gate) & (gg <= MAX_GRAD_SQ) & (np.abs(arm) < MAX_ARM).all(axis=1) & (w > 0) & (w <= 1)
        rho = np.where((hub == 0) | (ad <= hub), f32(1), hub / ad).astype(f32)
        wr = np.where(inlier, w * rho, f32(0)).astype(f32)
        J = np.stack([arm[:, 1] * g[:, 2] - arm[:, 2] * g[:, 1], arm[:, 2] * g[:, 0] - arm[:, 0] * g[:, 2],
                      arm[:, 0] * g[:, 1] - arm[:, 1] * g[:, 0], g[:, 0], g[:, 1], g[:, 2]], axis=1).astype(f32)
    J = np.where(inlier[:, None], J, f32(0))
    d = np.where(inlier, d, f32(0))
    Jd, dd, wd = J.astype(f64), d.astype(f64), wr.astype(f64)

    def fixed(a, b):
        return np.rint(np.ldexp(wd * (a * b), 24)).astype(np.int64)

    T = np.stack([fixed(Jd[:, a], Jd[:, b]) for a, b in H_PAIRS] + [fixed(Jd[:, a], dd) for a in range(6)] + [fixed(dd, dd)], axis=1)
    S = np.rint(np.ldexp(wd, 24)).astype(np.int64)
    return dict(inlier=inlier, has_gradient=has_grad, valid=valid, J=J, d=d, wr=wr, T=T.reshape(-1, 28), S=S, pw=pw)


def words_of(tm):
    out = np.zeros(N_WORDS, np.uint64)
    out[:28] = tm["T"].astype(np.uint64).sum(axis=0, dtype=np.uint64)  # (two's complement, modulo 2^64)
    out[W_INLIER], out[W_GRADIENT], out[W_SOURCE] = int(tm["inlier"].sum()), int(tm["has_gradient"].sum()), int(tm["valid"].sum())
    out[W_WEIGHT] = tm["S"].astype(np.uint64).sum(dtype=np.uint64)
    return out


def linearize(blocks, voxel_size, truncation_distance, pose, points=None, depth=None, sensor=None, stride=1, weights=None,
              min_weight=1e-4, gate=0.0, huber_delta=0.0):
    """the 32 words of khr_align_linearize"""
    src = depth_sources(depth, sensor, stride, weights) if depth is not None else point_sources(points, weights)
    assert len(src[0]) <= MAX_SOURCES
    return words_of(terms(blocks, voxel_size, truncation_distance, pose, src, min_weight, gate, huber_delta))


def unpack(words):
    """(H (6, 6), b (6,), e, n_inlier) as float64 from the words"""
    v = np.asarray(words, np.uint64).view(np.int64).astype(f64) * 2.0 ** -24
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(H_PAIRS):
        H[a, b] = H[b, a] = v[k]
    return H, v[W_B:W_B + 6].copy(), float(v[W_E]), int(words[W_INLIER])


def cholesky_solve(A, rhs):
    """L L^T = A written out as khr_align_frame writes it; None at a pivot that is not positive"""
    L = np.zeros((6, 6))
    for j in range(6):
        s = A[j, j]
        for k in range(j):
            s -= L[j, k] * L[j, k]
        if not (s > 0.0) or not np.isfinite(s):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            v = A[j, i]
            for k in range(j):
                v -= L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    y, x = np.zeros(6), np.zeros(6)
    for i in range(6):
        v = rhs[i]
        for k in range(i):
            v -= L[i, k] * y[k]
        y[i] = v / L[i, i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k, i] * x[k]
        x[i] = v / L[i, i]
    return x


def apply_twist(pose, xi):
    """R <- exp(omega^) R, t <- t + v on a 4x4 float64 pose"""
    T = np.array(pose, f64).reshape(4, 4)
    w = xi[:3]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th < 1e-8:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.eye(3) + A * K + B * (K @ K)
    T[:3, :3] = E @ T[:3, :3]
    T[:3, 3] += xi[3:]
    return T


def gauss_newton(linearize_at, pose, max_iterations=10, min_inliers=64, lam=1e-4, eps_rot=1e-5, eps_trans=1e-5):
    """khr_align_frame's loop over `linearize_at(pose) -> words`: (ok, pose, log) with log = per linearisation dict(n_inlier, e,
    rmse, cond); ok False = KHR_ENOTFOUND (the pose returned is the input)"""
    T0 = np.array(pose, f64).reshape(4, 4)
    T = T0.copy()
    log = []
    converged = False
    for _ in range(max_iterations):
        words = linearize_at(T)
        H, b, e, n_in = unpack(words)
        sum_w = float(int(words[W_WEIGHT])) * 2.0 ** -24  # sum of w * rho over the inliers
        log.append(dict(n_inlier=n_in, e=e, rmse=float(np.sqrt(e / sum_w)) if sum_w > 0 else 0.0,
                        cond=float(np.linalg.cond(H)) if n_in else float("inf")))
        if n_in < max(min_inliers, 6):
            return False, T0, log, False
        xi = cholesky_solve(H + lam * np.diag(np.diag(H)), -b)
        if xi is None:
            return False, T0, log, False
        T = apply_twist(T, xi)
        if np.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) < eps_rot and np.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]) < eps_trans:
            converged = True
            break
    return True, T, log, converged


def pose_error(T, truth):
    """(rotation angle rad, translation distance m) between two 4x4 poses"""
    T, truth = np.asarray(T, f64).reshape(4, 4), np.asarray(truth, f64).reshape(4, 4)
    dR = T[:3, :3] @ truth[:3, :3].T
    return float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def perturbed(pose, rot_deg=1.0, trans_m=0.03):
    """the true pose moved by a fixed twist of about rot_deg and trans_m (deterministic)"""
    axis = np.array([0.5, -0.7, 0.5])
    axis /= np.linalg.norm(axis)
    v = np.array([0.6, 0.5, -0.62])
    v /= np.linalg.norm(v)
    return apply_twist(pose, np.concatenate([axis * np.deg2rad(rot_deg), v * trans_m]))
