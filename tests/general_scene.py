"""An analytic scene for the general camera (tests/general_camera.py): a tilted plane N . p = C and a sphere that rises 0.4 m out of it
towards the cameras, seen through the pinhole model written out here in float64.  The sphere's centre lies 0.5 m BEHIND the plane:
the visible cap ends in a crease on the plane, not in a limb.  A projective signed distance is only zero-on-the-surface where
rays are not tangent: just outside a limb a ray enters and leaves the sphere before it reaches a point that is millimetres from the
surface, and the point is given the chord length as a negative distance (with the centre 0.9 m in FRONT of the plane, 4 of 39 600
mesh vertices of eight fused frames sat 0.052 - 0.065 m off the sphere, all on its limb).  Half a voxel as a bound on the fused
surface is a statement about surfaces seen at bounded incidence, and the scene keeps to those.  Nothing in this file calls the oracle, the numpy restatement or the
library: it is the geometry the integrator is held to (tests/test_cpu_general_camera.py, tests/test_gpu_general_camera.py)."""
import numpy as np

from general_camera import GENERAL_INTRINSICS, general_trajectory

W, H = 160, 120
N_FRAMES = 8
MIN_RANGE, MAX_RANGE = 0.1, 5.0
# the plane: unit normal towards the cameras, through P0.  Not axis-aligned on any axis.
PLANE_N = np.array([0.36, -0.84, 0.40]) / np.linalg.norm([0.36, -0.84, 0.40])
PLANE_P0 = np.array([1.0, 3.2, 1.5])
PLANE_C = float(PLANE_N @ PLANE_P0)
SPHERE_R = 0.9
_T = np.array([-0.2, 0.0, -0.2])  # (towards the middle of the views)
SPHERE_C = PLANE_P0 + _T - (_T @ PLANE_N + 0.5) * PLANE_N  # 0.5 m behind the plane: a cap 0.4 m high, 1.5 m across


def pixel_rays(fx, fy, cx, cy, width=W, height=H):
    """the pinhole model: pixel (u, v) looks along (x, y, 1) = ((u - cx) / fx, (v - cy) / fy, 1) in the optical frame"""
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    return np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)


def depth_image(pose, fx, fy, cx, cy, width=W, height=H):
    """z-depth of the nearest surface along each pixel's ray, float64; 0 where the ray meets nothing in front of the camera.
    p(z) = c + z * Rw (x, y, 1): z is the depth because the optical-frame direction has z = 1."""
    T = np.asarray(pose, np.float64)
    Rw, c = T[:3, :3], T[:3, 3]
    d = pixel_rays(fx, fy, cx, cy, width, height) @ Rw.T
    with np.errstate(divide="ignore", invalid="ignore"):
        zp = (PLANE_C - PLANE_N @ c) / (d @ PLANE_N)
        zp = np.where(zp > 0, zp, np.inf)
        # |c + z d - S|^2 = r^2
        oc = c - SPHERE_C
        a, b, cc = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * cc
        zs = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        zs = np.where(zs > 0, zs, np.inf)
    z = np.minimum(zp, zs)
    return np.where(np.isfinite(z), z, 0.0)


def frames(n=N_FRAMES, width=W, height=H):
    """[(stamp ns, pose float64 4x4, depth float32 [H][W])] along general_trajectory at GENERAL_INTRINSICS"""
    fx, fy, cx, cy = GENERAL_INTRINSICS(width, height)
    out = []
    for i in range(n):
        pose = np.ascontiguousarray(general_trajectory(i))
        out.append((int(round((1.0 + 0.1 * i) * 1e9)), pose, depth_image(pose, fx, fy, cx, cy, width, height).astype(np.float32)))
    return out


def surface_distance(points):
    """distance of each point (n, 3) to the nearer of the two surfaces (the whole plane, the whole sphere), float64"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return np.minimum(np.abs(p @ PLANE_N - PLANE_C), np.abs(np.linalg.norm(p - SPHERE_C, axis=1) - SPHERE_R))
