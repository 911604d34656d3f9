"""-m "not gpu": the definition of khr_render_view (ASSUMPTIONS.md A.12) as tests/render_replica.py restates it, on a hand-built
map with an analytic answer -- a plane whose signed distance is a linear function, so trilinear interpolation reproduces it up to
rounding -- and the presence of the C ABI symbol and its Python wrapper."""
import os
from types import SimpleNamespace

import numpy as np

import render_replica as rr
from khronos_amd import capi
from khronos_amd.synth import camera_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VPS, VS = 8, 0.1
VS32 = float(np.float32(VS))  # the voxel size the float32 arithmetic sees
# the surface: d(p) = N . (p - P0) with the unit gradient N, positive on the side the camera looks from
N = np.array([-0.96, -0.28, 0.0])
P0 = np.array([1.5, 0.0, 0.0])
BLOCKS = [(bx, by, bz) for bx in range(0, 3) for by in (-1, 0) for bz in (-1, 0)]  # x in [0, 2.4), y, z in [-0.8, 0.8)
SENSOR = SimpleNamespace(width=16, height=12, fx=32.0, fy=32.0, cx=8.0, cy=6.0, min_range=0.1, max_range=3.0)


def plane_blocks(hole=None):
    """block index -> download_block-style dict; every voxel holds the analytic distance of its centre with weight 1.  `hole`:
    (lo, hi) global voxel index bounds (inclusive) of a box of never-observed voxels (weight 0)"""
    out = {}
    l = np.arange(VPS)
    lx, ly, lz = (a.ravel() for a in np.meshgrid(l, l, l, indexing="ij"))
    lin = lx + VPS * (ly + VPS * lz)
    for b in BLOCKS:
        g = np.stack([b[0] * VPS + lx, b[1] * VPS + ly, b[2] * VPS + lz], axis=1)
        centre = (g + 0.5) * VS32
        dist = np.zeros(VPS ** 3, np.float32)
        dist[lin] = ((centre - P0) @ N).astype(np.float32)
        w = np.ones(VPS ** 3, np.float32)
        if hole is not None:
            inside = np.all((g >= np.asarray(hole[0])) & (g <= np.asarray(hole[1])), axis=1)
            w[lin[inside]] = 0
        lab = np.full(VPS ** 3, 7, np.uint32)
        col = np.tile(np.array([10, 20, 30, 255], np.uint8), (VPS ** 3, 1))
        out[b] = {"distance": dist, "weight": w, "color": col, "sem_label": lab, "flags": np.full(VPS ** 3, capi.VOX_ACTIVE, np.uint8)}
    return out


def render(blocks, position, yaw, **kw):
    return rr.render(np.array(list(blocks), np.int32), lambda i: blocks[tuple(int(v) for v in i)], VPS, VS, SENSOR,
                     camera_pose(np.asarray(position, float), yaw), **kw)


def analytic_depth(position):
    """z-depth at which the ray of each pixel meets the plane, camera at `position` looking along +x: p(t) = c + t (1, -x, -y)"""
    u, v = np.meshgrid(np.arange(SENSOR.width), np.arange(SENSOR.height))
    x = (u - SENSOR.cx) / SENSOR.fx
    y = (v - SENSOR.cy) / SENSOR.fy
    direction = np.stack([np.ones_like(x), -x, -y], axis=-1)
    return ((P0 - np.asarray(position)) @ N) / (direction @ N)


def test_plane_depth_normal_and_attributes():
    """Hit depth against the analytic depth.  The bound, from the arithmetic (u = 2^-24, coordinates below 2.5 m, 25 voxels):
    a sample's distance differs from the exact linear field by at most
      5u * 2.5 m (the five roundings of p_W; |grad d| = 1) + (2u + u) * 25 voxels * 0.1 m (g = p * inv - 0.5, and inv itself)
      + u * 0.2 m (the stored taps near the crossing) + 21u * 0.2 m (seven lerps of three roundings each)    < 1.6e-6 m;
    the crossing of two such samples moves by at most that over the field's slope along the ray (>= 0.89 per metre of z-depth),
    and frac, frac * dt and the final sum add 3u * 1.4 m: 1.6e-6 / 0.89 + 2.5e-7 < 2.1e-6 m.  Asserted: 2.1e-6 m.
    The normal: central differences over 0.2 m of samples that are each within 1.6e-6 m: a component of g is within 3.2e-6 of
    0.2 N, so the unit vector is within 3.2e-6 / 0.2 * 2 = 3.2e-5 of N per component."""
    cam = (0.3, 0.0, 0.0)
    out = render(plane_blocks(), cam, 0.0)
    assert (out["status"] == 1).all() and out["n_hit"] == SENSOR.width * SENSOR.height and out["n_blocked"] == 0
    want = analytic_depth(cam)
    err = np.abs(out["depth"].astype(np.float64) - want)
    print("max |depth - analytic| = %.3g m" % err.max())
    assert err.max() <= 2.1e-6
    nerr = np.abs(out["normal"].astype(np.float64) - N).max()
    print("max |normal - N| = %.3g" % nerr)
    assert nerr <= 3.2e-5
    assert (out["label"] == 7).all() and (out["flags"] == capi.VOX_ACTIVE).all()
    assert (out["color"] == np.array([10, 20, 30, 255], np.uint8)).all()
    # a coarser march finds the same surface, and without semantics the label image is zero
    coarse = render(plane_blocks(), cam, 0.0, step_voxels=1.0, with_semantics=False)
    assert (coarse["status"] == 1).all() and coarse["samples_per_ray"] == 30 and out["samples_per_ray"] == 59
    assert np.abs(coarse["depth"].astype(np.float64) - want).max() <= 2.1e-6
    assert not coarse["label"].any()


def test_behind_the_plane_is_blocked():
    out = render(plane_blocks(), (2.0, 0.0, 0.0), 0.0)
    assert (out["status"] == 2).all() and out["n_blocked"] == SENSOR.width * SENSOR.height
    for k in ("depth", "normal", "color", "label", "flags"):
        assert not out[k].any(), k


def test_looking_away_is_none():
    out = render(plane_blocks(), (0.3, 0.0, 0.0), np.pi)
    assert (out["status"] == 0).all() and out["n_hit"] == 0 and out["n_blocked"] == 0
    for k in ("depth", "normal", "color", "label", "flags"):
        assert not out[k].any(), k


def test_no_hit_through_a_hole_of_unobserved_voxels():
    """a box of zero-weight voxels around the surface, across the middle of the view: a ray that crosses the surface inside it
    has no observed front crossing and comes out blocked (it meets observed interior voxels behind the box); rays that cross
    the surface well outside it still hit"""
    cam = (0.3, 0.0, 0.0)
    hole = ((9, -1, -1), (19, 0, 0))  # x in [0.9, 2.0), y, z in [-0.1, 0.1)
    out = render(plane_blocks(hole), cam, 0.0)
    t = analytic_depth(cam)
    u, v = np.meshgrid(np.arange(SENSOR.width), np.arange(SENSOR.height))
    py, pz = -(u - SENSOR.cx) / SENSOR.fx * t, -(v - SENSOR.cy) / SENSOR.fy * t  # where each ray meets the plane
    # a sample has a tap in the box iff, per axis, one of its two tap indices is: y and z both in [-0.15, 0.15)
    inside = (np.abs(py) < 0.13) & (np.abs(pz) < 0.13)
    outside = (np.abs(py) > 0.17) | (np.abs(pz) > 0.17)
    assert inside.sum() >= 4 and outside.sum() >= 20
    assert (out["status"][inside] == 2).all()
    assert not out["depth"][inside].any()
    assert (out["status"][outside] == 1).all()
    assert np.abs(out["depth"][outside].astype(np.float64) - t[outside]).max() <= 2.1e-6


def test_c_abi_symbol_and_python_wrapper_exist():
    assert "khr_render_view" in capi.EXPORTS
    lib = capi.load_library()
    assert lib.khr_render_view.argtypes is not None and len(lib.khr_render_view.argtypes) == 10
    assert callable(getattr(capi.FusionContext, "render_view"))
    assert callable(getattr(capi.FusionContext, "render_view_into"))
    hdr = open(os.path.join(ROOT, "include", "khronos_amd.h")).read()
    for word in ("khr_render_request", "khr_render_stats", "int khr_render_view(khr_ctx*"):
        assert word in hdr, word
    import ctypes as C
    assert C.sizeof(capi.KhrRenderRequest) == 32 + 128 + 8 and C.sizeof(capi.KhrRenderStats) == 32


def test_render_kernel_uses_no_scratch_memory():
    """the compiler's report for k_render_view<16> and <8> (khronos_amd/lib/resource_usage.txt, written by the build): registers
    only, no LDS"""
    from test_cpu_resource_guard import _kernels, _pick
    sel = _pick(_kernels(), r"^_ZN3khr13k_render_viewILi(16|8)EEE")
    assert len(sel) == 2, sorted(sel)
    for name, r in sel.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == 0 and r["VGPRs"] <= 128, (name, r)
