"""A general camera for the parity tests: SE(3) poses with roll and pitch, and calibrated-looking intrinsics (fx != fy, principal
point off centre by a non-integer amount).  Every other pose in tests/ is yaw-only with fx = fy and a centred principal point;
such a pose has four exact zeros and one exact -1 in its rotation, which hides index, ordering and swap errors in every kernel that
transforms a point.  Helper module, not a conftest."""
import math

import numpy as np

import common
from khronos_amd.synth import camera_pose

# frames on which general_trajectory is checked (tests/test_cpu_general_camera.py) and may be compared
GENERAL_FRAMES = 40


def pose_rpy(position, yaw, pitch, roll):
    """float64 world_T_sensor for the optical frame of camera_pose (x right, y down, z forward): camera_pose(position, yaw), then
    pitched about the camera's own x axis (pitch > 0 looks up), then rolled about its own optical axis.  With pitch = roll = 0
    both factors are the exact identity, so the result equals camera_pose(position, yaw) entry for entry."""
    T = camera_pose(np.asarray(position, np.float64), yaw)
    cp, sp = math.cos(pitch), math.sin(pitch)
    cr, sr = math.cos(roll), math.sin(roll)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    Rz = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    T[:3, :3] = T[:3, :3] @ Rx @ Rz
    return T


def general_angles(i, dt=0.1, period=10.0):
    """(position, yaw, pitch, roll) of frame i.  The position is SyntheticStream's circle (radius 1.5 m) with the height swinging
    by 0.4 m.  The yaw starts 0.1 rad off the tangent and turns at a quarter of the rate of travel, so that over GENERAL_FRAMES
    frames neither cos(yaw) nor sin(yaw) comes near zero.  Pitch and roll shake with a period of four frames -- a hand-held
    camera, not a dolly -- so that both take both signs without a frame landing near zero, and their amplitudes drift slowly.
    Pitch and roll share their sign on every frame: with cos(yaw) < 0 < sin(yaw) that keeps the two products of every mixed
    entry of the rotation from cancelling (the CPU test asserts min |Rw[i][j]| > 0.05 over the frames)."""
    th = 2.0 * math.pi * i * dt / period
    pos = np.array([1.5 * math.cos(th), 1.5 * math.sin(th), 1.5 + 0.4 * math.sin(0.5 * i + 0.3)])
    yaw = math.pi / 2 + 0.1 + 0.24 * th
    drift = 1.0 + 0.08 * math.sin(0.37 * i)
    pitch = (0.39, 0.19, -0.39, -0.19)[i % 4] * drift
    roll = (0.28, 0.09, -0.28, -0.09)[i % 4] * drift
    return pos, yaw, pitch, roll


def general_trajectory(i, dt=0.1, period=10.0):
    return pose_rpy(*general_angles(i, dt, period))


def GENERAL_INTRINSICS(W, H):
    """(fx, fy, cx, cy): fx / fy = 1.196, principal point off centre by a non-integer amount"""
    return 0.55 * W, 0.46 * W, W / 2.0 + 3.25, H / 2.0 - 2.75


class GeneralStream:
    """SyntheticStream's scene seen through the general camera: render(i) uses general_trajectory(i) and the overridden
    fx, fy, cx, cy attributes (SyntheticStream.render passes them to the renderer as they are)."""

    def __init__(self, stream):
        self.s = stream
        self.W, self.H = stream.W, stream.H
        stream.fx, stream.fy, stream.cx, stream.cy = GENERAL_INTRINSICS(stream.W, stream.H)
        self.fx, self.fy, self.cx, self.cy = stream.fx, stream.fy, stream.cx, stream.cy

    def pose(self, i):
        return general_trajectory(i, self.s.dt, self.s.period)

    def stamp_ns(self, i):
        return self.s.stamp_ns(i)

    def set_mover(self, *a, **kw):
        return self.s.set_mover(*a, **kw)

    def render(self, i, pose=None):
        return self.s.render(i, pose=self.pose(i) if pose is None else pose)


def general_stream(width, height, **kw):
    from khronos_amd.synth import SyntheticStream
    return GeneralStream(SyntheticStream(width, height, **kw))


def make_general_pair(width=320, height=240, seed=1234, stream_kw=None, **cfg_kw):
    """common.make_pair with the stream's intrinsics overridden before the sensors are made, and the stream's default pose
    replaced by general_trajectory: (cfg, ctx, ora, stream, sen, osen)"""
    made = {}
    real = common.SyntheticStream

    def factory(w, h, **kw):
        made["s"] = general_stream(w, h, **kw)
        return made["s"]
    common.SyntheticStream = factory
    try:
        cfg, ctx, ora, s, sen, osen = common.make_pair(width, height, seed, stream_kw, **cfg_kw)
    finally:
        common.SyntheticStream = real
    return cfg, ctx, ora, s, sen, osen
