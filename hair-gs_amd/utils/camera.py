"""Synthetic camera rigs (counterpart of the reference's utils/camera.py:41-100 `generate_cameras`):
N-1 cameras on a circle around the anchor about one axis + one top view; OpenCV convention (x right, y down,
z forward); returns world-to-camera extrinsics."""
import collections

import numpy as np

ColmapCamera = collections.namedtuple("Camera", ["id", "model", "width", "height", "params"])


def _axis_rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], float)
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], float)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], float)


def generate_cameras(number_cameras, height, width, cam_pose=np.eye(4), anchor_pos=np.array([0, 0, 0]), offset=0.5,
                     rotation_axis="y", focal_length_px=500):
    """Returns ({id: ColmapCamera}, {id: w2c 4x4}).  `cam_pose` is the camera-to-world pose of camera 1."""
    ring = number_cameras - 1
    cams, Es = {}, {}
    anchor = np.asarray(anchor_pos, float)
    for i in range(ring):
        pose = np.array(cam_pose, float)
        pose[:3, 3] -= anchor
        Tm = np.eye(4)
        Tm[:3, :3] = _axis_rotation(rotation_axis, 2 * np.pi * i / ring)
        pose = Tm @ pose
        pose[:3, 3] += anchor
        Es[i + 1] = np.linalg.inv(pose)
        cams[i + 1] = ColmapCamera(i + 1, "SIMPLE_PINHOLE", width, height, [focal_length_px, width / 2, height / 2])
    pose = np.array(cam_pose, float)
    pose[:3, 3] = anchor + np.array([0, offset, 0])
    pose[:3, :3] = _axis_rotation("x", 3 * np.pi / 2) @ pose[:3, :3]
    Es[number_cameras] = np.linalg.inv(pose)
    cams[number_cameras] = ColmapCamera(number_cameras, "SIMPLE_PINHOLE", width, height,
                                        [focal_length_px, width / 2, height / 2])
    return cams, Es


def project_opencv(camera, E, points):
    """int16 [N, 2] pixel coordinates of world points [N, 3] through a pinhole camera (params[0] = f for both axes, params[1:3] =
    principal point; no distortion) with world-to-camera extrinsics E, truncated by astype(int16) as the reference does after
    cv2.projectPoints."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    E = np.asarray(E, dtype=np.float64)
    pc = p @ E[:3, :3].T + E[:3, 3]
    f, cx, cy = float(camera.params[0]), float(camera.params[1]), float(camera.params[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([f * (pc[:, 0] / pc[:, 2]) + cx, f * (pc[:, 1] / pc[:, 2]) + cy], axis=1)
    return uv.astype(np.int16)


def colmap_camera_to_projection_matrix(cam, w=None, h=None, znear=0.01, zfar=5):
    """Row-major OpenGL perspective matrix of a COLMAP pinhole camera: fov_y = focal2fov(fy, h), aspect w / h (w, h default to
    twice the principal point), as pyrr's create_perspective_projection builds it (ymax = znear tan(fov_y_deg pi / 360), xmax =
    ymax aspect, then the frustum from those bounds)."""
    from .graphics import focal2fov
    fy, cx, cy = cam.params[0], cam.params[1], cam.params[2]
    if cam.model != "SIMPLE_PINHOLE":
        fy, cx, cy = cam.params[1], cam.params[2], cam.params[3]
    w = cx * 2 if w is None else w
    h = cy * 2 if h is None else h
    fovy = np.rad2deg(focal2fov(fy, h))
    ymax = znear * np.tan(fovy * np.pi / 360.0)
    xmax = ymax * (w / h)
    left, right, bottom, top = -xmax, xmax, -ymax, ymax
    A = (right + left) / (right - left)
    B = (top + bottom) / (top - bottom)
    C = -(zfar + znear) / (zfar - znear)
    D = -2.0 * zfar * znear / (zfar - znear)
    E = 2.0 * znear / (right - left)
    F = 2.0 * znear / (top - bottom)
    return np.array([[E, 0.0, A, 0.0], [0.0, F, B, 0.0], [0.0, 0.0, C, D], [0.0, 0.0, -1.0, 0.0]])


def opencv_to_opengl_view_matrix(w2c):
    """OpenGL view matrix of an OpenCV world-to-camera matrix: the camera's y and z axes flipped, diag(1, -1, -1, 1) w2c."""
    return np.diag([1.0, -1.0, -1.0, 1.0]) @ np.asarray(w2c, dtype=np.float64)
