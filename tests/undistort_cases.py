"""Cameras, images and the small COLMAP scene shared by tests/test_undistort_cpu.py and tests/test_undistort_gpu.py."""
import os

import numpy as np

MODELS = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
REFUSED = ("OPENCV_FISHEYE", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE")


def camera(model, W, H, cam_id=1, f=None, c=None):
    """A camera of `model` with a visible amount of every coefficient the model has; f defaults to 0.8 W."""
    from data.colmap import Camera
    f = 0.8 * W if f is None else f
    cx, cy = (0.52 * W, 0.47 * H) if c is None else c
    params = {"SIMPLE_RADIAL": [f, cx, cy, -0.11],
              "RADIAL": [f, cx, cy, -0.15, 0.04],
              "OPENCV": [0.98 * f, 1.03 * f, cx, cy, -0.18, 0.06, 0.004, -0.003],
              "FULL_OPENCV": [0.98 * f, 1.03 * f, cx, cy, -0.2, 0.07, 0.003, -0.002, 0.01, 0.05, -0.02, 0.004]}[model]
    return Camera(id=cam_id, model=model, width=W, height=H, params=np.array(params, np.float64))


def pinhole(Wd, Hd, fx, fy, cx=None, cy=None, cam_id=1):
    from data.colmap import Camera
    return Camera(id=cam_id, model="PINHOLE", width=Wd, height=Hd,
                  params=np.array([fx, fy, Wd / 2 if cx is None else cx, Hd / 2 if cy is None else cy], np.float64))


def noise(N, H, W, C, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, C), dtype=np.uint8)


def binary_masks(N, H, W, seed=0):
    """Blocky 0 / 255 planes [N, H, W, 1]: edges for the threshold mode to cut."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 2, (N, (H + 4) // 5, (W + 4) // 5), dtype=np.uint8) * 255
    return np.repeat(np.repeat(small, 5, axis=1), 5, axis=2)[:, :H, :W, None].copy()


def build_scene(root):
    """A capture of 3 PNG images of 48 x 36 under <root>: camera 1 SIMPLE_RADIAL (two images), camera 2 OPENCV (one RGBA image), a
    mask for the first image, a few keypoints per image and a points3D.bin.  Returns (cameras, images)."""
    from PIL import Image as PILImage
    from data.colmap import Image, Point3D, write_cameras_binary, write_images_binary, write_points3D_binary
    from utils.transform import rot_to_wxyz_quat
    W, H = 48, 36
    sparse = os.path.join(root, "sparse", "0")
    for d in (sparse, os.path.join(root, "images"), os.path.join(root, "masks")):
        os.makedirs(d, exist_ok=True)
    cams = {1: camera("SIMPLE_RADIAL", W, H, 1), 2: camera("OPENCV", W, H, 2)}
    rng = np.random.default_rng(5)
    images = {}
    for i, (cid, C) in enumerate(((1, 3), (1, 3), (2, 4)), start=1):
        name = f"view_{i}.png"
        a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        PILImage.fromarray(a).save(os.path.join(root, "images", name))
        ang = 0.4 * i
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        xys = np.column_stack([rng.uniform(4, W - 4, 5), rng.uniform(4, H - 4, 5)])
        images[i] = Image(id=i, qvec=rot_to_wxyz_quat(R), tvec=np.array([0.1 * i, -0.2, 2.0 + i]), camera_id=cid, name=name, xys=xys,
                          point3D_ids=np.arange(1, 6, dtype=np.int64))
    mask = np.zeros((H, W), np.uint8)
    mask[8:30, 10:40] = 255
    PILImage.fromarray(mask).save(os.path.join(root, "masks", "view_1.png"))
    pts = {k: Point3D(id=k, xyz=rng.normal(size=3), rgb=rng.integers(0, 256, 3), error=0.5, image_ids=np.array([1, 2, 3]),
                      point2D_idxs=[k - 1] * 3) for k in range(1, 6)}
    write_cameras_binary(cams, os.path.join(sparse, "cameras.bin"))
    write_images_binary(images, os.path.join(sparse, "images.bin"))
    write_points3D_binary(pts, os.path.join(sparse, "points3D.bin"))
    return cams, images


def tree_bytes(root):
    """{relative path: bytes} of every file under root."""
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out
