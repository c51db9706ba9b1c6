"""Planes and the small pinhole scene shared by tests/test_rescale_cpu.py and tests/test_rescale_gpu.py."""
import os

import numpy as np

from tests.undistort_cases import binary_masks, noise, tree_bytes  # noqa: F401

SIDE_FILES = ("hair_eval_data.npz", "head_reconstruction_data.npz", "head_mesh.ply")


def pair_planes(N, H, W, seed=0):
    """(angle, confidence, mask) uint8 [N, H, W]: every angle byte (0 and 255 among them), confidences with runs of 0, and a blocky
    mask that leaves whole footprints outside."""
    rng = np.random.default_rng(seed)
    angle = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
    conf = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
    conf[rng.random((N, H, W)) < 0.2] = 0
    return angle, conf, np.ascontiguousarray(binary_masks(N, H, W, seed=seed + 1)[:, :, :, 0])


def smooth_pair_planes(N, H, W, seed=0):
    """Like pair_planes, with angles that vary slowly (coherent footprints: high output confidences) around the 0 / 255 wrap."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (x * 3 + y * 2)[None] + rng.integers(0, 256, (N, 1, 1))
    angle = ((base + rng.integers(-3, 4, (N, H, W))) % 256).astype(np.uint8)
    conf = rng.integers(100, 256, (N, H, W), dtype=np.uint8)
    return angle, conf, np.ascontiguousarray(binary_masks(N, H, W, seed=seed + 1)[:, :, :, 0])


def build_scene(root):
    """A pinhole capture under <root>: camera 1 PINHOLE 48 x 36 (view_1.png with a mask and an orientation pair, view_2.jpg with a pair
    and no mask), camera 2 SIMPLE_PINHOLE 45 x 31 (view_3.png RGBA with a mask, view_4.png with nothing); keypoints, a points3D.bin
    and the three side files.  Returns (cameras, images)."""
    from PIL import Image as PILImage
    from data.colmap import Camera, Image, Point3D, write_cameras_binary, write_images_binary, write_points3D_binary
    from utils.transform import rot_to_wxyz_quat
    sparse = os.path.join(root, "sparse", "0")
    for d in (sparse, os.path.join(root, "images"), os.path.join(root, "masks"), os.path.join(root, "orientations")):
        os.makedirs(d, exist_ok=True)
    cams = {1: Camera(1, "PINHOLE", 48, 36, np.array([40.0, 41.5, 24.3, 17.6])),
            2: Camera(2, "SIMPLE_PINHOLE", 45, 31, np.array([38.0, 22.1, 15.2]))}
    rng = np.random.default_rng(5)
    images = {}
    for i, (cid, name, C, mask, pair) in enumerate(((1, "view_1.png", 3, True, True), (1, "view_2.jpg", 3, False, True),
                                                    (2, "view_3.png", 4, True, False), (2, "view_4.png", 3, False, False)), start=1):
        W, H = cams[cid].width, cams[cid].height
        a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        if name.endswith(".jpg"):
            PILImage.fromarray(a).save(os.path.join(root, "images", name), format="JPEG", quality=95)
        else:
            PILImage.fromarray(a).save(os.path.join(root, "images", name))
        if mask:
            m = np.zeros((H, W), np.uint8)
            m[7:29, 9:40] = 255
            PILImage.fromarray(m).save(os.path.join(root, "masks", name))
        if pair:
            t, c, _ = smooth_pair_planes(1, H, W, seed=i)
            PILImage.fromarray(t[0]).save(os.path.join(root, "orientations", name.split(".")[0] + "_orientation.png"))
            PILImage.fromarray(c[0]).save(os.path.join(root, "orientations", name.split(".")[0] + "_confidence.png"))
        ang = 0.4 * i
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        xys = np.column_stack([rng.uniform(4, W - 4, 5), rng.uniform(4, H - 4, 5)])
        images[i] = Image(id=i, qvec=rot_to_wxyz_quat(R), tvec=np.array([0.1 * i, -0.2, 2.0 + i]), camera_id=cid, name=name, xys=xys,
                          point3D_ids=np.arange(1, 6, dtype=np.int64))
    pts = {k: Point3D(id=k, xyz=rng.normal(size=3), rgb=rng.integers(0, 256, 3), error=0.5, image_ids=np.array([1, 2, 3, 4]),
                      point2D_idxs=[k - 1] * 4) for k in range(1, 6)}
    write_cameras_binary(cams, os.path.join(sparse, "cameras.bin"))
    write_images_binary(images, os.path.join(sparse, "images.bin"))
    write_points3D_binary(pts, os.path.join(sparse, "points3D.bin"))
    for k, name in enumerate(SIDE_FILES):
        with open(os.path.join(root, name), "wb") as fh:
            fh.write(bytes([k + 1]) * (10 + k))
    return cams, images


def decoded(root):
    """{relative path: uint8 array} of every PNG / JPEG under root."""
    from PIL import Image as PILImage
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            if f.endswith((".png", ".jpg")):
                with PILImage.open(os.path.join(dp, f)) as im:
                    out[os.path.relpath(os.path.join(dp, f), root)] = np.asarray(im).copy()
    return out
