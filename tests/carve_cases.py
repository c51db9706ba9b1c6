"""Cameras, masks, images and the small COLMAP scene shared by tests/test_carve_cpu.py and tests/test_carve_gpu.py."""
import os

import numpy as np

SIZES = ((45, 31), (64, 48))       # the two view sizes that the equality cases mix (W, H)


def look_at(centre, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """(R, t) world -> camera of a camera at `centre` looking at `target` (x right, y down, z forward)."""
    c, target, up = (np.asarray(a, np.float64) for a in (centre, target, up))
    f = target - c
    f /= np.linalg.norm(f)
    if abs(f @ up) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    return R, -R @ c


def view(R, t, W, H, f, name="view", cx=None, cy=None):
    from utils.carve import View
    return View(R=np.asarray(R, np.float64), t=np.asarray(t, np.float64), fx=float(f), fy=float(f) * 1.03,
                cx=W / 2 + 0.3 if cx is None else cx, cy=H / 2 - 0.2 if cy is None else cy, W=W, H=H, name=name)


def ring_views(V, radius=3.0, height=0.4, sizes=SIZES, f_scale=0.9):
    """V cameras on a ring around the origin, looking at it; sizes alternate."""
    out = []
    for k in range(V):
        a = 2.0 * np.pi * k / V + 0.3
        W, H = sizes[k % len(sizes)]
        R, t = look_at((radius * np.cos(a), radius * np.sin(a), height * (1 + k % 3)))
        out.append(view(R, t, W, H, f_scale * W, name=f"ring_{k}.png"))
    return out


def axis_views(dist, W=64, H=64, f=200.0):
    """Six cameras on the axes at `dist` from the origin, principal point at the image centre, fx = fy = f."""
    from utils.carve import View
    out = []
    for k, c in enumerate(((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))):
        R, t = look_at(dist * np.asarray(c, np.float64))
        out.append(View(R=R, t=t, fx=f, fy=f, cx=W / 2, cy=H / 2, W=W, H=H, name=f"axis_{k}.png"))
    return out


def sphere_mask(v, r, value=255):
    """uint8 [H, W]: a pixel is set iff the ray through its centre passes within r of the world origin (float64)."""
    xs = (np.arange(v.W, dtype=np.float64) + 0.5 - v.cx) / v.fx
    ys = (np.arange(v.H, dtype=np.float64) + 0.5 - v.cy) / v.fy
    d = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None], np.ones((v.H, v.W))), axis=-1)
    o = np.asarray(v.t, np.float64)                       # the world origin in camera coordinates
    dist = np.linalg.norm(np.cross(np.broadcast_to(o, d.shape), d), axis=-1) / np.linalg.norm(d, axis=-1)
    return np.where((dist <= r) & (o[2] > 0), value, 0).astype(np.uint8)


def random_masks(views, density, seed=0, value=None):
    """uint8 planes with about `density` of the pixels set (to `value`, or to random non-zero values)."""
    rng = np.random.default_rng(seed)
    out = []
    for v in views:
        on = rng.random((v.H, v.W)) < density
        vals = rng.integers(1, 256, (v.H, v.W)) if value is None else np.full((v.H, v.W), value)
        out.append(np.where(on, vals, 0).astype(np.uint8))
    return out


def random_images(views, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (v.H, v.W, 3), dtype=np.uint8) for v in views]


def identity_view(W, H):
    """R = I, t = 0, fx = fy = 1, cx = cy = 0: the point (x, y, 1) lands on u = x, v = y exactly."""
    from utils.carve import View
    return View(R=np.eye(3), t=np.zeros(3), fx=1.0, fy=1.0, cx=0.0, cy=0.0, W=W, H=H, name="identity.png")


def border_points(W, H):
    """Points for identity_view(W, H) with the expected `seen`: u == 0 is seen and u == W is not (likewise v); zc == 0, zc < 0, NaN and
    Inf coordinates are not seen."""
    inf, nan = float("inf"), float("nan")
    pts = [((0.0, 0.0, 1.0), 1), ((float(W), 0.0, 1.0), 0), ((float(W - 1), float(H - 1), 1.0), 1), ((0.0, float(H), 1.0), 0),
           ((-1.0, 0.0, 1.0), 0), ((0.0, -1.0, 1.0), 0), ((1.0, 1.0, 0.0), 0), ((1.0, 1.0, -1.0), 0), ((0.0, 0.0, 0.0), 0),
           ((nan, 0.0, 1.0), 0), ((0.0, nan, 1.0), 0), ((0.0, 0.0, nan), 0), ((inf, 0.0, 1.0), 0), ((0.0, -inf, 1.0), 0),
           ((0.0, 0.0, inf), 0), ((inf, inf, inf), 0), ((2.0 * (W - 1), 2.0 * (H - 1), 2.0), 1), ((0.5, 0.5, 1.0), 1)]
    return np.array([p for p, _ in pts], np.float64), np.array([s for _, s in pts], np.int32)


def cloud(n, seed=0, spread=1.2):
    return np.random.default_rng(seed).normal(scale=spread, size=(n, 3))


def build_scene(root, r=1.0, model="PINHOLE", n_points=60, text_points=False):
    """A capture under <root>: six axis cameras at 10 r (64 x 64, f = 200), sphere masks of radius r, random RGB images, and a COLMAP
    cloud of n_points normal points (spread r).  Returns (views, masks, images, (xyz, rgb, error))."""
    from PIL import Image as PILImage
    from data.colmap import Camera, Image, Point3D, write_cameras_binary, write_images_binary, write_points3D_binary
    from utils.carve import view_of
    from utils.transform import rot_to_wxyz_quat
    sparse = os.path.join(root, "sparse", "0")
    for d in (sparse, os.path.join(root, "images"), os.path.join(root, "masks")):
        os.makedirs(d, exist_ok=True)
    raw = axis_views(10.0 * r)
    params = {"PINHOLE": [200.0, 200.0, 32.0, 32.0], "SIMPLE_PINHOLE": [200.0, 32.0, 32.0],
              "OPENCV": [200.0, 200.0, 32.0, 32.0, 0.01, 0.0, 0.0, 0.0]}[model]
    cams, images = {}, {}
    for k, v in enumerate(raw, start=1):
        cams[k] = Camera(id=k, model=model, width=v.W, height=v.H, params=np.array(params, np.float64))
        images[k] = Image(id=k, qvec=rot_to_wxyz_quat(v.R), tvec=v.t, camera_id=k, name=v.name, xys=np.zeros((0, 2)),
                          point3D_ids=np.zeros(0, np.int64))
    write_cameras_binary(cams, os.path.join(sparse, "cameras.bin"))
    write_images_binary(images, os.path.join(sparse, "images.bin"))
    rng = np.random.default_rng(11)
    xyz = rng.normal(scale=r, size=(n_points, 3))
    rgb = rng.integers(0, 256, (n_points, 3), dtype=np.uint8)
    err = rng.uniform(0.1, 2.0, n_points)
    if text_points:
        with open(os.path.join(sparse, "points3D.txt"), "w") as fh:
            fh.write("# 3D point list\n")
            for i in range(n_points):
                fh.write(f"{i + 1} {float(xyz[i, 0])!r} {float(xyz[i, 1])!r} {float(xyz[i, 2])!r} {rgb[i, 0]} {rgb[i, 1]} {rgb[i, 2]} {float(err[i])!r}\n")
    else:
        write_points3D_binary({i + 1: Point3D(id=i + 1, xyz=xyz[i], rgb=rgb[i], error=err[i], image_ids=np.array([1, 2]),
                                              point2D_idxs=[0, 0]) for i in range(n_points)}, os.path.join(sparse, "points3D.bin"))
    if model == "OPENCV":
        views = None
    else:
        views = [view_of(cams[k], images[k]) for k in cams]
    masks = [sphere_mask(v, r) for v in raw]
    imgs = random_images(raw, seed=4)
    for v, m, im in zip(raw, masks, imgs):
        PILImage.fromarray(m).save(os.path.join(root, "masks", v.name))
        PILImage.fromarray(im).save(os.path.join(root, "images", v.name))
    return views, masks, imgs, (xyz, rgb, err)


def read_points(path):
    from data.colmap import read_points3D_binary
    return read_points3D_binary(path)
