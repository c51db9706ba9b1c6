"""Time of the mask carving (csrc/hgs_carve.hip through utils/carve.py and init_cloud.py): a --grid^3 voxel grid against --views views of
1920x1080 whose masks are the analytic silhouettes of an ellipsoid seen from a ring of cameras (nothing occludes: the rule defaults
to min_views 3, min_percent 100).  GPU ms, each the median of --reps launches between device events after a warm-up, buffers
resident: hgs_carve_grid over the cube [-1.2, 1.2]^3 -- with the given rule, and with min_views = all views, min_percent = 0, which
a voxel in every frame leaves only at the last view --, hgs_carve_shell on the result, hgs_carve_votes with the colour sums on
2 10^5 points; init_cloud.py --mode hull end to end on the same capture written to a temporary scene (PNG decoding, packing, both
grids, the copies and the write included; one run after a warm-up); and the numpy path's seconds for a 64^3 grid over the same
cube -- that size, not scaled.  Prints one JSON line and writes it to profiles/carve_timing.json (--out).
  python tools/carve_timing.py [--grid 256] [--views 32] [--reps 7] [--no_driver] [--no_numpy] [--out profiles/carve_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]

import numpy as np

W, H, F = 1920, 1080, 1600.0
AXES = np.array([0.8, 0.6, 1.0])            # the ellipsoid's half axes
RING = 4.0                                  # the cameras' distance from its centre


def look_at(c):
    f = -c / np.linalg.norm(c)
    r = np.cross(f, np.array([0.0, 0.0, 1.0]))
    r /= np.linalg.norm(r)
    R = np.stack([r, np.cross(f, r), f])
    return R, -R @ c


def capture(V):
    """(views, masks): V cameras on a ring with a little height, and the ellipsoid's silhouette in each (a pixel is set iff the ray
    through its centre meets the ellipsoid)."""
    from utils.carve import View
    views, masks = [], []
    xs, ys = (np.arange(W) + 0.5 - W / 2) / F, (np.arange(H) + 0.5 - H / 2) / F
    d_cam = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None], np.ones((H, W))), axis=-1)
    for k in range(V):
        a = 2.0 * np.pi * k / V
        c = np.array([RING * np.cos(a), RING * np.sin(a), 0.5 * np.sin(3 * a)])
        R, t = look_at(c)
        views.append(View(R=R, t=t, fx=F, fy=F, cx=W / 2, cy=H / 2, W=W, H=H, name=f"view_{k:02d}.png"))
        d = (d_cam @ R) / AXES                                   # world directions, in the space where the ellipsoid is the unit sphere
        o = c / AXES
        dist2 = (np.cross(np.broadcast_to(o, d.shape), d) ** 2).sum(-1) / (d * d).sum(-1)
        masks.append(np.where(dist2 <= 1.0, 255, 0).astype(np.uint8))
    return views, masks


def events(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def write_scene(root, views, masks):
    from PIL import Image as PILImage
    from data.colmap import Camera, Image, write_cameras_binary, write_images_binary
    from utils.transform import rot_to_wxyz_quat
    sparse = os.path.join(root, "sparse", "0")
    for d in (sparse, os.path.join(root, "images"), os.path.join(root, "masks")):
        os.makedirs(d)
    cams = {1: Camera(1, "PINHOLE", W, H, np.array([F, F, W / 2, H / 2]))}
    images = {k + 1: Image(id=k + 1, qvec=rot_to_wxyz_quat(v.R), tvec=v.t, camera_id=1, name=v.name, xys=np.zeros((0, 2)),
                           point3D_ids=np.zeros(0, np.int64)) for k, v in enumerate(views)}
    write_cameras_binary(cams, os.path.join(sparse, "cameras.bin"))
    write_images_binary(images, os.path.join(sparse, "images.bin"))
    for k, (v, m) in enumerate(zip(views, masks)):
        PILImage.fromarray(m).save(os.path.join(root, "masks", v.name))
        rgb = np.stack([m // 2 + 40, np.full_like(m, 10 + 7 * (k % 30)), 255 - m // 2], axis=-1)
        PILImage.fromarray(rgb).save(os.path.join(root, "images", v.name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min_views", type=int, default=3)
    ap.add_argument("--min_percent", type=int, default=100)
    ap.add_argument("--no_driver", action="store_true")
    ap.add_argument("--no_numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carve_timing.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "carve_timing.py measures the GPU path: it needs the GPU"
    from utils import carve
    views, masks = capture(a.views)
    images = [np.repeat(m[:, :, None], 3, axis=2) for m in masks]
    packed = carve.pack(views, masks, images, "cuda")
    n = a.grid
    origin, h = np.full(3, -1.2), 2.4 / n
    voxels = n ** 3
    res = {"device": torch.cuda.get_device_name(0), "grid": [n, n, n], "views": a.views, "view_size": [W, H], "reps": a.reps,
           "min_views": a.min_views, "min_percent": a.min_percent, "mask_bytes": int(sum(m.size for m in masks))}
    occ = carve.grid_device(origin, h, (n, n, n), packed, a.min_views, a.min_percent)
    res["kept_voxels"] = int(occ.sum())
    g_ms = events(lambda: carve.grid_device(origin, h, (n, n, n), packed, a.min_views, a.min_percent), a.reps)
    full_ms = events(lambda: carve.grid_device(origin, h, (n, n, n), packed, a.views, 0), a.reps)   # (a voxel every view sees is decided by the last view only)
    s_ms = events(lambda: carve.shell_device(occ), a.reps)
    res["shell_voxels"] = int(carve.shell_device(occ).sum())
    pts = torch.from_numpy(np.random.default_rng(0).uniform(-1.0, 1.0, (a.points, 3))).cuda()
    v_ms = events(lambda: carve.votes_device(pts, packed, with_rgb=True), a.reps)
    res.update({"grid_ms": round(g_ms, 3), "grid_ns_per_voxel": round(g_ms * 1e6 / voxels, 4),
                "grid_projections_upper_bound": voxels * a.views,
                "grid_bytes_per_voxel": {"written": 1, "mask_lookups_at_most": a.views, "view_record_bytes_scalar": 152 * a.views},
                "grid_ms_rule_all_views_0_percent": round(full_ms, 3),
                "shell_ms": round(s_ms, 3), "shell_GB_per_s_read_once_written_once": round(2 * voxels / s_ms / 1e6, 1),
                "votes_points": a.points, "votes_ms": round(v_ms, 3),
                "votes_projections_per_s": round(a.points * a.views / v_ms * 1e3)})
    if not a.no_driver:
        import init_cloud
        with tempfile.TemporaryDirectory() as tmp:
            write_scene(os.path.join(tmp, "scene"), views, masks)
            argv = ["-s", os.path.join(tmp, "scene"), "--grid", str(n), "--min_views", str(a.min_views), "--min_percent",
                    str(a.min_percent), "--device", "cuda", "--overwrite"]
            init_cloud.main(argv)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res["driver_points_written"] = init_cloud.main(argv)
            res["driver_e2e_s"] = round(time.perf_counter() - t0, 3)
    if not a.no_numpy:
        t0 = time.perf_counter()
        carve.grid_numpy(origin, 2.4 / 64, (64, 64, 64), views, masks, a.min_views, a.min_percent)
        dt = time.perf_counter() - t0
        res.update({"numpy_grid": [64, 64, 64], "numpy_s": round(dt, 2), "numpy_projections_per_s": round(64 ** 3 * a.views / dt)})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
