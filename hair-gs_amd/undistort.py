#!/usr/bin/env python3
"""Undistorts a COLMAP capture (what the reference leaves to COLMAP's image_undistorter): a scene whose sparse model holds
SIMPLE_RADIAL, RADIAL, OPENCV or FULL_OPENCV cameras becomes a scene of PINHOLE cameras, which the loader accepts.
  python undistort.py -s <scene> -o <out scene> [--images images] [--device cuda|cpu] [--batch 16]
                      [--blank_pixels 0] [--min_scale 0.2] [--max_scale 2.0] [--orient] [--overwrite]
Reads <scene>/sparse/0 (binary or text), <scene>/<images>/<name> and, where it exists, <scene>/masks/<name>; writes
  <out>/sparse/0/cameras.bin    one PINHOLE camera per source camera id (utils/undistort.py undistorted_camera)
  <out>/sparse/0/images.bin     the same poses, names and point3D ids; the keypoints mapped into the new cameras on the host
  <out>/sparse/0/points3D.bin   the source file, byte for byte (points3D.txt where only the text form exists)
  <out>/images/<name>           bilinear;   <out>/masks/<name>   thresholded at 127.5 (a bilinear mask would erode under the loader)
Images are read with PIL (modes L, RGB, RGBA; PNG or JPEG) and must have their camera's size; a PNG is written as PNG, a JPEG as JPEG
at quality 95 under the same name (the loader finds files by name).  Images of one (camera, size, channel count) go through the
kernel in batches of --batch.  Orientation maps are not warped -- their angles are relative to the image axes, which bend under
the warp: run orient.py on the result, or pass --orient.  A scene that holds only pinhole cameras is refused (nothing to do), and
so is an existing, non-empty <out> without --overwrite."""
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np

_MODES = {"L": 1, "RGB": 3, "RGBA": 4}


def read_sparse(sparse):
    from data.colmap import read_extrinsics_binary, read_extrinsics_text, read_intrinsics_binary, read_intrinsics_text
    if os.path.exists(os.path.join(sparse, "images.bin")):
        return read_intrinsics_binary(os.path.join(sparse, "cameras.bin")), read_extrinsics_binary(os.path.join(sparse, "images.bin"))
    return (read_intrinsics_text(os.path.join(sparse, "cameras.txt"), pinhole_only=False),
            read_extrinsics_text(os.path.join(sparse, "images.txt")))


def read_image(path, camera, what, gray=False):
    """(uint8 [H, W, C], PIL format) of an image that must have its camera's size."""
    from PIL import Image
    with Image.open(path) as im:
        fmt = im.format
        if fmt not in ("PNG", "JPEG"):
            raise SystemExit(f"undistort.py: {path}: format {fmt} is not supported (PNG or JPEG)")
        if gray:
            im = im.convert("L")
        if im.mode not in _MODES:
            raise SystemExit(f"undistort.py: {path}: image mode {im.mode} is not supported (L, RGB or RGBA)")
        a = np.asarray(im)
    if a.shape[:2] != (int(camera.height), int(camera.width)):
        raise SystemExit(f"undistort.py: {path}: {what} of {a.shape[1]} x {a.shape[0]} pixels, camera {camera.id} has "
                         f"{camera.width} x {camera.height}")
    return a.reshape(a.shape[0], a.shape[1], -1), fmt


def write_image(path, a, fmt):
    from PIL import Image
    im = Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a)
    if fmt == "JPEG":
        im.save(path, format="JPEG", quality=95)
    else:
        im.save(path, format="PNG")


def warp_folder(jobs, cameras, out_cameras, mode, device, batch, gray):
    """jobs: (camera id, source path, output path).  Groups by (camera, channel count), warps in batches, writes."""
    from utils.undistort import undistort_images
    groups = {}
    for cid, src, dst in jobs:
        a, fmt = read_image(src, cameras[cid], "a mask" if gray else "an image", gray=gray)
        groups.setdefault((cid, a.shape), []).append((a, fmt, dst))
    for (cid, _), views in groups.items():
        for b0 in range(0, len(views), batch):
            chunk = views[b0:b0 + batch]
            out, _ = undistort_images(np.stack([a for a, _, _ in chunk]), cameras[cid], out_cameras[cid], mode, device=device)
            for i, (_, fmt, dst) in enumerate(chunk):
                write_image(dst, out[i], fmt)
    return len(jobs)


def main(argv=None):
    parser = ArgumentParser(description="Undistort a COLMAP capture into a scene of PINHOLE cameras")
    parser.add_argument("--source_path", "-s", required=True, help="scene directory (sparse/0, <images>/, masks/)")
    parser.add_argument("--output_path", "-o", required=True, help="scene directory to write")
    parser.add_argument("--images", "-i", default="images")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernel; cpu: the numpy path")
    parser.add_argument("--batch", type=int, default=16, help="images of one camera per kernel launch")
    parser.add_argument("--blank_pixels", type=float, default=0.0)
    parser.add_argument("--min_scale", type=float, default=0.2)
    parser.add_argument("--max_scale", type=float, default=2.0)
    parser.add_argument("--orient", action="store_true", help="run orient.py on the undistorted scene")
    parser.add_argument("--overwrite", action="store_true")
    args = parser.parse_args(argv)
    from data.colmap import Image as ColmapImage, write_cameras_binary, write_images_binary
    from utils.undistort import is_pinhole, undistort_keypoints, undistorted_camera
    if args.device not in ("cuda", "cpu"):
        raise SystemExit(f"undistort.py: --device {args.device}: cuda or cpu")
    src, out = args.source_path, args.output_path
    sparse = os.path.join(src, "sparse", "0")
    cameras, images = read_sparse(sparse)
    if all(is_pinhole(c) for c in cameras.values()):
        raise SystemExit(f"undistort.py: {src} holds only pinhole cameras: there is nothing to undistort")
    if os.path.abspath(out) == os.path.abspath(src):
        raise SystemExit("undistort.py: the output scene must not be the source scene")
    if os.path.isdir(out) and os.listdir(out) and not args.overwrite:
        raise SystemExit(f"undistort.py: {out} exists and is not empty (pass --overwrite)")
    try:
        out_cameras = {cid: undistorted_camera(c, args.blank_pixels, args.min_scale, args.max_scale) for cid, c in cameras.items()}
    except ValueError as e:
        raise SystemExit(f"undistort.py: {e}")
    out_sparse = os.path.join(out, "sparse", "0")
    for d in (out_sparse, os.path.join(out, "images")):
        os.makedirs(d, exist_ok=True)
    write_cameras_binary(out_cameras, os.path.join(out_sparse, "cameras.bin"))
    write_images_binary({k: ColmapImage(id=im.id, qvec=im.qvec, tvec=im.tvec, camera_id=im.camera_id, name=im.name,
                                        xys=undistort_keypoints(im.xys, cameras[im.camera_id], out_cameras[im.camera_id]),
                                        point3D_ids=im.point3D_ids) for k, im in images.items()},
                        os.path.join(out_sparse, "images.bin"))
    for name in ("points3D.bin", "points3D.txt"):
        if os.path.exists(os.path.join(sparse, name)):
            shutil.copyfile(os.path.join(sparse, name), os.path.join(out_sparse, name))
            break
    stale = os.path.join(out_sparse, "points3D.ply")     # (the loader's conversion of an earlier run's points)
    if os.path.exists(stale):
        os.remove(stale)
    device = None if args.device == "cpu" else "cuda"
    batch = max(1, args.batch)
    jobs, mask_jobs = [], []
    for im in images.values():
        fname = os.path.basename(im.name)                  # (as the loader forms it)
        path = os.path.join(src, args.images, fname)
        if not os.path.exists(path):
            raise SystemExit(f"undistort.py: {path} is missing")
        jobs.append((im.camera_id, path, os.path.join(out, "images", fname)))
        if os.path.exists(os.path.join(src, "masks", fname)):
            mask_jobs.append((im.camera_id, os.path.join(src, "masks", fname), os.path.join(out, "masks", fname)))
    n = warp_folder(jobs, cameras, out_cameras, "bilinear", device, batch, gray=False)
    if mask_jobs:
        os.makedirs(os.path.join(out, "masks"), exist_ok=True)
        warp_folder(mask_jobs, cameras, out_cameras, "threshold", device, batch, gray=True)
    print(f"{n} image(s) and {len(mask_jobs)} mask(s) undistorted into {out}")
    if args.orient:
        import orient
        orient.main(["-s", out, "--device", args.device, "--batch", str(batch)] + (["--overwrite"] if args.overwrite else []))
    else:
        print(f"orientation maps are not warped: orient.py must be run on {out} before training (or pass --orient)")
    return n


if __name__ == "__main__":
    main()
