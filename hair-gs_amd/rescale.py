#!/usr/bin/env python3
"""Writes a smaller copy of a pinhole capture, so that train.py -r 1 on the copy and every capture tool (init_cloud.py, init_scalp.py,
view_metrics.py, which read cameras.bin) see one consistent, properly filtered scene.  Without it the loader resizes on every load
and subsamples the mask, orientation and confidence planes (scene/scene.py camera_from_info).
  python rescale.py -s <scene> -o <out scene> -r R [--images images] [--device cuda|cpu] [--batch 16]
                    [--orientations average|estimate|skip] [--overwrite]
-r has the loader's meaning (scene.scene.target_size owns the rule): 2, 4 and 8 divide both sides, any larger number is the target
width, -1 scales an image wider than 1600 px to 1600.  A camera the rule leaves alone keeps its size.
Reads <scene>/sparse/0 (binary or text; PINHOLE and SIMPLE_PINHOLE cameras -- run undistort.py first on any other), <scene>/<images>/<name>
and, where they exist, <scene>/masks/<name> and <scene>/orientations/<stem>_{orientation,confidence}.png; writes
  <out>/sparse/0/cameras.bin    every camera at its new size (utils/rescale.py rescaled_camera: COLMAP's Camera::Rescale)
  <out>/sparse/0/images.bin     the same poses, names and point3D ids; the keypoints scaled
  <out>/sparse/0/points3D.bin   the source file, byte for byte (points3D.txt where only the text form exists)
  <out>/images/<name>           area average (an RGBA image's alpha is a fourth channel);   <out>/masks/<name>   thresholded at 127.5
  <out>/orientations/           --orientations average (the default where <scene>/orientations exists): the pairs averaged as
                                double-angle vectors, gated by the source mask where there is one; estimate: orient.py runs on the
                                result; skip: none are written
  hair_eval_data.npz, head_reconstruction_data.npz, head_mesh.ply    copied where they exist (they do not depend on the resolution)
A PNG is written as PNG, a JPEG as JPEG at quality 95 under the same name.  Planes of one (camera, size, channel count) go through the
kernel in batches of --batch.  Refused: a scene no camera of which would shrink (nothing to do), -o equal to -s, an existing,
non-empty <out> without --overwrite, and a view with only one file of its orientation pair."""
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np

SIDE_FILES = ("hair_eval_data.npz", "head_reconstruction_data.npz", "head_mesh.ply")


def _batches(groups, batch):
    for key, views in groups.items():
        for b0 in range(0, len(views), batch):
            yield key, views[b0:b0 + batch]


def rescale_folder(jobs, cameras, out_cameras, mode, device, batch, gray):
    """jobs: (camera id, source path, output path).  Groups by (camera, channel count), rescales in batches, writes."""
    from undistort import read_image, write_image
    from utils.rescale import rescale_images
    groups = {}
    for cid, src, dst in jobs:
        a, fmt = read_image(src, cameras[cid], "a mask" if gray else "an image", gray=gray)
        groups.setdefault((cid, a.shape), []).append((a, fmt, dst))
    for (cid, _), chunk in _batches(groups, batch):
        out = rescale_images(np.stack([a for a, _, _ in chunk]), (out_cameras[cid].width, out_cameras[cid].height), mode, device=device)
        for i, (_, fmt, dst) in enumerate(chunk):
            write_image(dst, out[i], fmt)
    return len(jobs)


def rescale_pairs(jobs, cameras, out_cameras, device, batch):
    """jobs: (camera id, source stem path, mask path or None, output stem path).  Groups by (camera, mask or not)."""
    from undistort import read_image, write_image
    from utils.rescale import rescale_orientation
    groups = {}
    for cid, src, mask, dst in jobs:
        planes = [read_image(src + suffix, cameras[cid], "an orientation plane", gray=True)[0][:, :, 0]
                  for suffix in ("_orientation.png", "_confidence.png")]
        planes.append(None if mask is None else read_image(mask, cameras[cid], "a mask", gray=True)[0][:, :, 0])
        groups.setdefault((cid, mask is not None), []).append((planes, dst))
    for (cid, masked), chunk in _batches(groups, batch):
        t, c = rescale_orientation(np.stack([p[0] for p, _ in chunk]), np.stack([p[1] for p, _ in chunk]),
                                   np.stack([p[2] for p, _ in chunk]) if masked else None,
                                   (out_cameras[cid].width, out_cameras[cid].height), device=device)
        for i, (_, dst) in enumerate(chunk):
            write_image(dst + "_orientation.png", t[i][:, :, None], "PNG")
            write_image(dst + "_confidence.png", c[i][:, :, None], "PNG")
    return len(jobs)


def main(argv=None):
    parser = ArgumentParser(description="Write a smaller copy of a pinhole capture")
    parser.add_argument("--source_path", "-s", required=True, help="scene directory (sparse/0, <images>/, masks/, orientations/)")
    parser.add_argument("--output_path", "-o", required=True, help="scene directory to write")
    parser.add_argument("--resolution", "-r", type=int, required=True, help="2, 4, 8: divide; larger: the target width; -1: 1600 at most")
    parser.add_argument("--images", "-i", default="images")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the numpy path")
    parser.add_argument("--batch", type=int, default=16, help="planes of one camera per kernel launch")
    parser.add_argument("--orientations", choices=("average", "estimate", "skip"), default=None,
                        help="average (the default where <scene>/orientations exists), estimate (orient.py on the result) or skip")
    parser.add_argument("--overwrite", action="store_true")
    args = parser.parse_args(argv)
    from data.colmap import Image as ColmapImage, write_cameras_binary, write_images_binary
    from scene.scene import target_size
    from undistort import read_sparse
    from utils.rescale import rescale_keypoints, rescaled_camera
    if args.device not in ("cuda", "cpu"):
        raise SystemExit(f"rescale.py: --device {args.device}: cuda or cpu")
    src, out = args.source_path, args.output_path
    sparse = os.path.join(src, "sparse", "0")
    cameras, images = read_sparse(sparse)
    sizes = {cid: target_size(int(c.width), int(c.height), args.resolution) for cid, c in cameras.items()}
    try:
        out_cameras = {cid: rescaled_camera(c, sizes[cid]) for cid, c in cameras.items()}
    except ValueError as e:
        raise SystemExit(f"rescale.py: {e}")
    if all(sizes[cid] == (int(c.width), int(c.height)) for cid, c in cameras.items()):
        raise SystemExit(f"rescale.py: -r {args.resolution} shrinks no camera of {src}: there is nothing to do")
    if os.path.abspath(out) == os.path.abspath(src):
        raise SystemExit("rescale.py: the output scene must not be the source scene")
    if os.path.isdir(out) and os.listdir(out) and not args.overwrite:
        raise SystemExit(f"rescale.py: {out} exists and is not empty (pass --overwrite)")
    mode = args.orientations
    has_maps = os.path.isdir(os.path.join(src, "orientations"))
    if mode is None:
        mode = "average" if has_maps else "skip"
    elif mode == "average" and not has_maps:
        raise SystemExit(f"rescale.py: --orientations average: {os.path.join(src, 'orientations')} does not exist")
    device = None if args.device == "cpu" else "cuda"
    batch = max(1, args.batch)
    jobs, mask_jobs, pair_jobs = [], [], []
    for im in images.values():
        fname = os.path.basename(im.name)                  # (as the loader forms it)
        path = os.path.join(src, args.images, fname)
        if not os.path.exists(path):
            raise SystemExit(f"rescale.py: {path} is missing")
        jobs.append((im.camera_id, path, os.path.join(out, "images", fname)))
        mask = os.path.join(src, "masks", fname)
        if os.path.exists(mask):
            mask_jobs.append((im.camera_id, mask, os.path.join(out, "masks", fname)))
        if mode == "average":
            stem = os.path.join(src, "orientations", fname.split(".")[0])
            found = [os.path.exists(stem + suffix) for suffix in ("_orientation.png", "_confidence.png")]
            if any(found) and not all(found):
                raise SystemExit(f"rescale.py: {stem}: only one of _orientation.png and _confidence.png exists")
            if all(found):
                pair_jobs.append((im.camera_id, stem, mask if os.path.exists(mask) else None,
                                  os.path.join(out, "orientations", fname.split(".")[0])))
    out_sparse = os.path.join(out, "sparse", "0")
    for d in (out_sparse, os.path.join(out, "images")):
        os.makedirs(d, exist_ok=True)
    write_cameras_binary(out_cameras, os.path.join(out_sparse, "cameras.bin"))
    write_images_binary({k: ColmapImage(id=im.id, qvec=im.qvec, tvec=im.tvec, camera_id=im.camera_id, name=im.name,
                                        xys=rescale_keypoints(im.xys, cameras[im.camera_id], out_cameras[im.camera_id]),
                                        point3D_ids=im.point3D_ids) for k, im in images.items()},
                        os.path.join(out_sparse, "images.bin"))
    for name in ("points3D.bin", "points3D.txt"):
        if os.path.exists(os.path.join(sparse, name)):
            shutil.copyfile(os.path.join(sparse, name), os.path.join(out_sparse, name))
            break
    stale = os.path.join(out_sparse, "points3D.ply")     # (the loader's conversion of an earlier run's points)
    if os.path.exists(stale):
        os.remove(stale)
    for name in SIDE_FILES:
        if os.path.exists(os.path.join(src, name)):
            shutil.copyfile(os.path.join(src, name), os.path.join(out, name))
    n = rescale_folder(jobs, cameras, out_cameras, "average", device, batch, gray=False)
    if mask_jobs:
        os.makedirs(os.path.join(out, "masks"), exist_ok=True)
        rescale_folder(mask_jobs, cameras, out_cameras, "threshold", device, batch, gray=True)
    if pair_jobs:
        os.makedirs(os.path.join(out, "orientations"), exist_ok=True)
        rescale_pairs(pair_jobs, cameras, out_cameras, device, batch)
    shapes = sorted({f"{c.width} x {c.height} -> {sizes[cid][0]} x {sizes[cid][1]}" for cid, c in cameras.items()})
    print(f"{n} image(s), {len(mask_jobs)} mask(s) and {len(pair_jobs)} orientation pair(s) rescaled into {out} (-r {args.resolution}: "
          f"{', '.join(shapes)})")
    if mode == "estimate":
        import orient
        orient.main(["-s", out, "--device", args.device, "--batch", str(batch)] + (["--overwrite"] if args.overwrite else []))
    elif mode == "skip":
        print(f"orientation maps are not written: orient.py must be run on {out} before training (or pass --orientations estimate)")
    return n


if __name__ == "__main__":
    main()
