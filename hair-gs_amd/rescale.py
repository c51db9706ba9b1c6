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
non-empty <out> without --overwrite, and a view with only one file of its orientation pair.  The file names, the image reader and the
scene-writing steps are data/capture.py's (undistort.py calls the same ones); this driver holds its arguments, its refusals, the camera
and keypoint rule of utils/rescale.py, the orientation pairs and the side files."""
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np

SIDE_FILES = ("hair_eval_data.npz", "head_reconstruction_data.npz", "head_mesh.ply")


def rescale_pairs(jobs, cameras, out_cameras, device, batch):
    """jobs: (camera id, source pair paths, mask path or None, output pair paths).  Groups by (camera, mask or not)."""
    from data import capture
    from utils.rescale import rescale_orientation
    groups = {}
    for cid, pair, mask, dst in jobs:
        size, owner = (int(cameras[cid].width), int(cameras[cid].height)), f"camera {cameras[cid].id}"
        planes = [capture.read_image(path, size, "an orientation plane", owner, convert="L")[0] for path in pair]
        planes.append(None if mask is None else capture.read_image(mask, size, "a mask", owner, convert="L")[0])
        groups.setdefault((cid, mask is not None), []).append((planes, dst))
    for (cid, masked), chunk in capture.batches(groups, batch):
        t, c = rescale_orientation(np.stack([p[0] for p, _ in chunk]), np.stack([p[1] for p, _ in chunk]),
                                   np.stack([p[2] for p, _ in chunk]) if masked else None,
                                   (out_cameras[cid].width, out_cameras[cid].height), device=device)
        for i, (_, dst) in enumerate(chunk):
            capture.write_image(dst[0], t[i][:, :, None], "PNG")
            capture.write_image(dst[1], c[i][:, :, None], "PNG")
    return len(jobs)


def run(args):
    """Writes the smaller scene and returns (its image count, the orientation mode); every refusal is a ValueError."""
    from data import capture
    from scene.scene import target_size
    from utils.rescale import rescale_images, rescale_keypoints, rescaled_camera
    if args.device not in ("cuda", "cpu"):
        raise ValueError(f"--device {args.device}: cuda or cpu")
    src, out = args.source_path, args.output_path
    cameras, images = capture.read_sparse(os.path.join(src, "sparse", "0"))
    sizes = {cid: target_size(int(c.width), int(c.height), args.resolution) for cid, c in cameras.items()}
    out_cameras = {cid: rescaled_camera(c, sizes[cid]) for cid, c in cameras.items()}
    if all(sizes[cid] == (int(c.width), int(c.height)) for cid, c in cameras.items()):
        raise ValueError(f"-r {args.resolution} shrinks no camera of {src}: there is nothing to do")
    capture.check_output(src, out, args.overwrite)
    mode = args.orientations
    has_maps = os.path.isdir(os.path.join(src, capture.ORIENTATIONS))
    if mode is None:
        mode = "average" if has_maps else "skip"
    elif mode == "average" and not has_maps:
        raise ValueError(f"--orientations average: {os.path.join(src, capture.ORIENTATIONS)} does not exist")
    device = None if args.device == "cpu" else "cuda"
    jobs, mask_jobs, pair_jobs = [], [], []
    for name, job, mask_job in capture.view_jobs(src, out, args.images, images):
        jobs.append(job)
        if mask_job:
            mask_jobs.append(mask_job)
        if mode == "average":
            pair = capture.pair_paths(os.path.join(src, capture.ORIENTATIONS), name)
            found = [os.path.exists(path) for path in pair]
            if any(found) and not all(found):
                raise ValueError(f"{os.path.join(src, capture.ORIENTATIONS, capture.stem(name))}: only one of {capture.ORIENTATION} and "
                                 f"{capture.CONFIDENCE} exists")
            if all(found):
                pair_jobs.append((job[0], pair, mask_job and mask_job[1], capture.pair_paths(os.path.join(out, capture.ORIENTATIONS), name)))
    capture.write_sparse(src, out, cameras, images, out_cameras, rescale_keypoints)
    for name in SIDE_FILES:
        if os.path.exists(os.path.join(src, name)):
            shutil.copyfile(os.path.join(src, name), os.path.join(out, name))

    def shrink(how):
        return lambda cid, stack: rescale_images(stack, (out_cameras[cid].width, out_cameras[cid].height), how, device=device)
    n = capture.process_folder(jobs, cameras, False, args.batch, shrink("average"))
    if mask_jobs:
        os.makedirs(os.path.join(out, capture.MASKS), exist_ok=True)
        capture.process_folder(mask_jobs, cameras, True, args.batch, shrink("threshold"))
    if pair_jobs:
        os.makedirs(os.path.join(out, capture.ORIENTATIONS), exist_ok=True)
        rescale_pairs(pair_jobs, cameras, out_cameras, device, args.batch)
    shapes = sorted({f"{c.width} x {c.height} -> {sizes[cid][0]} x {sizes[cid][1]}" for cid, c in cameras.items()})
    print(f"{n} image(s), {len(mask_jobs)} mask(s) and {len(pair_jobs)} orientation pair(s) rescaled into {out} (-r {args.resolution}: "
          f"{', '.join(shapes)})")
    return n, mode


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
    args.batch = max(1, args.batch)
    try:
        n, mode = run(args)
    except ValueError as e:
        raise SystemExit(f"rescale.py: {e}")
    if mode == "estimate":
        import orient
        orient.main(["-s", args.output_path, "--device", args.device, "--batch", str(args.batch)] + (["--overwrite"] if args.overwrite else []))
    elif mode == "skip":
        print(f"orientation maps are not written: orient.py must be run on {args.output_path} before training (or pass --orientations estimate)")
    return n


if __name__ == "__main__":
    main()
