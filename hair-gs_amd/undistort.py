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
so is an existing, non-empty <out> without --overwrite.  The file names, the image reader and the scene-writing steps are
data/capture.py's (rescale.py calls the same ones); this driver holds its arguments, its refusals, the camera and keypoint rule of
utils/undistort.py and the warp."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser


def run(args):
    """Writes the undistorted scene and returns its image count; every refusal is a ValueError."""
    from data import capture
    from utils.undistort import is_pinhole, undistort_images, undistort_keypoints, undistorted_camera
    if args.device not in ("cuda", "cpu"):
        raise ValueError(f"--device {args.device}: cuda or cpu")
    src, out = args.source_path, args.output_path
    cameras, images = capture.read_sparse(os.path.join(src, "sparse", "0"))
    if all(is_pinhole(c) for c in cameras.values()):
        raise ValueError(f"{src} holds only pinhole cameras: there is nothing to undistort")
    capture.check_output(src, out, args.overwrite)
    out_cameras = {cid: undistorted_camera(c, args.blank_pixels, args.min_scale, args.max_scale) for cid, c in cameras.items()}
    capture.write_sparse(src, out, cameras, images, out_cameras, undistort_keypoints)
    device = None if args.device == "cpu" else "cuda"
    views = list(capture.view_jobs(src, out, args.images, images))
    jobs, mask_jobs = [job for _, job, _ in views], [mask_job for _, _, mask_job in views if mask_job]

    def warp(mode):
        return lambda cid, stack: undistort_images(stack, cameras[cid], out_cameras[cid], mode, device=device)[0]
    n = capture.process_folder(jobs, cameras, False, args.batch, warp("bilinear"))
    if mask_jobs:
        os.makedirs(os.path.join(out, capture.MASKS), exist_ok=True)
        capture.process_folder(mask_jobs, cameras, True, args.batch, warp("threshold"))
    print(f"{n} image(s) and {len(mask_jobs)} mask(s) undistorted into {out}")
    return n


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
    args.batch = max(1, args.batch)
    try:
        n = run(args)
    except ValueError as e:
        raise SystemExit(f"undistort.py: {e}")
    if args.orient:
        import orient
        orient.main(["-s", args.output_path, "--device", args.device, "--batch", str(args.batch)] + (["--overwrite"] if args.overwrite else []))
    else:
        print(f"orientation maps are not warped: orient.py must be run on {args.output_path} before training (or pass --orient)")
    return n


if __name__ == "__main__":
    main()
