#!/usr/bin/env python3
"""Writes the orientation maps a capture needs for training (what the reference's dataset parsers make with
utils/vision.py estimate_orientation_field): for every image in <scene>/<images>, <scene>/orientations/<stem>_orientation.png
(theta * 255 / pi) and <stem>_confidence.png (confidence * 255), both truncated to uint8; data/capture.py (pair_paths) forms the
names, for this driver as for the loader.
  python orient.py -s <scene> [--images images] [--device cuda|cpu] [--batch 16] [--overwrite]
                   [--kernel_size 31] [--sigma 2] [--lambda_ 3] [--gamma 0.5] [--num_angles 180]
Images are read with PIL: mode L as it is, RGB through OpenCV's RGB2GRAY weights, RGBA without its alpha; other modes are refused.
On the GPU, views of one size go through the kernels in batches of --batch.  A view whose pair of maps exists is skipped unless
--overwrite is given; a view without any orientation variance (a uniform image) stops the run."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np


def read_gray(path):
    from PIL import Image
    from utils.vision import to_gray
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            raise ValueError(f"{path}: image mode {im.mode} is not supported (L, RGB or RGBA)")
        return to_gray(np.asarray(im))


def list_images(folder):
    from PIL import Image
    exts = {e for e, fmt in Image.registered_extensions().items() if fmt in Image.OPEN}
    return sorted(f for f in os.listdir(folder) if os.path.isfile(os.path.join(folder, f)) and os.path.splitext(f)[1].lower() in exts)


def write_maps(pair, field, conf):
    from PIL import Image
    from utils.vision import orientation_pngs
    for path, plane in zip(pair, orientation_pngs(field, conf)):
        Image.fromarray(plane).save(path)


def main(argv=None):
    parser = ArgumentParser(description="Orientation maps of a capture's images")
    parser.add_argument("--source_path", "-s", required=True, help="scene directory (holds <images>/; orientations/ is written)")
    parser.add_argument("--images", "-i", default="images")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the CPU path (scipy FFT)")
    parser.add_argument("--batch", type=int, default=16, help="views of one size per kernel launch")
    parser.add_argument("--overwrite", action="store_true")
    parser.add_argument("--kernel_size", type=int, default=31)
    parser.add_argument("--sigma", type=float, default=2)
    parser.add_argument("--lambda_", type=float, default=3)
    parser.add_argument("--gamma", type=float, default=0.5)
    parser.add_argument("--num_angles", type=int, default=180)
    args = parser.parse_args(argv)
    from data import capture
    from utils.vision import NoVarianceError, estimate_orientation_field, estimate_orientation_fields
    params = dict(kernel_size=args.kernel_size, sigma=args.sigma, lambda_=args.lambda_, gamma=args.gamma, num_angles=args.num_angles)
    folder = os.path.join(args.source_path, args.images)
    out_dir = os.path.join(args.source_path, capture.ORIENTATIONS)
    os.makedirs(out_dir, exist_ok=True)
    todo = []
    for name in list_images(folder):
        pair = capture.pair_paths(out_dir, name)
        if all(os.path.exists(path) for path in pair) and not args.overwrite:
            continue
        todo.append((name, pair))
    print(f"{len(todo)} view(s) to estimate in {folder}")
    if args.device == "cpu":
        for name, pair in todo:
            gray = read_gray(os.path.join(folder, name))
            try:
                field, conf = estimate_orientation_field(gray, **params)
            except ValueError as e:
                raise SystemExit(f"orient.py: {os.path.join(folder, name)}: {e}")
            write_maps(pair, field, conf)
        return len(todo)
    import torch
    groups = {}
    for name, pair in todo:
        g = read_gray(os.path.join(folder, name))
        groups.setdefault(g.shape, []).append((name, pair, g))
    for views in groups.values():
        for b0 in range(0, len(views), max(1, args.batch)):
            chunk = views[b0:b0 + max(1, args.batch)]
            gray = torch.from_numpy(np.stack([g for _, _, g in chunk])).to(args.device)
            try:
                field, conf = estimate_orientation_fields(gray, **params)
            except NoVarianceError as e:
                raise SystemExit(f"orient.py: {', '.join(os.path.join(folder, chunk[i][0]) for i in e.views)}: no pixel with nonzero "
                                 "orientation variance (a uniform image?): the confidence is undefined")
            field, conf = field.cpu().numpy(), conf.cpu().numpy()
            for i, (_, pair, _) in enumerate(chunk):
                write_maps(pair, field[i], conf[i])
    return len(todo)


if __name__ == "__main__":
    main()
