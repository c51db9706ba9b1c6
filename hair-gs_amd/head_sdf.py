#!/usr/bin/env python3
"""Builds the signed distance field of a capture's head mesh and writes the capture's head_sdf.npz, which train.py --lambda_head
loads for the head-penetration term (utils/head_sdf.py states the arithmetic of the field and of the term).
  python head_sdf.py -s <scene> [--mesh <obj|ply>] [--grid 128] [--pad 0.1] [--device cuda|cpu] [--overwrite]
  python head_sdf.py -s <scene> --report <model dir | strand PLY> [--device cuda|cpu]
The mesh is --mesh, by default <scene>/head_mesh.ply, read as init_scalp.py reads it (an OBJ, or a triangle PLY).  The field covers
the mesh's bounding box widened by --pad times its longest side, with --grid nodes along the longest widened side; a face with a
vertex that is not finite is dropped and a face of zero area skipped, and both counts are printed with the box and the spacing.
head_sdf.npz is written under a temporary name and renamed into place; a file that is already there is replaced only with
--overwrite.  The build is the plain nodes x faces form: --device cpu (the numpy path) is for small grids.
--report reads <scene>/head_sdf.npz and the joints of a trained strand model (a model directory is read at its newest
point_cloud/iteration_N) and prints how many joints lie inside the head, their share, the deepest penetration and the mean depth, in
scene units (utils.head_sdf.penetration_stats: the term's own sampling statement); nothing is written.  main() returns the HeadSDF, or
the report's dict."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np


def _fail(msg):
    raise SystemExit(f"head_sdf.py: {msg}")


def _load_mesh(path):
    from data.head_data import load_mesh           # (the reader behind init_scalp.load_mesh)
    try:
        return load_mesh(path)
    except ValueError as e:
        _fail(str(e))


def model_joints(path):
    """The joints f32 [E, 3] of a strand model: a PLY, or a model directory at its newest iteration."""
    from utils.ply import read_ply
    from utils.system import model_ply
    try:
        ply = model_ply(path)
        els = read_ply(ply)
    except (ValueError, OSError) as e:
        _fail(str(e))
    d = dict(els)
    if len(els) != 5 or "segment" not in d or "vertex" not in d:
        _fail(f"{ply}: not a strand model (5 elements: vertex, edge, segment, strand_root_idx, ref_strand_root); a Gaussian cloud has no joints")
    v = d["vertex"]
    return ply, np.stack([np.asarray(v[n], np.float32) for n in "xyz"], axis=1)


def report(source_path, model, device):
    from utils import head_sdf as H
    path = H.scene_sdf_path(source_path)
    if not os.path.exists(path):
        _fail(f"{path} is missing: run head_sdf.py -s {source_path} first")
    try:
        sdf = H.load_sdf(path)
    except ValueError as e:
        _fail(str(e))
    ply, joints = model_joints(model)
    st = H.penetration_stats(joints, sdf, device=device)
    print(f"{ply}: {st['joints']} joint(s), {st['inside']} inside the head ({100.0 * st['share']:.3f} %), deepest {st['deepest']:.6g}, "
          f"mean depth {st['mean_depth']:.6g} (scene units; spacing {sdf.spacing:.6g})")
    return st


def main(argv=None):
    parser = ArgumentParser(description="Build the signed distance field of a capture's head mesh (head_sdf.npz), or report a model's joints against it")
    parser.add_argument("--source_path", "-s", required=True, help="scene directory (head_mesh.ply; head_sdf.npz is written here)")
    parser.add_argument("--mesh", default=None, help="the head mesh, .obj or .ply, aligned to the cameras (default: <scene>/head_mesh.ply)")
    parser.add_argument("--grid", type=int, default=128, help="nodes along the longest side of the widened box (2 to 512)")
    parser.add_argument("--pad", type=float, default=0.1, help="widen the mesh's box on every side by this share of its longest side")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the numpy path")
    parser.add_argument("--overwrite", action="store_true")
    parser.add_argument("--report", default=None, metavar="MODEL", help="a trained strand model (directory or PLY): print its joints' penetration, write nothing")
    args = parser.parse_args(argv)
    from utils import head_sdf as H
    if args.device not in ("cuda", "cpu"):
        _fail(f"--device {args.device}: cuda or cpu")
    device = None if args.device == "cpu" else "cuda"
    src = args.source_path
    if not os.path.isdir(src):
        _fail(f"{src} is not a directory")
    if args.report is not None:
        return report(src, args.report, device)
    result = H.scene_sdf_path(src)
    if os.path.exists(result) and not args.overwrite:
        _fail(f"{result} exists: pass --overwrite to replace it")
    verts, faces = _load_mesh(args.mesh or os.path.join(src, "head_mesh.ply"))
    stats = {}
    try:
        sdf = H.build_sdf(verts, faces, grid=args.grid, pad=args.pad, device=device, stats=stats)
    except ValueError as e:
        _fail(str(e))
    nx, ny, nz = sdf.shape
    top = sdf.origin + (np.array(sdf.shape) - 1) * sdf.spacing
    print(f"{verts.shape[0]} vertices, {faces.shape[0]} faces: {stats['faces']} used, {stats['dropped']} dropped (a vertex not finite), "
          f"{stats['degenerate']} degenerate (zero area)")
    print(f"box {sdf.origin.tolist()} .. {top.tolist()}, h {sdf.spacing:.6g}, {nx} x {ny} x {nz} nodes, "
          f"{int((sdf.phi < 0).sum())} inside")
    if not (sdf.phi < 0).any():
        print("no node lies inside: the term will find nothing to push out (faces must be wound counter-clockwise seen from outside, "
              "and --grid fine enough for a node to fall inside)")
    tmp = os.path.join(src, f"head_sdf.{os.getpid()}.tmp.npz")                  # (np.savez appends .npz to any other ending)
    H.save_sdf(tmp, sdf)
    os.replace(tmp, result)
    print(f"written to {result}")
    return sdf


if __name__ == "__main__":
    main()
