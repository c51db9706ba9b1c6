#!/usr/bin/env python3
"""Labels the scalp on a capture's head mesh from its hair masks and writes the capture's head_reconstruction_data.npz, the only source
of the strand roots that Stage II, Stage III, the evaluation and export_strands.py --max_root_distance need (utils/scalp.py states the
arithmetic).  synthesize.py writes that file from ground-truth strands and the reference's parsers from FLAME's fixed scalp region; a
capture of one's own has neither, but it has a head mesh aligned to the cameras and the hair masks.
  python init_scalp.py -s <scene> [--mesh <obj|ply>] [--spacing 0] [--min_cos 0.25] [--depth_tol T]
                       [--min_views 2] [--min_percent 70] [--dilate 0] [--max_points 20000]
                       [--device cuda|cpu] [--overwrite]
Reads <scene>/sparse/0 (binary or text; PINHOLE and SIMPLE_PINHOLE cameras only -- undistort.py makes them), <scene>/masks/<name> for
every image of the model (data/capture.py forms the names, as for the loader), and the mesh: --mesh, by default <scene>/head_mesh.ply.  An OBJ is read by data.head_data.load_obj
(polygons fanned into triangles), a PLY by utils/ply.py (a `vertex` element with x, y, z and a `face` element whose list property
holds three indices in every row).
The samples are the mesh's vertices and, with --spacing > 0, points spread over every face about that far apart.  A sample votes in
the views that see it: in frame, its normal turned towards the camera by at least --min_cos (the cosine), and no deeper than
--depth_tol behind the mesh's own depth map of that view (1 % of the mesh's bounding-box diagonal by default; absolute, in scene
units).  It is scalp where at least --min_views views see it and --min_percent percent of them find hair at its pixel.  --dilate r
widens every mask by r pixels first.  These defaults are knobs, not measured optima: hair that hangs in front of skin votes that
skin as scalp in the views where it does, and --min_percent is what one turns against it.
More than --max_points kept samples are thinned to those at positions floor(j*n/max_points) of their order (utils.carve.select).
head_reconstruction_data.npz gets head_verts = the mesh's vertices and scalp_verts = the kept points; it is written under a temporary
name and renamed into place.  A file that is already there is kept, once, as head_reconstruction_data.orig.npz, and is replaced only
with --overwrite.  main() returns the number of scalp points and prints the counts: samples, never visible, kept, dropped faces."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np

RESULT, BACKUP = "head_reconstruction_data.npz", "head_reconstruction_data.orig.npz"


def _fail(msg):
    raise SystemExit(f"init_scalp.py: {msg}")


def load_mesh(path):
    """(verts f64 [NV, 3], faces int64 [F, 3]) of an OBJ or a triangle PLY (data.head_data.load_mesh; refused in this driver's name)."""
    from data import head_data
    try:
        return head_data.load_mesh(path)
    except ValueError as e:
        _fail(str(e))


def main(argv=None):
    parser = ArgumentParser(description="Label the scalp on a capture's head mesh from its hair masks (the defaults are knobs, not measured optima)")
    parser.add_argument("--source_path", "-s", required=True, help="scene directory (sparse/0, masks/, head_mesh.ply)")
    parser.add_argument("--mesh", default=None, help="the head mesh, .obj or .ply, aligned to the cameras (default: <scene>/head_mesh.ply)")
    parser.add_argument("--spacing", type=float, default=0.0, help="0: the vertices only; > 0: also points about this far apart on every face")
    parser.add_argument("--min_cos", type=float, default=0.25, help="smallest cosine between a sample's normal and the ray to the camera (a knob)")
    parser.add_argument("--depth_tol", type=float, default=None, help="how far behind the mesh's depth map a sample still counts as visible, "
                        "in scene units (default: 1 %% of the mesh's bounding-box diagonal; a knob)")
    parser.add_argument("--min_views", type=int, default=2, help="a knob, not a measured optimum")
    parser.add_argument("--min_percent", type=int, default=70, help="percent of the views that see a sample which must find hair there (a knob)")
    parser.add_argument("--dilate", type=int, default=0, help="widen every mask by this many pixels first")
    parser.add_argument("--max_points", type=int, default=20000)
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the numpy path")
    parser.add_argument("--overwrite", action="store_true")
    args = parser.parse_args(argv)
    from data import capture
    from data.head_reconstruction_data import save_head_reconstruction_data_npz
    from utils import carve, scalp
    from utils.views import load_views, read_plane
    if args.device not in ("cuda", "cpu"):
        _fail(f"--device {args.device}: cuda or cpu")
    if args.min_views < 1 or not 0 <= args.min_percent <= 100 or args.dilate < 0 or args.max_points < 1 or not 0.0 <= args.min_cos <= 1.0 \
            or not (np.isfinite(args.spacing) and args.spacing >= 0.0) or (args.depth_tol is not None and not (np.isfinite(args.depth_tol) and args.depth_tol >= 0.0)):
        _fail("--min_views >= 1, 0 <= --min_percent <= 100, --dilate >= 0, --max_points >= 1, 0 <= --min_cos <= 1, --spacing >= 0 and "
              "--depth_tol >= 0 expected")
    src = args.source_path
    if not os.path.isdir(os.path.join(src, capture.MASKS)):
        _fail(f"{src} has no masks/ folder: there is nothing to label with")
    result, backup = os.path.join(src, RESULT), os.path.join(src, BACKUP)
    if os.path.exists(result) and not args.overwrite:
        _fail(f"{result} exists: pass --overwrite to replace it (the first file replaced is kept as {BACKUP})")
    try:
        views = load_views(os.path.join(src, "sparse", "0"))
        masks = [read_plane(capture.mask_path(src, capture.file_name(v)), v, "the mask", sized="a mask") for v in views]
    except ValueError as e:
        _fail(str(e))
    verts, faces = load_mesh(args.mesh or os.path.join(src, "head_mesh.ply"))
    device = None if args.device == "cpu" else "cuda"
    if args.dilate:
        masks = [carve.dilate(m, args.dilate, device=device) for m in masks]
    finite = verts[np.isfinite(verts).all(axis=1)]
    if finite.shape[0] == 0 or faces.shape[0] == 0:
        _fail("the mesh has no face or no finite vertex")
    depth_tol = 0.01 * float(np.linalg.norm(finite.max(axis=0) - finite.min(axis=0))) if args.depth_tol is None else args.depth_tol
    stats = {}
    try:
        points, vis, hits, kept = scalp.label_scalp(verts, faces, views, masks, args.spacing, args.min_cos, depth_tol, args.min_views,
                                                    args.min_percent, device=device, stats=stats)
    except ValueError as e:
        _fail(str(e))
    print(f"{len(views)} view(s), {verts.shape[0]} vertices, {faces.shape[0]} faces, depth_tol {depth_tol:.6g}")
    print(f"{vis.shape[0]} sample(s): {int((vis == 0).sum())} never visible, {int(kept.sum())} kept; {stats['dropped']} (face, view) pair(s) "
          "dropped (a vertex behind the camera or not finite)")
    if points.shape[0] == 0:
        _fail(f"no sample is scalp under --min_views {args.min_views}, --min_percent {args.min_percent}, --min_cos {args.min_cos}, "
              f"--depth_tol {depth_tol:.6g}, --dilate {args.dilate} (is the mesh aligned to the cameras?)")
    points = points[carve.select(points.shape[0], args.max_points)]
    tmp = os.path.join(src, f"head_reconstruction_data.{os.getpid()}.tmp.npz")     # (np.savez appends .npz to any other ending)
    save_head_reconstruction_data_npz(tmp, head_verts=verts, scalp_verts=points)
    if os.path.exists(result) and not os.path.exists(backup):                     # the first replacement: the old file moves aside, once
        os.replace(result, backup)
    os.replace(tmp, result)
    print(f"{points.shape[0]} scalp point(s) written to {result}")
    return points.shape[0]


if __name__ == "__main__":
    main()
