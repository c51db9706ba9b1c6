#!/usr/bin/env python3
"""Traces strands from a capture's scalp through its lifted hair directions and saves them as a strand model (utils/trace.py states
the arithmetic): scalp-rooted strands straight from the capture tools' outputs, which train.py refines at once as Stage III (skipping
Stages I and II) and export_strands.py writes as a .hair / .data asset.
  python trace_strands.py -s <scene> -m <model dir>
      [--grid 128] [--radius 1.5] [--step 0.5] [--max_steps 400] [--max_angle 60] [--min_conf 0.5] [--max_gap 4]
      [--roots N] [--points 32] [--min_joints 4] [--min_length 0] [--head_margin 0] [--width 1e-4]
      [--fill N] [--fill_fixed_conf C] [--fill_domain hull|box] [--fill_min_views 3] [--fill_min_percent 50] [--no_fill_scalp]
      [--field out.npz] [--device cuda|cpu] [--overwrite]
Reads <scene>/sparse/0/points3D.ply, whose normals init_cloud.py --directions fills with a hair line per point (points with a zero
normal carry none and are left out), <scene>/head_reconstruction_data.npz (init_scalp.py: the scalp points are the roots, all of them
or --roots N of them at positions floor(j*n/N), utils.carve.select) and, when present, <scene>/head_sdf.npz (head_sdf.py): nodes whose
head distance is below --head_margin take no part.
The directions are splatted into a volume over the bounding box of the directed points and the roots, --grid nodes along its longest
side with the pad of radius + one spacing included; --radius and --step are in voxels.  A strand leaves its root along the direction
away from the mean of the head's vertices, follows the volume in steps of --step, and stops at the volume's border, at a turn sharper
than --max_angle degrees, after --max_gap steps in a row with less than --min_conf aligned mass, or after --max_steps steps.  These
defaults are knobs, not measured optima.
Strands of fewer than --min_joints joints or shorter than --min_length (scene units) are dropped; the others are resampled to --points
joints at uniform arc length and saved, grey, as <model dir>/point_cloud/iteration_1/point_cloud.ply, next to input.ply and
cameras.json as a first training run writes them.  A model directory that already holds a point_cloud/ is refused without --overwrite.
--fill N (default 0: nothing below runs) fills the volume between the scalp and the visible hair before the trace (utils/field_fill.py
states the arithmetic): the nodes with at least --fill_fixed_conf aligned mass (default: --min_conf) are held fixed, and so are the
nodes around the scalp points, splatted with their outward directions (--no_fill_scalp leaves those out); N Jacobi sweeps relax the
tensors d d^T of the nodes between them, and the filled nodes get the direction and the confidence (0 to 1) of the relaxed tensor.
<scene>/head_sdf.npz is required: the fill stays --head_margin outside the head.  --fill_domain hull also keeps it inside the masks'
hull (<scene>/masks/, a node votes as a point of init_cloud.py does, --fill_min_views and --fill_min_percent); box fills every node
outside the head, which suits synthetic scenes.  Prints the fixed, free and out nodes, the largest change of the last sweep and the
filled nodes that reach --min_conf.
--field also saves the direction volume (origin, spacing, shape, dir, conf), filled if it was.  Prints the skipped points, the
non-empty nodes, the strands per stop reason and the kept / dropped counts; main() returns the number of strands saved."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np

ITERATION = 1


def _fail(msg):
    raise SystemExit(f"trace_strands.py: {msg}")


def _write_inputs(source_path, model_path, ply_path):
    """input.ply and cameras.json, as scene.Scene writes them on a first run."""
    from data.dataset_readers import readColmapSceneInfo
    from scene.scene import camera_to_json
    os.makedirs(model_path, exist_ok=True)
    with open(ply_path, "rb") as src, open(os.path.join(model_path, "input.ply"), "wb") as dst:
        dst.write(src.read())
    try:
        info = readColmapSceneInfo(source_path, None)
    except (OSError, ValueError, KeyError) as e:
        _fail(f"{source_path}: the capture's cameras could not be read ({e})")
    with open(os.path.join(model_path, "cameras.json"), "w") as fh:
        json.dump([camera_to_json(i, c) for i, c in enumerate(info.cameras)], fh)


def fill_allowed(src, field, sdf, head_margin, domain, min_views, min_percent, device):
    """bool [nz, ny, nx]: the nodes the fill may relax.  Head distance >= head_margin; for the hull also the carve vote of the node
    positions against the capture's masks, views and masks read as init_cloud.py reads them."""
    from data import capture
    from utils import carve
    from utils import head_sdf as H
    nodes = field.nodes()
    d = H.sample(nodes.astype(np.float32), sdf, 0.0)[2].reshape(field.conf.shape)
    allowed = d >= np.float32(head_margin)
    if domain == "hull":
        from utils.views import load_views, read_plane
        if not os.path.isdir(os.path.join(src, capture.MASKS)):
            _fail(f"{src} has no {capture.MASKS}/ folder to take the hair's hull from: --fill_domain box fills every node outside the head")
        try:
            views = load_views(os.path.join(src, "sparse", "0"))
            masks = [read_plane(capture.mask_path(src, capture.file_name(v)), v, "the mask") for v in views]
        except ValueError as e:
            _fail(str(e))
        seen, hits = carve.mask_votes(nodes, views, masks, device=device)
        allowed &= carve.keep(seen, hits, min_views, min_percent).reshape(allowed.shape)
    return allowed


def fill_volume(args, src, field, scalp, head_verts, sdf, device):
    """Steps 3 to 6 of --fill: the scalp's nodes, the head exclusion, the domain, and the relaxation.  Returns the filled Field."""
    from utils import field_fill as FF
    from utils import trace as T
    fixed_conf = args.min_conf if args.fill_fixed_conf is None else args.fill_fixed_conf
    if not args.no_fill_scalp:
        sf = T.build_field(scalp, T.initial_directions(scalp, head_verts), field.origin, field.spacing, field.shape,
                           args.radius * field.spacing, device=device)
        take = (sf.conf >= fixed_conf) & (field.conf < fixed_conf)
        field.dir[take], field.conf[take] = sf.dir[take], sf.conf[take]
        print(f"{scalp.shape[0]} scalp point(s) splatted with their outward directions: {int(take.sum())} node(s) taken from them")
    print(f"{T.exclude_head(field, sdf, args.head_margin)} node(s) cleared: closer to the head than {args.head_margin:g}")
    allowed = fill_allowed(src, field, sdf, args.head_margin, args.fill_domain, args.fill_min_views, args.fill_min_percent, device)
    kind = FF.classify(field, fixed_conf, allowed)
    n_fixed, n_free, n_out = FF.counts(kind)
    print(f"fill ({args.fill_domain}): {n_fixed} fixed, {n_free} free, {n_out} out node(s)")
    stats = {}
    filled = FF.fill_field(field, kind, args.fill, device=device, stats=stats)
    reached = int(((kind == FF.FREE) & (filled.conf >= args.min_conf)).sum())
    print(f"{args.fill} sweep(s): the last one changed an entry by {stats['last_change']:.3e} at the most; {reached} of {n_free} free node(s) "
          f"ended with at least {args.min_conf:g}")
    return filled


def main(argv=None, field=None):
    """field: a utils.trace.Field to trace through instead of the one built from the cloud (programs and tests; not an option)."""
    knob = " (a knob, not a measured optimum)"
    parser = ArgumentParser(description="Trace strands from the scalp through the lifted hair directions and save them as a strand model "
                                        "(the defaults are knobs, not measured optima)")
    parser.add_argument("--source_path", "-s", required=True, help="scene directory (sparse/0/points3D.ply with directions, head_reconstruction_data.npz)")
    parser.add_argument("--model_path", "-m", required=True, help="model directory: point_cloud/iteration_1/point_cloud.ply is written there")
    parser.add_argument("--grid", type=int, default=128, help="nodes along the longest side of the direction volume" + knob)
    parser.add_argument("--radius", type=float, default=1.5, help="splat radius of a point, in voxels" + knob)
    parser.add_argument("--step", type=float, default=0.5, help="step length, in voxels" + knob)
    parser.add_argument("--max_steps", type=int, default=400, help="1 to 4096" + knob)
    parser.add_argument("--max_angle", type=float, default=60.0, help="sharpest turn between two steps, in degrees" + knob)
    parser.add_argument("--min_conf", type=float, default=0.5, help="least aligned mass, in fully weighted points, for a step to follow the volume" + knob)
    parser.add_argument("--max_gap", type=int, default=4, help="steps in a row a strand may coast straight on" + knob)
    parser.add_argument("--roots", type=int, default=None, metavar="N", help="trace from N of the scalp points (default: all)")
    parser.add_argument("--points", type=int, default=32, help="joints of a saved strand")
    parser.add_argument("--min_joints", type=int, default=4, help="drop strands that stopped with fewer joints")
    parser.add_argument("--min_length", type=float, default=0.0, help="drop strands shorter than this, in scene units")
    parser.add_argument("--head_margin", type=float, default=0.0, help="with head_sdf.npz: nodes closer to the head than this take no part")
    parser.add_argument("--width", type=float, default=1e-4, help="initial strand width")
    parser.add_argument("--fill", type=int, default=0, metavar="N", help="fill the volume between the scalp and the visible hair with N Jacobi sweeps (0: no fill)")
    parser.add_argument("--fill_fixed_conf", type=float, default=None, metavar="C", help="nodes with at least this aligned mass are held fixed (default: --min_conf)")
    parser.add_argument("--fill_domain", choices=("hull", "box"), default="hull", help="hull: inside the masks' hull and outside the head; box: every node outside the head")
    parser.add_argument("--fill_min_views", type=int, default=3, help="the hull's vote rule, as init_cloud.py --min_views")
    parser.add_argument("--fill_min_percent", type=int, default=50, help="the hull's vote rule, as init_cloud.py --min_percent")
    parser.add_argument("--no_fill_scalp", action="store_true", help="do not hold the scalp's outward directions fixed")
    parser.add_argument("--field", default=None, metavar="NPZ", help="also save the direction volume")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the numpy path")
    parser.add_argument("--overwrite", action="store_true")
    args = parser.parse_args(argv)
    from data.dataset_readers import fetchPly
    from data.head_reconstruction_data import load_head_reconstruction_data_npz
    from utils import carve
    from utils import head_sdf as H
    from utils import trace as T
    if args.device not in ("cuda", "cpu"):
        _fail(f"--device {args.device}: cuda or cpu")
    device = None if args.device == "cpu" else "cuda"
    finite = all(math.isfinite(v) for v in (args.radius, args.step, args.max_angle, args.min_conf, args.min_length, args.head_margin, args.width))
    if not finite or not (args.radius > 0 and args.step > 0 and 0 <= args.max_angle <= 180 and 1 <= args.max_steps <= T.MAX_STEPS
                          and args.max_gap >= 0 and args.points >= 2 and args.min_joints >= 2 and args.min_length >= 0 and args.width > 0
                          and (args.roots is None or args.roots >= 1)):
        _fail("--radius > 0, --step > 0, 0 <= --max_angle <= 180, 1 <= --max_steps <= 4096, --max_gap >= 0, --points >= 2, --min_joints >= 2, "
              "--min_length >= 0, --width > 0 and --roots >= 1 expected, all finite")
    if not 0 <= args.fill <= 65536 or (args.fill_fixed_conf is not None and not math.isfinite(args.fill_fixed_conf)) or args.fill_min_views < 1 \
            or not 0 <= args.fill_min_percent <= 100:
        _fail("0 <= --fill <= 65536, a finite --fill_fixed_conf, --fill_min_views >= 1 and 0 <= --fill_min_percent <= 100 expected")
    src, model = args.source_path, args.model_path
    ply_path = os.path.join(src, "sparse", "0", "points3D.ply")
    if not os.path.exists(ply_path):
        _fail(f"{ply_path} is missing: run init_cloud.py --directions -s {src} first")
    try:
        pcd = fetchPly(ply_path)
    except (ValueError, OSError, KeyError) as e:
        _fail(f"{ply_path}: {e}")
    points, dirs = np.asarray(pcd.points, np.float64), np.asarray(pcd.normals, np.float64)
    directed = dirs.any(axis=1)
    if not directed.any():
        _fail(f"{ply_path} holds no non-zero normal: init_cloud.py --directions writes the hair directions there")
    head_path = os.path.join(src, "head_reconstruction_data.npz")
    if not os.path.exists(head_path):
        _fail(f"{head_path} is missing: run init_scalp.py -s {src} first")
    head = load_head_reconstruction_data_npz(head_path)
    scalp = np.asarray(head.scalp_verts, np.float64).reshape(-1, 3)
    if scalp.shape[0] == 0:
        _fail(f"{head_path} holds no scalp point")
    pc_dir = os.path.join(model, "point_cloud")
    if os.path.isdir(pc_dir) and os.listdir(pc_dir) and not args.overwrite:
        _fail(f"{model} already holds a point_cloud/: pass --overwrite to write iteration_{ITERATION} into it")
    sdf = None
    if os.path.exists(H.scene_sdf_path(src)):
        try:
            sdf = H.load_sdf(H.scene_sdf_path(src))
        except ValueError as e:
            _fail(str(e))
    elif args.fill:
        _fail(f"{H.scene_sdf_path(src)} is missing: without it --fill would run into the head; run head_sdf.py -s {src} first")
    roots = scalp[carve.select(scalp.shape[0], scalp.shape[0] if args.roots is None else args.roots)]
    p0 = T.initial_directions(roots, head.head_verts)
    points, dirs = points[directed], dirs[directed]
    stats = {}
    try:
        if field is None:
            origin, h, shape = T.grid_box(points, roots, args.grid, args.radius)
            field = T.build_field(points, dirs, origin, h, shape, args.radius * h, device=device, stats=stats)
            print(f"{points.shape[0]} directed point(s) of {directed.shape[0]}, {stats['skipped']} skipped (not finite, or no direction); "
                  f"{shape[0]} x {shape[1]} x {shape[2]} nodes, h {h:.6g}, {stats['nonempty']} not empty")
        else:
            field = T.Field(field.origin, field.spacing, field.shape, field.dir.copy(), field.conf.copy())
            print(f"a given volume of {field.shape[0]} x {field.shape[1]} x {field.shape[2]} nodes, h {field.spacing:.6g}")
        if args.fill:
            field = fill_volume(args, src, field, scalp, head.head_verts, sdf, device)
        elif sdf is not None:
            print(f"{T.exclude_head(field, sdf, args.head_margin)} node(s) cleared: closer to the head than {args.head_margin:g}")
        h = field.spacing
        joints, count, reason = T.trace(roots, p0, field, args.step * h, args.max_steps, math.cos(math.radians(args.max_angle)),
                                        args.min_conf, args.max_gap, device=device)
    except ValueError as e:
        _fail(str(e))
    print(f"{roots.shape[0]} root(s): " + ", ".join(f"{int((reason == c).sum())} stopped by {name}" for c, name in enumerate(T.REASONS)))
    length = T.lengths(joints, count)
    keep = (count >= args.min_joints) & (length >= args.min_length)
    n = int(keep.sum())
    print(f"{n} strand(s) kept, {int((~keep).sum())} dropped (fewer than {args.min_joints} joints or shorter than {args.min_length:g})")
    if n == 0:
        _fail("no strand is left: is the cloud directed (init_cloud.py --directions), are the roots near it, is --min_conf too high?")
    strands = T.resample(joints[keep], count[keep], args.points).astype(np.float32)
    from scene.hair_gaussian_model import HairGaussianModel
    hair = HairGaussianModel.from_strands(strands, width=args.width, sh_degree=0, device="cpu", ref_strand_root=scalp)
    _write_inputs(src, model, ply_path)
    out = os.path.join(pc_dir, f"iteration_{ITERATION}", "point_cloud.ply")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hair.save_ply(out)
    if args.field:
        T.save_field(args.field, field)
        print(f"the direction volume written to {args.field}")
    print(f"{n} strand(s) of {args.points} joints written to {out}")
    return n


if __name__ == "__main__":
    main()
