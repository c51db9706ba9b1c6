#!/usr/bin/env python3
"""Exports the strands of a trained strand model (Stage II / III) as hair assets other tools read: the step behind train.py /
merge.py that the reference leaves to scripts/convert_output.py (MeshLab PLYs of the joints only).
  python export_strands.py -m <model dir | strand PLY> [-s <capture>] -o <out> --format hair|usc|ply_edges|ply_faces|npz [--format ...]
                           [--points 100] [--min_segments 1] [--min_length 0] [--max_root_distance D] [--colour model|strand]
                           [--device cuda|cpu] [--interpolate [--roots N] [--guides 4] [--max_guide_distance D] [--max_angle 60] [--no_guides]]
                           [--resolve_head [--head_margin 0] [--collide_iters 8] [--head_sdf PATH]]
                           [--attach_roots [--attach_margin 0] [--attach_step S] [--attach_max_steps 256] [--attach_pull 1] [--attach_descent 0.25]
                            [--attach_max_distance D] [--attach_field PATH] [--attach_min_conf 0.5] [--attach_scalp_distance D] [--drop_unattached]]
                           [--smooth_strands [--smooth_iters 10] [--smooth_lambda 0.5] [--smooth_mu -0.53] [--smooth_max_move D]]
                           [--dedupe DIST]
                           [--select_guides K [--select_samples 16] [--select_iters 10]]
                           [--simplify TOL]
A model directory is read at its newest point_cloud/iteration_N (utils/system.py model_ply, as eval.py reads it); the SH degree is read off the file.  Every
strand is resampled by arc length to --points points (0: its joints as they are) with per-point colour, opacity and width
(scene/strand_export.py: the contract; --device cuda = the HIP kernels on the model's device tensors, cpu = the numpy path), strands
with fewer than --min_segments segments, shorter than --min_length or rooted farther than --max_root_distance from the nearest
strand root are dropped, and one file per --format is written (data/strand_files.py):
  hair       <out>.hair   Cem Yuksel's format: segment counts, points, thickness = width, transparency = 1 - opacity, colours
  usc        <out>.data   USC-HairSalon's layout: strand count, then per strand a point count and its float32 points
  ply_edges  <out>.ply    vertices + an `edge` element (polylines)
  ply_faces  <out>.ply    one thin triangle per segment, for viewers without polylines (<out>_faces.ply if ply_edges is also asked for)
  npz        <out>.npz    the keys of hair_eval_data.npz (oriented points)
The strand roots come from the model file; -s names a capture whose head_reconstruction_data.npz replaces them (needed only where
the file has none).  --colour strand gives the PLYs one hue per strand instead of the model's colours.
--interpolate turns the exported strands into guides of a dense groom (scene/groom.py: the contract): every strand root -- the file's,
or with -s the capture's scalp points, --roots N of them taken evenly -- gets a strand blended from its --guides nearest guides by
inverse squared distance; roots farther than --max_guide_distance from every guide's root get none, and guides whose root-to-tip
direction turns more than --max_angle degrees from the nearest guide's are left out (a root at a parting follows one side).  The guides
are written first (--no_guides: not at all), then the interpolated strands.  --points 0 has no fixed number of points to blend and is
refused.  With -s and a head_sdf.npz in the capture, the number of interpolated points inside the head is printed.
--resolve_head pushes every strand that will be written out of the head (scene/strand_collide.py: the contract): after the resampling
and --interpolate, before the writers, a joint closer to the head than --head_margin (scene units, inside counting as negative) is
moved out along the gradient of the capture's distance field -- --head_sdf, by default <-s>/head_sdf.npz, which head_sdf.py writes --
in at most --collide_iters pushes (1 to 32), and the joints behind it keep their segments' lengths and return to their path.  Roots do
not move and attributes are untouched; the points inside before and after, the points moved, those left inside and the largest
displacement are printed.  It works on ragged strands (--points 0) too.  Without the flag the strands are written as they are.
--attach_roots roots every strand on the head (scene/strand_attach.py: the contract): trained strands begin wherever a view saw hair,
millimetres to centimetres above the skin.  After the resampling and its filters, before --interpolate and --resolve_head (guides are
rooted before they are blended, and the new joints are pushed out with the rest), a polyline is marched from every strand's root joint
back to the head of the same distance field (--head_sdf, else <-s>/head_sdf.npz): it starts along the strand's backward tangent, follows
the direction volume --attach_field (an .npz of trace_strands.py --field) where that has at least --attach_min_conf aligned mass, and
is pulled down the field's gradient with weight --attach_pull, never descending by less than --attach_descent of a step, in steps of
--attach_step (half the field's spacing) and at most --attach_max_steps of them, until it lands --attach_margin above the surface.  The
new joints are put in front of the strand's own with the root joint's attributes; with --points M > 0 the joined strand is resampled
to M points again.  A strand already on the head, one farther than --attach_max_distance from it and one whose march fails keep all
their bits (--drop_unattached drops the failed ones); with --attach_scalp_distance D a strand that landed farther than D from every
strand root -- on the face or the neck -- is restored too.  The strands attached, already rooted, failed by reason and dropped, the
joints added, the largest and mean root gap before and the largest |d - margin| of the landed roots are printed.  Without the flag
the strands are written as they are.
--smooth_strands low-passes every strand (scene/strand_smooth.py: the contract): the joints are trained Gaussian endpoints, which jitter
from segment to segment, and a renderer that takes its tangents from neighbouring points shades that jitter as frizz.  After the
resampling and --attach_roots (the kink where the marched joints meet the strand's own is smoothed with the landed root pinned), before
--interpolate (guides are smoothed before they are blended) and --resolve_head (a joint the filter pulled into the head is pushed out
again), --smooth_iters (1 to 256) times a sweep that moves every inner joint by --smooth_lambda towards the mean of its neighbours,
weighted by the original segment lengths, is followed by one with --smooth_mu (negative, below -lambda: Taubin's filter, which does
not shrink the strand; 0: plain Laplacian smoothing, which does); with --smooth_max_move D no joint ends farther than D from where it
was.  Roots, tips and attributes keep their bits, strands of fewer than 3 or more than 1024 joints or with a coordinate that is not
finite are left alone and counted, and the spacing is not made uniform again.  The strands smoothed and left alone, the joints held at
D, the largest and mean displacement, the mean turning angle per joint before and after and the strands' length ratios are printed.
Without the flag the strands are written as they are.
--select_guides K picks K guide strands from the strands that are written (scene/strand_guides.py: the contract): what a simulation of
the groom wants -- a few representative strands, and for every written strand the guide it follows.  It runs last, after --interpolate
and --resolve_head and just in front of the writers, on exactly the strands that are written, and needs a fixed number of points per
strand (--points M > 0).  Lloyd's k-means over --select_samples (2 to 64) joints taken evenly along every strand, seeded by index, at
most --select_iters (1 to 256) assignments; every cluster's most central member is its guide.  The main outputs are written as without
the flag, byte for byte; for every --format the guide strands go to the same path with _guides in front of the extension, and
<out>_guide_binding.npz holds guide_strand (the guide's index among the written strands), strand_guide (every written strand's guide,
-1 for a strand with a coordinate that is not finite), strand_distance (the RMS joint distance to the cluster's centre), cluster_size,
k, samples, iterations and converged.  The guides made, the empty clusters, the iterations, the cluster sizes, the distances and the
total squared distance after the first and the last assignment are printed.  --guides belongs to --interpolate and is another thing.
--simplify TOL drops every joint that lies within TOL (scene units) of the chord that replaces it (scene/strand_simplify.py: the
contract): the chain up to here keeps a strand's point count or multiplies it, --points is one number for all strands, and after
--smooth_strands most joints lie on their neighbours' chord to well under a hair's width, while .hair, .data and the PLYs are ragged by
design.  It is Douglas-Peucker's rule with the distance to the segment, so a curl that turns back over its chord is not flattened; it
runs last, directly in front of the writers, on exactly the strands that are written -- after --interpolate and --resolve_head, and
after --select_guides has chosen (the k-means needs the uniform strands): the guide files then hold the simplified strands at
guide_strand, and <out>_guide_binding.npz is what it is without the flag.  Kept joints keep the bits of their points and attributes,
roots and tips are always kept, strands of fewer than 3 or more than 1024 joints or with a coordinate that is not finite are left
alone and counted, and attributes are not looked at: the line `Simplified strands (tol ...): ...` says how many joints are left, how
many a strand keeps, the rounds taken, the largest deviation of a dropped joint and, per attribute, how far a dropped joint's value
was from linear between the kept joints around it.  It works with --points 0 too.  Without the flag the strands are written as they
are.
--dedupe DIST drops the near copies among the strands that are written (scene/strand_dedupe.py: the contract): --interpolate gives a
root that sits on a guide's root that guide back, and a trained model carries duplicated strands of its own, which a renderer pays for
and shades darker than one.  A strand is dropped when an earlier strand that is itself kept has EVERY joint within DIST (scene units)
of its own joint of the same index; earlier strands win, so the trained strands beat the interpolated ones.  It is the chain's only
strand-to-strand step and runs after --interpolate and --resolve_head, before --select_guides (the k-means then clusters, and the
binding indexes, the strands that are written) and --simplify; it compares joint by joint and needs a fixed number of points per
strand (--points M > 0).  Kept strands keep every bit; strands with a coordinate that is not finite pair with nothing and stay.  The
line `Deduplicated strands (dist ...): ...` says how many strands stay, the pairs found, the rounds the resolution took, how many
kept strands replace others and the most one replaces.  A DIST that pairs more than 2^27 times glues the groom together and is refused.
Without the flag the strands are written as they are."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np

FORMATS = ("hair", "usc", "ply_edges", "ply_faces", "npz")


def load_strand_model(path, capture=None, device="cpu"):
    """The strand model of a PLY with its strands walked; a Gaussian cloud (one element) is refused."""
    from scene.hair_gaussian_model import HairGaussianModel
    from scene.ply_io import load_hair_ply
    from utils.ply import read_ply
    els = read_ply(path)
    if len(els) == 1:
        raise ValueError(f"{path}: a Gaussian cloud (one PLY element) has no strands to export; run merge.py (Stage II) on it first")
    seg = dict(els).get("segment")
    if len(els) != 5 or seg is None:
        raise ValueError(f"{path}: not a strand model (5 elements: vertex, edge, segment, strand_root_idx, ref_strand_root)")
    n_rest = sum(1 for n in seg.dtype.names if n.startswith("f_rest_"))
    sh_degree = int(round(np.sqrt((n_rest + 3) / 3))) - 1
    roots = None
    if capture is not None:
        from data.head_reconstruction_data import load_head_reconstruction_data_npz
        head = os.path.join(capture, "head_reconstruction_data.npz")
        if not os.path.exists(head):
            raise FileNotFoundError(f"{head}: the capture has no head reconstruction to take strand roots from")
        roots = np.asarray(load_head_reconstruction_data_npz(head).scalp_verts)
    file_has_roots = dict(els)["ref_strand_root"].shape[0] > 0
    if not file_has_roots and roots is None:
        raise ValueError(f"{path}: the model file carries no strand roots to orient its strands by; pass -s <capture>")
    gs = HairGaussianModel(sh_degree, device=device)
    load_hair_ply(gs, path, elements=els, walk=False)      # (the file is read once; the walk follows the choice of roots)
    if roots is not None:
        gs.ref_strand_root = roots
    gs.compute_strands_info()
    return gs


def output_paths(out, formats):
    base = out
    for ext in (".hair", ".data", ".ply", ".npz"):
        if base.lower().endswith(ext):
            base = base[:-len(ext)]
    paths = {"hair": base + ".hair", "usc": base + ".data", "ply_edges": base + ".ply", "npz": base + ".npz",
             "ply_faces": base + ("_faces.ply" if "ply_edges" in formats else ".ply")}
    return {f: paths[f] for f in formats}


def interpolated(args, model, guides):
    """--interpolate: the exported strands as guides, a strand for every strand root blended from them (scene/groom.py), and the two
    together (or, with --no_guides, the interpolated ones alone)."""
    from scene.groom import concatenate, interpolate_strands
    from utils.carve import select
    roots = np.asarray(model.ref_strand_root, np.float64).reshape(-1, 3)
    if args.roots is not None:
        if args.roots < 0:
            raise ValueError(f"--roots {args.roots}: a number of roots")
        roots = roots[select(roots.shape[0], args.roots)]
    groom = interpolate_strands(guides, roots, k=args.guides, max_guide_distance=args.max_guide_distance, max_angle=args.max_angle,
                                device=None if args.device == "cpu" else args.device, first_id=model.strands_info.n_strands)
    new = groom.strands
    mean = float(groom.n_guides.mean()) if new.n_strands else 0.0
    print(f"Interpolated: {roots.shape[0]} roots, {groom.n_dropped} dropped (no guide in reach), {new.n_strands} strands from "
          f"{guides.n_strands} guides, {mean:.2f} guides per root on average")
    if args.source_path is not None:
        from utils import head_sdf
        path = head_sdf.scene_sdf_path(args.source_path)
        if os.path.exists(path) and not args.resolve_head:       # (--resolve_head reports, and removes, the points inside)
            _, _, d, in_range = head_sdf.sample(new.points, head_sdf.load_sdf(path))
            with np.errstate(invalid="ignore"):
                inside = int(np.count_nonzero(in_range & (d < 0)))
            print(f"Inside the head ({path}): {inside} of {new.points.shape[0]} interpolated points (they are written as they are)")
    return new if args.no_guides else concatenate(guides, new)


def head_field_path(args):
    """--resolve_head: the distance field's file, --head_sdf or the capture's; None where there is none."""
    from utils import head_sdf
    path = args.head_sdf if args.head_sdf is not None else (head_sdf.scene_sdf_path(args.source_path) if args.source_path is not None else None)
    return path if path is not None and os.path.exists(path) else None


def resolved(args, path, strands):
    """--resolve_head: the strands pushed out of the head of the field at `path` (scene/strand_collide.py), and what that did."""
    from scene.strand_collide import resolve_head
    from utils import head_sdf
    out, st = resolve_head(strands, head_sdf.load_sdf(path), margin=args.head_margin, iters=args.collide_iters,
                           device=None if args.device == "cpu" else args.device)
    print(f"Resolved against the head ({path}, margin {args.head_margin:g}): inside the head before: {st['inside_before']} of {st['joints']} "
          f"points, after: {st['inside_after']} (deepest {st['deepest_before']:.4g} -> {st['deepest_after']:.4g}); moved {st['moved']} points "
          f"of {st['strands_touched']} strands, unresolved: {st['unresolved']}, largest displacement {st['largest_displacement']:.4g}")
    return out


def attach_knobs(args):
    """--attach_roots: the march's keyword arguments (scene/strand_attach.py check_parameters)."""
    return dict(margin=args.attach_margin, step=args.attach_step, max_steps=args.attach_max_steps, pull=args.attach_pull,
                descent=args.attach_descent, max_distance=args.attach_max_distance, min_conf=args.attach_min_conf)


def attached(args, path, model, strands):
    """--attach_roots: the strands marched back to the head of the field at `path` (scene/strand_attach.py), and what that did."""
    from scene import strand_attach as SA
    from utils import head_sdf
    from utils.trace import load_field
    volume = load_field(args.attach_field) if args.attach_field is not None else None
    scalp = {}
    if args.attach_scalp_distance is not None:
        scalp = dict(scalp_points=np.asarray(model.ref_strand_root, np.float64).reshape(-1, 3), scalp_distance=args.attach_scalp_distance)
    out, rep = SA.attach_roots(strands, head_sdf.load_sdf(path), volume, points=args.points, device=None if args.device == "cpu" else args.device,
                               **scalp, **attach_knobs(args))
    failed = sum(rep["failed"].values())
    dropped = 0
    if args.drop_unattached and failed:
        out = SA.select_strands(out, (rep["reason"] == SA.REACHED) | (rep["reason"] == SA.NEAR))
        dropped = failed
    reasons = ", ".join(f"{k} {v}" for k, v in rep["failed"].items())
    print(f"Attached to the head ({path}, margin {args.attach_margin:g}" + (f", steered by {args.attach_field}" if volume is not None else "")
          + f"): {rep['attached']} of {rep['strands']} strands attached, {rep['near']} already rooted, {failed} failed"
          + (f" ({reasons})" if failed else "") + f", {dropped} dropped; {rep['joints_added']} joints added; root gap before: largest "
          f"{rep['gap_max']:.4g}, mean {rep['gap_mean']:.4g}; largest |d - margin| of the landed roots: {rep['landed_error']:.3g}")
    return out


def smoothed(args, strands):
    """--smooth_strands: the strands low-passed (scene/strand_smooth.py), and what that did."""
    from scene.strand_smooth import smooth_strands
    out, rep = smooth_strands(strands, iters=args.smooth_iters, lam=args.smooth_lambda, mu=args.smooth_mu, max_move=args.smooth_max_move,
                              device=None if args.device == "cpu" else args.device)
    print(f"Smoothed strands ({args.smooth_iters} x lambda {args.smooth_lambda:g} | mu {args.smooth_mu:g}): {rep['smoothed']} of {rep['strands']} "
          f"strands smoothed, left alone: {rep['short']} short, {rep['long']} long, {rep['nonfinite']} not finite; {rep['joints']} joints, "
          + (f"{rep['clamped']} held at {args.smooth_max_move:g}, " if args.smooth_max_move is not None else "")
          + f"largest displacement {rep['largest_displacement']:.4g}, mean {rep['mean_displacement']:.4g}; mean turning angle per joint "
          f"{rep['turning_before']:.4g} -> {rep['turning_after']:.4g} degrees; length after / before: {rep['length_ratio_min']:.4f} to "
          f"{rep['length_ratio_max']:.4f}, mean {rep['length_ratio_mean']:.4f}")
    return out


def deduplicated(args, strands):
    """--dedupe: the strands without their near copies (scene/strand_dedupe.py), and what that did."""
    from scene.strand_dedupe import dedupe_strands
    out, rep = dedupe_strands(strands, args.dedupe, device=None if args.device == "cpu" else args.device)
    print(f"Deduplicated strands (dist {args.dedupe:g}): {rep['kept']} of {rep['strands']} strands kept, {rep['dropped']} dropped "
          f"({rep['nonfinite']} not finite, which pair with nothing); {rep['pairs']} pairs, {rep['rounds']} rounds; {rep['groups']} kept strands "
          f"replace others, at most {rep['largest_group']} each; joints {rep['joints_before']} -> {rep['joints_after']}")
    return out


def selected(args, strands):
    """--select_guides: (guide strands, binding) of the strands that are written (scene/strand_guides.py), and what that did."""
    from scene.strand_guides import select_guides
    guides, binding, rep = select_guides(strands, args.select_guides, samples=args.select_samples, iters=args.select_iters,
                                         device=None if args.device == "cpu" else args.device)
    print(f"Selected guides (k {args.select_guides}, {args.select_samples} samples, at most {args.select_iters} iterations): {guides.n_strands} "
          f"guides from {rep['eligible']} of {rep['strands']} strands ({rep['nonfinite']} not finite), {rep['clusters_empty']} of "
          f"{rep['clusters_made']} clusters empty; {rep['iterations']} iterations, " + ("converged" if rep["converged"] else "not converged")
          + f"; cluster size {rep['size_min']} to {rep['size_max']}, mean {rep['size_mean']:.4g}; RMS joint distance to the centre: mean "
          f"{rep['distance_mean']:.4g}, largest {rep['distance_max']:.4g}; total squared distance {rep['total_first']:.6g} -> {rep['total_last']:.6g}")
    binding = dict(binding, k=np.int64(args.select_guides), samples=np.int64(args.select_samples), iterations=np.int64(rep["iterations"]),
                   converged=np.bool_(rep["converged"]))
    return guides, binding


def simplified(args, strands):
    """--simplify: the strands with the joints within TOL of their chord dropped (scene/strand_simplify.py), and what that did."""
    from scene.strand_simplify import simplify_strands
    out, rep = simplify_strands(strands, args.simplify, device=None if args.device == "cpu" else args.device)
    print(f"Simplified strands (tol {args.simplify:g}): {rep['joints_after']} of {rep['joints_before']} joints kept ({rep['ratio']:.4f}); "
          f"{rep['ok']} of {rep['strands']} strands simplified, left alone: {rep['short']} short, {rep['long']} long, {rep['nonfinite']} not "
          f"finite; joints kept per strand {rep['kept_min']} to {rep['kept_max']}, mean {rep['kept_mean']:.4g}; at most {rep['rounds_max']} "
          f"rounds; largest deviation of a dropped joint {rep['largest_deviation']:.4g}; largest attribute deviation from linear: "
          + ", ".join(f"{v:.3g}" for v in rep["attr_deviation"]))
    return out


def write_formats(paths, formats, strands, colour):
    """One file per format of `formats` at paths[format] (data/strand_files.py)."""
    from data import strand_files as F
    for f in formats:
        if f == "hair":
            F.write_strands_cy(paths[f], strands)
        elif f == "usc":
            F.write_strands_usc(paths[f], strands)
        elif f == "npz":
            F.write_strands_npz(paths[f], strands)
        else:
            F.write_strands_ply(paths[f], strands, faces=(f == "ply_faces"), colour=colour)
        print(f"Saved {f}: {paths[f]}")


def main(argv=None):
    parser = ArgumentParser(description="Export the strands of a trained model as hair assets")
    parser.add_argument("--model_path", "-m", required=True, help="a strand model PLY, or a model directory")
    parser.add_argument("--source_path", "-s", default=None, help="capture whose head reconstruction gives the strand roots")
    parser.add_argument("--output", "-o", required=True, help="output path; the format's extension is appended")
    parser.add_argument("--format", action="append", choices=FORMATS, help="repeatable; default: hair")
    parser.add_argument("--points", type=int, default=100, help="points per strand; 0 = the joints themselves")
    parser.add_argument("--min_segments", type=int, default=1)
    parser.add_argument("--min_length", type=float, default=0.0)
    parser.add_argument("--max_root_distance", type=float, default=None)
    parser.add_argument("--colour", default="model", choices=["model", "strand"], help="vertex colours of the PLY outputs")
    parser.add_argument("--device", default="cuda", choices=["cuda", "cpu"], help="cuda: the HIP kernels; cpu: the numpy path")
    parser.add_argument("--interpolate", action="store_true", help="add a strand for every strand root, blended from the nearest exported strands")
    parser.add_argument("--roots", type=int, default=None, help="with --interpolate: take this many of the strand roots, evenly")
    parser.add_argument("--guides", type=int, default=4, help="with --interpolate: guides blended per root (1 to 8)")
    parser.add_argument("--max_guide_distance", type=float, default=None, help="with --interpolate: roots farther than this from every guide's root get no strand")
    parser.add_argument("--max_angle", type=float, default=60.0, help="with --interpolate: guides whose chord turns more than this many degrees from the nearest guide's are left out")
    parser.add_argument("--no_guides", action="store_true", help="with --interpolate: write the interpolated strands only")
    parser.add_argument("--resolve_head", action="store_true", help="push every strand out of the head, keeping its segments' lengths")
    parser.add_argument("--head_margin", type=float, default=0.0, help="with --resolve_head: keep the joints this far outside the head")
    parser.add_argument("--collide_iters", type=int, default=8, help="with --resolve_head: pushes per joint at most (1 to 32)")
    parser.add_argument("--head_sdf", default=None, help="with --resolve_head: the head's distance field; default: <source_path>/head_sdf.npz")
    parser.add_argument("--attach_roots", action="store_true", help="march every strand's root back to the head and prepend the new joints")
    parser.add_argument("--attach_margin", type=float, default=0.0, help="with --attach_roots: target distance above the head surface")
    parser.add_argument("--attach_step", type=float, default=None, help="with --attach_roots: march step length; default: half the field's spacing")
    parser.add_argument("--attach_max_steps", type=int, default=256, help="with --attach_roots: steps per strand at most (1 to 1024)")
    parser.add_argument("--attach_pull", type=float, default=1.0, help="with --attach_roots: weight of the pull toward the head")
    parser.add_argument("--attach_descent", type=float, default=0.25, help="with --attach_roots: least cosine between a step and the way down (above 0, at most 1)")
    parser.add_argument("--attach_max_distance", type=float, default=None, help="with --attach_roots: strands starting farther than this from the head stay as they are")
    parser.add_argument("--attach_field", default=None, help="with --attach_roots: the direction volume (an .npz of trace_strands.py --field) that steers the march")
    parser.add_argument("--attach_min_conf", type=float, default=0.5, help="with --attach_roots: least aligned mass the volume must have at a point to steer")
    parser.add_argument("--attach_scalp_distance", type=float, default=None, help="with --attach_roots: a landed root farther than this from every strand root is off the scalp; its strand is restored")
    parser.add_argument("--drop_unattached", action="store_true", help="with --attach_roots: drop the strands whose march failed (default: write them unchanged)")
    parser.add_argument("--smooth_strands", action="store_true", help="low-pass every strand (Taubin's lambda|mu filter, both ends pinned)")
    parser.add_argument("--smooth_iters", type=int, default=10, help="with --smooth_strands: lambda|mu sweep pairs (1 to 256)")
    parser.add_argument("--smooth_lambda", type=float, default=0.5, help="with --smooth_strands: the smoothing sweep's factor (above 0, at most 1)")
    parser.add_argument("--smooth_mu", type=float, default=-0.53, help="with --smooth_strands: the inflating sweep's factor (-1 to below -lambda; 0: none, the strands shrink)")
    parser.add_argument("--smooth_max_move", type=float, default=None, help="with --smooth_strands: no joint ends farther than this from where it was")
    parser.add_argument("--select_guides", type=int, default=None, metavar="K", help="pick K guide strands from the written strands by k-means, with a binding (1 to 65536)")
    parser.add_argument("--select_samples", type=int, default=16, help="with --select_guides: joints compared per strand (2 to 64)")
    parser.add_argument("--select_iters", type=int, default=10, help="with --select_guides: assignments at most (1 to 256)")
    parser.add_argument("--simplify", type=float, default=None, metavar="TOL", help="drop every joint within TOL (scene units) of the chord that replaces it; runs last")
    parser.add_argument("--dedupe", type=float, default=None, metavar="DIST", help="drop every strand whose joints all lie within DIST (scene units) of an earlier kept strand's")
    args = parser.parse_args(argv)
    if args.dedupe is not None:
        from scene.strand_dedupe import check_parameters as check_dedupe
        try:
            check_dedupe(args.dedupe)
        except ValueError as e:
            parser.exit(2, f"export_strands.py: --dedupe: {e}\n")
        if args.points <= 0:
            parser.exit(2, "export_strands.py: --dedupe compares strands joint by joint and needs a fixed number of points per strand: "
                           "--points M > 0 is needed (--points 0, the joints themselves, cannot be combined with it)\n")
    if args.select_guides is not None:
        from scene.strand_guides import check_parameters as check_select
        try:
            check_select(args.select_guides, args.select_samples, args.select_iters)
        except ValueError as e:
            parser.exit(2, f"export_strands.py: --select_guides: {e}\n")
        if args.points <= 0:
            parser.exit(2, "export_strands.py: --select_guides compares strands joint by joint and needs a fixed number of points per strand: "
                           "--points M > 0 is needed (--points 0, the joints themselves, cannot be combined with it)\n")
    if args.simplify is not None:
        from scene.strand_simplify import check_parameters as check_simplify
        try:
            check_simplify(args.simplify)
        except ValueError as e:
            parser.exit(2, f"export_strands.py: --simplify: {e}\n")
    field = None
    if args.smooth_strands:
        from scene.strand_smooth import check_parameters as check_smooth
        try:
            check_smooth(args.smooth_iters, args.smooth_lambda, args.smooth_mu, args.smooth_max_move)
        except ValueError as e:
            parser.exit(2, f"export_strands.py: --smooth_strands: {e}\n")
    if args.attach_roots:
        from scene.strand_attach import MAX_STEPS as ATTACH_MAX_STEPS
        for flag, value, good, words in (
                ("--attach_margin", args.attach_margin, np.isfinite(args.attach_margin) and args.attach_margin >= 0.0, "a finite distance >= 0"),
                ("--attach_step", args.attach_step, args.attach_step is None or (np.isfinite(args.attach_step) and args.attach_step > 0.0), "a finite length > 0"),
                ("--attach_max_steps", args.attach_max_steps, 1 <= args.attach_max_steps <= ATTACH_MAX_STEPS, f"1 to {ATTACH_MAX_STEPS}"),
                ("--attach_pull", args.attach_pull, np.isfinite(args.attach_pull) and args.attach_pull >= 0.0, "a finite weight >= 0"),
                ("--attach_descent", args.attach_descent, 0.0 < args.attach_descent <= 1.0, "above 0, at most 1"),
                ("--attach_max_distance", args.attach_max_distance, args.attach_max_distance is None or args.attach_max_distance >= 0.0, "a distance >= 0"),
                ("--attach_min_conf", args.attach_min_conf, np.isfinite(args.attach_min_conf), "a finite mass"),
                ("--attach_scalp_distance", args.attach_scalp_distance, args.attach_scalp_distance is None or args.attach_scalp_distance >= 0.0, "a distance >= 0"),
                ("--attach_field", args.attach_field, args.attach_field is None or os.path.exists(args.attach_field), "no such file")):
            if not good:
                parser.exit(2, f"export_strands.py: {flag} {value}: {words}\n")
        field = head_field_path(args)
        if field is None:
            parser.exit(2, "export_strands.py: --attach_roots needs the head's distance field and found none"
                           + (f" at {args.head_sdf}" if args.head_sdf is not None else
                              f" at {os.path.join(args.source_path, 'head_sdf.npz')}" if args.source_path is not None else " (no -s and no --head_sdf)")
                           + ": run head_sdf.py on the capture, or name a field with --head_sdf\n")
    if args.resolve_head:
        if not (np.isfinite(args.head_margin) and args.head_margin >= 0.0):
            parser.exit(2, f"export_strands.py: --head_margin {args.head_margin}: a finite distance >= 0\n")
        if not 1 <= args.collide_iters <= 32:
            parser.exit(2, f"export_strands.py: --collide_iters {args.collide_iters}: 1 to 32\n")
        field = head_field_path(args)
        if field is None:
            parser.exit(2, "export_strands.py: --resolve_head needs the head's distance field and found none"
                           + (f" at {args.head_sdf}" if args.head_sdf is not None else
                              f" at {os.path.join(args.source_path, 'head_sdf.npz')}" if args.source_path is not None else " (no -s and no --head_sdf)")
                           + ": run head_sdf.py on the capture, or name a field with --head_sdf\n")
    if args.interpolate and args.points == 0:
        parser.exit(2, "export_strands.py: --interpolate blends strands point by point and needs a fixed number of points per strand: "
                       "--points 0 (the joints themselves) cannot be combined with it\n")
    formats = list(dict.fromkeys(args.format or ["hair"]))
    from scene.strand_export import resample_strands
    from utils.system import model_ply
    ply = model_ply(args.model_path)
    model = load_strand_model(ply, args.source_path, device=args.device)
    print(f"Loaded {ply}: {model.endpoint_pairs.shape[0]} segments, {model.strands_info.n_strands} strands")
    result = resample_strands(model, points=args.points, min_segments=args.min_segments, min_length=args.min_length,
                              max_root_distance=args.max_root_distance, device=None if args.device == "cpu" else args.device)
    print(f"Strands: {model.strands_info.n_strands}, kept: {result.n_strands}, points: {result.points.shape[0]}"
          + (f" ({args.points} per strand)" if args.points else " (the joints)"))
    if args.attach_roots:
        result = attached(args, field, model, result)
    if args.smooth_strands:
        result = smoothed(args, result)
    if args.interpolate:
        result = interpolated(args, model, result)
    if args.resolve_head:
        result = resolved(args, field, result)
    if args.dedupe is not None:
        from hgs_runtime import HgsError
        try:
            result = deduplicated(args, result)
        except (ValueError, HgsError) as e:
            parser.exit(2, f"export_strands.py: --dedupe: {e}\n")
    paths = output_paths(args.output, formats)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    picked = None
    if args.select_guides is not None:
        try:
            picked = selected(args, result)
        except ValueError as e:
            parser.exit(2, f"export_strands.py: --select_guides: {e}\n")
    if args.simplify is not None:
        result = simplified(args, result)
    write_formats(paths, formats, result, args.colour)
    if picked is not None:
        guides, binding = picked
        if args.simplify is not None:                                              # the guides as they are written: chosen before, simplified with the rest
            from scene.strand_simplify import take_strands
            guides = take_strands(result, binding["guide_strand"])
        guide_paths = {f: "_guides".join(os.path.splitext(p)) for f, p in paths.items()}
        write_formats(guide_paths, formats, guides, args.colour)
        paths = dict(paths, **{f + "_guides": p for f, p in guide_paths.items()})
        paths["guide_binding"] = output_paths(args.output, ["npz"])["npz"][:-len(".npz")] + "_guide_binding.npz"
        np.savez(paths["guide_binding"], **binding)
        print(f"Saved guide binding: {paths['guide_binding']}")
    return result, paths


if __name__ == "__main__":
    main()
