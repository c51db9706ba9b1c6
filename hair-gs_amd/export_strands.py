#!/usr/bin/env python3
"""Exports the strands of a trained strand model (Stage II / III) as hair assets other tools read: the step behind train.py /
merge.py that the reference leaves to scripts/convert_output.py (MeshLab PLYs of the joints only).
  python export_strands.py -m <model dir | strand PLY> [-s <capture>] -o <out> --format hair|usc|ply_edges|ply_faces|npz [--format ...]
                           [--points 100] [--min_segments 1] [--min_length 0] [--max_root_distance D] [--colour model|strand]
                           [--device cuda|cpu]
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
the file has none).  --colour strand gives the PLYs one hue per strand instead of the model's colours."""
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
    args = parser.parse_args(argv)
    formats = list(dict.fromkeys(args.format or ["hair"]))
    from data import strand_files as F
    from scene.strand_export import resample_strands
    from utils.system import model_ply
    ply = model_ply(args.model_path)
    model = load_strand_model(ply, args.source_path, device=args.device)
    print(f"Loaded {ply}: {model.endpoint_pairs.shape[0]} segments, {model.strands_info.n_strands} strands")
    result = resample_strands(model, points=args.points, min_segments=args.min_segments, min_length=args.min_length,
                              max_root_distance=args.max_root_distance, device=None if args.device == "cpu" else args.device)
    print(f"Strands: {model.strands_info.n_strands}, kept: {result.n_strands}, points: {result.points.shape[0]}"
          + (f" ({args.points} per strand)" if args.points else " (the joints)"))
    paths = output_paths(args.output, formats)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    for f in formats:
        if f == "hair":
            F.write_strands_cy(paths[f], result)
        elif f == "usc":
            F.write_strands_usc(paths[f], result)
        elif f == "npz":
            F.write_strands_npz(paths[f], result)
        else:
            F.write_strands_ply(paths[f], result, faces=(f == "ply_faces"), colour=args.colour)
        print(f"Saved {f}: {paths[f]}")
    return result, paths


if __name__ == "__main__":
    main()
