#!/usr/bin/env python3
"""Scores a trained model's renders against its capture's images, view by view: PSNR, SSIM, L1, PSNR over the hair mask, the
foreground mask's IoU, and the orientation map's mean angle error, share within 10 / 20 degrees and training loss term
(definitions: loss/image_metrics.py).  Works on any capture Scene loads, with or without ground-truth strands.
  python view_metrics.py -s <capture> -m <model dir> [--batch 8] [--per_view] [--json out.json]
The model is read at its newest point_cloud/iteration_N, as render.py reads it.  Every camera is scored, keyed by image_name and
listed in name order; views of one size go through the kernel --batch at a time.  Prints a metrics x (mean, min, max) table, and
every view's row with --per_view.  --json writes {"model", "iteration", "views": {name: {...}}, "mean": {...}}; inf and None are
written as null, and a mean skips the views whose value is None.
These are fit scores on the training views: the capture has no held-out split (neither the reference nor this port reads
--eval)."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser


def parse_args(argv=None):
    from arguments import GeneralParams, ModelParams, get_combined_args
    parser = ArgumentParser(description="Image metrics of a trained model on its capture's views")
    ModelParams(parser, sentinel=True)
    GeneralParams(parser)
    parser.add_argument("--batch", type=int, default=8, help="views of one size per kernel launch")
    parser.add_argument("--per_view", action="store_true", help="also print every view's row")
    parser.add_argument("--json", default=None, help="also write the metrics to this file")
    if argv is not None:
        sys.argv = [sys.argv[0]] + list(argv)
    args = get_combined_args(parser)
    for group in (ModelParams, GeneralParams):   # no cfg_args next to the model: class defaults
        for name, default, _ in group.FIELDS:
            if getattr(args, name, None) is None:
                setattr(args, name, default() if callable(default) else default)
    args.json = getattr(args, "json", None)          # (get_combined_args drops options left at None)
    if args.batch < 1:
        parser.error("--batch must be >= 1")
    return args


def mean_of_views(views):
    """Per metric, the mean over the views whose value is not None (None where every view has None)."""
    from loss.image_metrics import METRICS
    out = {}
    for k in METRICS:
        vals = [v[k] for v in views.values() if v.get(k) is not None]
        out[k] = math.fsum(vals) / len(vals) if vals else None
    return out


def summarize(model, iteration, per_view):
    """The driver's result: the metric keys of every view in name order, and their mean."""
    from loss.image_metrics import METRICS
    views = {n: {k: m[k] for k in METRICS} for n, m in sorted(per_view.items())}
    return {"model": model, "iteration": iteration, "views": views, "mean": mean_of_views(views)}


def _jsonable(x):
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, float) and not math.isfinite(x):
        return None
    return x


def to_json(result):
    return json.dumps(_jsonable(result), allow_nan=False, indent=1)


def _fmt(x):
    return "-" if x is None else f"{x:.6f}"


def format_table(result, per_view=False):
    from loss.image_metrics import METRICS
    rows = [["metric", "mean", "min", "max"]]
    for k in METRICS:
        vals = [v[k] for v in result["views"].values() if v[k] is not None]
        rows.append([k, _fmt(result["mean"][k]), _fmt(min(vals) if vals else None), _fmt(max(vals) if vals else None)])
    text = [rows]
    if per_view:
        pv = [["view"] + list(METRICS)] + [[n] + [_fmt(v[k]) for k in METRICS] for n, v in result["views"].items()]
        text.append(pv)
    out = []
    for t in text:
        w = [max(len(r[c]) for r in t) for c in range(len(t[0]))]
        out.append("\n".join("  ".join(cell.ljust(w[c]) if c == 0 else cell.rjust(w[c]) for c, cell in enumerate(r)) for r in t))
    return "\n\n".join(out)


def main(argv=None):
    args = parse_args(argv)
    pc = os.path.join(args.model_path, "point_cloud")
    if not os.path.isdir(pc) or not any(d.startswith("iteration_") for d in os.listdir(pc)):
        raise SystemExit(f"view_metrics.py: {args.model_path} holds no trained model (point_cloud/iteration_N)")
    import torch
    from loss.image_metrics import score_cameras
    from scene import Scene
    from utils.general import safe_state
    safe_state(getattr(args, "quiet", False))
    with torch.no_grad():
        scene = Scene(args, shuffle=False)
        per_view = score_cameras(scene.getCameras(), scene.gaussians, batch=args.batch)
    result = summarize(args.model_path, scene.loaded_iter, per_view)
    print(f"{args.model_path} at iteration {scene.loaded_iter}: {len(per_view)} view(s) (fit scores on the training views)")
    print(format_table(result, args.per_view))
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(to_json(result) + "\n")
    return result


if __name__ == "__main__":
    main()
