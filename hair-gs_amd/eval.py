#!/usr/bin/env python3
"""Scores a saved model against the capture's ground-truth strands (reference eval.py, which fails: it passes compute_metrics
a `return_table=` keyword the function does not take).  Precision, recall, F1 and strand consistency at the four default
(distance, angle) pairs, bidirectional like the reference's call, printed as a metrics x thresholds table.
  python eval.py -s <capture with hair_eval_data.npz> -p <point_cloud.ply | model dir> [--device cuda|cpu] [--json out.json]
A model directory is read at its newest point_cloud/iteration_N (utils/system.py model_ply).  Only the reference's `-pt gs` loader is provided: a
1-element PLY is a Gaussian cloud (foreground means + longest axes), a 5-element PLY a strand model (its joints in strand
order); reference data/eval_data.py:174-186."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from argparse import ArgumentParser

import numpy as np


def load_eval_data_from_gaussians(path, device="cpu"):
    """reference data/eval_data.py:174-186: the oriented points of a saved Gaussian cloud or strand model (the SH degree is
    read off the file's f_rest properties)."""
    from loss.metrics import compute_eval_data_from_gs, compute_eval_data_from_hair_gs
    from scene.gaussian_model import GaussianModel
    from scene.hair_gaussian_model import HairGaussianModel
    from utils.ply import read_ply
    els = read_ply(path)
    attrs = els[0][1] if len(els) == 1 else dict(els).get("segment")
    if attrs is None:
        raise ValueError(f"{path}: neither a Gaussian cloud (1 element) nor a strand model (5 elements)")
    n_rest = sum(1 for n in attrs.dtype.names if n.startswith("f_rest_"))
    sh_degree = int(round(np.sqrt((n_rest + 3) / 3))) - 1
    if len(els) == 1:
        gs = GaussianModel(sh_degree, device=device)
        gs.load_ply(path)
        return compute_eval_data_from_gs(gs)
    gs = HairGaussianModel(sh_degree, device=device)
    gs.load_ply(path)
    return compute_eval_data_from_hair_gs(gs, compute_edges=True)


def format_table(metrics, labels):
    rows = [["metric"] + list(labels)]
    rows += [[k] + [f"{float(x):.6f}" for x in v] + ["-"] * (len(labels) - len(v)) for k, v in metrics.items()]   # ("-": not computed, e.g. strand consistency without strand ids)
    w = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    return "\n".join("  ".join(cell.ljust(w[c]) if c == 0 else cell.rjust(w[c]) for c, cell in enumerate(r)) for r in rows)


def main(argv=None):
    parser = ArgumentParser(description="Evaluation of reconstruction results")
    parser.add_argument("--source_data_path", "-s", required=True, help="capture directory holding hair_eval_data.npz")
    parser.add_argument("--pred_data_path", "-p", required=True, help="a saved model PLY, or a model directory")
    parser.add_argument("--pred_data_type", "-pt", default="gs", choices=["gs"], help="type of the prediction data")
    parser.add_argument("--device", default="cuda", help="cuda: the HIP kernels; cpu: the CPU path (scipy cKDTree)")
    parser.add_argument("--json", default=None, help="also write the metrics to this file")
    args = parser.parse_args(argv)
    from data.eval_data import load_hair_eval_data_npz
    from loss.metrics import compute_metrics
    from utils.system import model_ply
    gt_path = os.path.join(args.source_data_path, "hair_eval_data.npz")
    gt = load_hair_eval_data_npz(gt_path)
    print(f"Loaded GT data from {gt_path}")
    ply = model_ply(args.pred_data_path)
    pred = load_eval_data_from_gaussians(ply, device="cpu")     # (the same oriented points for either device's metrics)
    print(f"Loaded evaluation data from {ply}")
    metrics, labels = compute_metrics(pred, gt, bidirectional=True, device=None if args.device == "cpu" else args.device)
    print(format_table(metrics, labels))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"metrics": {k: [float(x) for x in v] for k, v in metrics.items()}, "thresholds": labels,
                       "device": args.device, "pred": ply}, fh, indent=1)
    return metrics, labels


if __name__ == "__main__":
    main()
