"""End-to-end time of compute_metrics on the CPU path and on the GPU (csrc/hgs_metrics.hip): numpy in -> dict out, uploads and
host preparation included; median of 5 after one warm-up call, at 200 k points (2 000 straight strands) and 1 M points
(10 000 curly strands), 100 points per strand, prediction = GT size, bidirectional, strand ids on both sides.  Prints one JSON line.
  python tools/metrics_timing.py [--sizes 2000:0,10000:1] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]

import numpy as np


def side(pts, dtype):
    from loss.metrics import HairEvalData
    d = (pts[:, 1:] - pts[:, :-1]).astype(dtype)
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return HairEvalData(pts[:, :-1].reshape(-1, 3), d.reshape(-1, 3), np.repeat(np.arange(pts.shape[0]), pts.shape[1] - 1))


def timed(fn, reps):
    import torch
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000:0,10000:1", help="strands:curly pairs")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from loss.metrics import compute_metrics
    from synthetic import strand_polylines
    assert torch.cuda.is_available(), "metrics_timing.py measures the GPU path: it needs the GPU"
    res = {"reps": a.reps}
    for item in a.sizes.split(","):
        S, curly = (int(x) for x in item.split(":"))
        gt = side(strand_polylines(S, 100, seed=7, curly=bool(curly)), np.float64)
        pred = side(strand_polylines(S, 100, seed=8, curly=bool(curly)), np.float32)
        cpu_s, cpu = timed(lambda: compute_metrics(pred, gt, bidirectional=True), a.reps)
        gpu_s, gpu = timed(lambda: compute_metrics(pred, gt, bidirectional=True, device="cuda"), a.reps)
        same = cpu[1] == gpu[1] and cpu[0].keys() == gpu[0].keys() and all(
            cpu[0][k].dtype == gpu[0][k].dtype and cpu[0][k].tobytes() == gpu[0][k].tobytes() for k in cpu[0])
        res[f"{len(gt.points)}"] = {"strands": S, "curly": bool(curly), "cpu_s": round(cpu_s, 4), "gpu_s": round(gpu_s, 4),
                                    "speedup": round(cpu_s / gpu_s, 1), "equal": bool(same)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
