"""One strand-growth event (HairTopologyMixin.growing) at a merged-model size: 10^5 strands of 4 segments (4 10^5 segments),
growth_averaging_points 3, degree-3 f_rest, 2000 reference roots (a scalp's vertices, which orient the strands in the re-walk).
Reports the event end to end on the device form (plan + scan + fill + cat_segments + the re-walk of compute_strands_info) and its
three phases, the same event on the host form (HGS_GROWTH=host: numpy), and the two growth kernels alone from a
`rocprofv3 --kernel-trace --stats` run of this script in a child process.  Medians of --reps events, each on a fresh model,
after one warm-up event.  Prints one JSON line.
  python tools/growth_timing.py [--strands 100000] [--segments 4] [--reps 5] [--no-rocprof]"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]

import numpy as np

KERNELS = ("grow_plan_kernel", "grow_fill_kernel")


def model(S, n_seg):
    import torch
    from arguments import OptimizationParams
    from scene.hair_gaussian_model import HairGaussianModel
    from synthetic import strand_polylines
    pts = strand_polylines(S, n_seg, seed=3).astype(np.float32)
    m = HairGaussianModel.from_strands(pts, device="cuda", sh_degree=3, ref_strand_root=pts[::max(1, S // 2000), 0])
    m.training_setup(OptimizationParams())
    with torch.no_grad():
        m._features_rest.normal_(0.0, 0.05)
    m.compute_strands_info()
    return m


def events(S, n_seg, reps, form):
    import torch
    os.environ["HGS_GROWTH"] = form
    ts, grown = [], None
    for i in range(reps + 1):
        m = model(S, n_seg)
        info = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.growing(info, strands_info_is_current=True)
        torch.cuda.synchronize()
        if i:
            ts.append(time.perf_counter() - t0)
        grown = info["grow"]
    return statistics.median(ts), grown


def phases(S, n_seg, reps):
    """Median ms of the device form's three phases: decisions + new rows (_grow_device: two launches, the scan, one sync),
    cat_segments, the re-walk (compute_strands_info)."""
    import torch
    os.environ["HGS_GROWTH"] = "device"
    ts = []
    for i in range(reps + 1):
        m = model(S, n_seg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, new = m._grow_device(int(m.training_args.growth_averaging_points), 0.002)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m.cat_segments(*new)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        m.compute_strands_info()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if i:
            ts.append((t1 - t0, t2 - t1, t3 - t2))
    med = [statistics.median(x) for x in zip(*ts)]
    return {k: round(v * 1e3, 2) for k, v in zip(("plan_scan_fill_ms", "cat_segments_ms", "rewalk_ms"), med)}


def kernel_stats(S, n_seg, reps):
    """Mean time per launch of the two growth kernels from rocprofv3's kernel statistics (child process: this script, device form)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="growth_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "growth", "--", sys.executable, os.path.abspath(__file__),
           "--strands", str(S), "--segments", str(n_seg), "--reps", str(reps), "--device-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"error": f"rocprofv3 exit {r.returncode}", "tail": (r.stdout + r.stderr)[-800:]}
    res = {}
    found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        res["files"] = [os.path.relpath(p, out) for p in glob.glob(os.path.join(out, "**", "*"), recursive=True)][:20]
    for path in found:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in KERNELS:
                    if k in name:
                        try:
                            res[k] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2)}
                        except (KeyError, ValueError):
                            res[k] = {"columns": list(row)}
    shutil.rmtree(out, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--device-only", action="store_true", help=argparse.SUPPRESS)   # (the rocprofv3 child)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "growth_timing.py measures the GPU path: it needs the GPU"
    if a.device_only:
        events(a.strands, a.segments, a.reps, "device")
        return
    dev_s, grown = events(a.strands, a.segments, a.reps, "device")
    host_s, grown_h = events(a.strands, a.segments, max(1, a.reps // 2), "host")
    res = {"strands": a.strands, "segments": a.strands * a.segments, "grown": grown, "grown_host": grown_h,
           "event_device_ms": round(dev_s * 1e3, 2), "event_host_ms": round(host_s * 1e3, 2), "reps": a.reps,
           "device_phases": phases(a.strands, a.segments, a.reps)}
    if not a.no_rocprof:
        res["kernels"] = kernel_stats(a.strands, a.segments, a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
