#!/usr/bin/env python3
"""Times one strand export (scene/strand_export.py, csrc/hgs_export.hip): a 10^5-strand x 80-segment model
(synthetic.make_strand_model, seed 0) resampled to 100 points per strand.  After a warm-up of each path, in this one process:
the device path end to end (resample_strands(device="cuda"): attribute table, both kernels, the filters' host step, results copied
to host arrays; wall clock around a synchronised call, five calls), each kernel on its own (device events around --repeats
back-to-back launches, the time per launch; five such windows, the two kernels alternating; median and spread reported) and the
numpy path on the same model (wall clock; --host-repeats runs).  Also checks that
the two paths agree on that model.  --device-only skips the numpy path (for a kernel-trace run).  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--segments", type=int, default=80)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import synthetic
    import torch
    from scene import strand_export as X
    m = synthetic.make_strand_model(args.strands, args.segments, seed=0, device="cuda")
    m.compute_strands_info()
    S, M = m.strands_info.n_strands, args.points
    off, rows, seg = X._device_tables(m)
    ep = m._endpoints.detach().contiguous()
    attr = X.export_attributes(m)
    kept = torch.arange(S, dtype=torch.int32, device="cuda")

    def events(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out

    def e2e_s():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = X.resample_strands(m, points=M, device="cuda")
        return time.perf_counter() - t0, res

    def host_s():
        t0 = time.perf_counter()
        res = X.resample_strands(m, points=M)
        return time.perf_counter() - t0, res

    _, (cum, _, _) = events(lambda: X.arclen_device(off, rows, ep))          # warm-up of everything that follows
    events(lambda: X.resample_device(off, rows, seg, ep, attr, cum, kept, M))
    e2e_s()
    arclen, resample, e2e = [], [], []

    def window(fn):
        def run():
            for _ in range(args.repeats):
                fn()
        return events(run)[0] / args.repeats

    for _ in range(5):
        arclen.append(window(lambda: X.arclen_device(off, rows, ep)))
        resample.append(window(lambda: X.resample_device(off, rows, seg, ep, attr, cum, kept, M)))
    for _ in range(5):
        t, dev = e2e_s()
        e2e.append(t)
    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    total = int(rows.shape[0])
    # bytes the kernels must move at least: rows + vertices read once and cum written; cum, rows, vertices and attributes of two
    # joints read per sample (cached in practice) and the sample written
    result = {"strands": S, "segments": total, "points_per_strand": M, "gpu": torch.cuda.get_device_name(0),
              "arclen_kernel_ms": stats(arclen), "resample_kernel_ms": stats(resample), "device_e2e_s": stats(e2e),
              "arclen_min_bytes": total * (16 + 12 + 8) + S * 16, "resample_written_bytes": S * M * (12 + 4 * int(attr.shape[1]))}
    if not args.device_only:
        host_s()
        host = []
        for _ in range(args.host_repeats):
            t, hres = host_s()
            host.append(t)
        result["numpy_s"] = stats(host)
        result["paths_agree_bitwise"] = bool(all(x.tobytes() == y.tobytes() for x, y in zip(dev, hres)))
        result["device_slowest_below_numpy_fastest"] = bool(max(e2e) < min(host))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
