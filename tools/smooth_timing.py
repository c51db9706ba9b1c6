#!/usr/bin/env python3
"""Times one smoothing of exported strands (scene/strand_smooth.py, csrc/hgs_strand_smooth.hip): --strands strands (10^5) of --points
points (100), each a gentle helix 2 mm a joint with a trained strand's jitter (sigma 0.3 mm) on every joint, the defaults (10 x lambda
0.5 | mu -0.53, no max_move); everything from seed 0.  After a warm-up of each path, in this one process: the kernel on its own
(device events around --repeats back-to-back launches on resident buffers, the time per launch; five such windows; median and spread
reported) at the defaults and at iters = 1 and iters = 50 -- the three figures separate the load / store cost from the cost per sweep;
the ragged leg: the same strands plus ONE strand of 1024 joints, which sizes the LDS slice, and with it the wavefronts a workgroup and a
CU hold, for the whole launch; the device path end to end (smooth_strands(device="cuda"): uploads, the kernel, results copied to host
arrays, lengths and the report; wall clock around a synchronised call, five calls) and the numpy path on the same inputs (wall clock;
--host-repeats runs).  Also checks that the two paths agree byte for byte.  --device-only skips the numpy path.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np


def scene(K, M, seed=0, extra=()):
    """A StrandExport of K strands of M points, and one more strand for every size in `extra`."""
    from scene.strand_export import StrandExport
    rng = np.random.default_rng(seed)

    def helices(k, m):
        t = 2e-3 * np.arange(m)[None, :]
        r, w, ph = rng.uniform(0.01, 0.03, (k, 1)), rng.uniform(20.0, 60.0, (k, 1)), rng.uniform(0.0, 6.28, (k, 1))
        curve = np.stack([r * np.cos(w * t + ph), r * np.sin(w * t + ph), np.broadcast_to(-0.8 * t, (k, m))], axis=2)
        return (rng.uniform(-0.1, 0.1, (k, 1, 3)) + curve + rng.normal(scale=3e-4, size=(k, m, 3))).astype(np.float32).reshape(-1, 3)

    parts, sizes = [helices(K, M)], [M] * K
    for m in extra:
        parts.append(helices(1, m))
        sizes.append(m)
    pts = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = off.shape[0] - 1
    return StrandExport(pts, np.zeros((pts.shape[0], 1), np.float32), off, np.arange(n, dtype=np.int64), np.zeros(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    from scene import strand_smooth as SS
    uniform, ragged = scene(args.strands, args.points), scene(args.strands, args.points, extra=(SS.MAX_JOINTS,))
    dev = {name: (torch.as_tensor(s.points, device="cuda"), torch.as_tensor(s.offsets, device="cuda"), SS.longest_eligible(s.offsets))
           for name, s in (("uniform", uniform), ("ragged", ragged))}

    def events(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out

    def window(fn):
        def run():
            for _ in range(args.repeats):
                fn()
        return events(run)[0] / args.repeats

    def kernel(name, iters=10):
        p, o, m = dev[name]
        return SS.smooth_device(p, o, iters=iters, max_joints=m)

    def e2e_s():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = SS.smooth_strands(uniform, device="cuda")
        return time.perf_counter() - t0, res

    def host_s():
        t0 = time.perf_counter()
        res = SS.smooth_strands(uniform)
        return time.perf_counter() - t0, res

    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    legs = {"kernel_ms": ("uniform", 10), "kernel_iters1_ms": ("uniform", 1), "kernel_iters50_ms": ("uniform", 50),
            "kernel_ragged_ms": ("ragged", 10)}
    for leg in legs.values():                                                      # warm-up of everything that follows
        events(lambda: kernel(*leg))
    e2e_s()
    times = {k: [] for k in legs}
    for _ in range(5):
        for k, leg in legs.items():
            times[k].append(window(lambda: kernel(*leg)))
    e2e = []
    for _ in range(5):
        t, (res, report) = e2e_s()
        e2e.append(t)
    P = int(uniform.points.shape[0])
    med = {k: float(np.median(v)) for k, v in times.items()}
    result = {"strands": args.strands, "points_per_strand": args.points, "iters": 10, "lam": 0.5, "mu": -0.53,
              "gpu": torch.cuda.get_device_name(0), "report": report, **{k: stats(v) for k, v in times.items()},
              "ms_per_sweep_pair_from_iters_1_and_50": round((med["kernel_iters50_ms"] - med["kernel_iters1_ms"]) / 49.0, 5),
              "ragged_over_uniform": round(med["kernel_ragged_ms"] / med["kernel_ms"], 3), "device_e2e_s": stats(e2e),
              "point_bytes_read_and_written": 24 * P,
              "point_traffic_gb_per_s_at_kernel_median": round(24 * P / (med["kernel_ms"] * 1e-3) / 1e9, 1)}
    if not args.device_only:
        host = []
        for _ in range(max(1, args.host_repeats)):
            t, (hres, hreport) = host_s()
            host.append(t)
        result["numpy_s"] = stats(host)
        result["paths_agree_bytewise"] = bool(res.points.tobytes() == hres.points.tobytes() and res.length.tobytes() == hres.length.tobytes()
                                              and report == hreport)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
