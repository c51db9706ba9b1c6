#!/usr/bin/env python3
"""Times one simplification of exported strands (scene/strand_simplify.py, csrc/hgs_strand_simplify.hip): --strands strands (10^5) of
--points points (100), helices 2 mm a joint (0.98 of a step around the axis, 0.199 along it) from random places and phases, in three legs
of radius -- 1 cm, 5 cm and straight -- at --tol 0.3 mm; everything from seed 0.  After a warm-up of each path, in this one process: the
kernel on its own (device events around --repeats back-to-back launches on resident buffers, the time per launch; five such windows;
median and spread reported) per leg, with the rounds it took and the joints it kept; the ragged leg: the 1 cm strands plus ONE strand of
1024 joints, which sizes the LDS slice, and with it the wavefronts a workgroup and a CU hold (W = 1), for the whole launch; the device
path end to end on the 1 cm leg (simplify_strands(device="cuda"): uploads, the kernel, the flags copied to the host, the compaction,
lengths and the report; wall clock around a synchronised call, five calls) and the numpy path on the same input (wall clock;
--host-repeats runs).  Also checks that the two paths agree byte for byte.  --device-only skips the numpy path.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np


def scene(K, M, radius, seed=0, extra=()):
    """A StrandExport of K helices of M points and radius `radius` (None: straight), and one more for every size in `extra`."""
    from scene.strand_export import StrandExport
    rng = np.random.default_rng(seed)

    def helices(k, m):
        t = 2e-3 * np.arange(m)[None, :]
        origin, ph = rng.uniform(-0.1, 0.1, (k, 1, 3)), rng.uniform(0.0, 6.28, (k, 1))
        if radius is None:
            curve = np.stack([0.98 * t * np.cos(ph), 0.98 * t * np.sin(ph), np.broadcast_to(-0.199 * t, (k, m))], axis=2)
        else:
            a = 0.98 * t / radius + ph
            curve = np.stack([radius * np.cos(a), radius * np.sin(a), np.broadcast_to(-0.199 * t, (k, m))], axis=2)
        return (origin + curve).astype(np.float32).reshape(-1, 3)

    parts, sizes = [helices(K, M)], [M] * K
    for m in extra:
        parts.append(helices(1, m))
        sizes.append(m)
    pts = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = off.shape[0] - 1
    attrs = rng.uniform(0.0, 1.0, (pts.shape[0], 5)).astype(np.float32)
    return StrandExport(pts, attrs, off, np.arange(n, dtype=np.int64), np.zeros(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--tol", type=float, default=3e-4)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    from scene import strand_simplify as SS
    scenes = {"radius_1cm": scene(args.strands, args.points, 0.01), "radius_5cm": scene(args.strands, args.points, 0.05),
              "straight": scene(args.strands, args.points, None), "ragged_1cm": scene(args.strands, args.points, 0.01, extra=(SS.MAX_JOINTS,))}
    dev = {name: (torch.as_tensor(s.points, device="cuda"), torch.as_tensor(s.offsets, device="cuda"), SS.longest_eligible(s.offsets))
           for name, s in scenes.items()}

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

    def kernel(name):
        p, o, m = dev[name]
        return SS.simplify_device(p, o, args.tol, max_joints=m)

    def e2e_s():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = SS.simplify_strands(scenes["radius_1cm"], args.tol, device="cuda")
        return time.perf_counter() - t0, res

    def host_s():
        t0 = time.perf_counter()
        res = SS.simplify_strands(scenes["radius_1cm"], args.tol)
        return time.perf_counter() - t0, res

    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    legs = {}
    for name in scenes:                                                            # warm-up of everything that follows, and what each leg does
        keep, status, rounds = events(lambda: kernel(name))[1]
        K = int(status.shape[0])
        legs[name] = {"strands": K, "joints": int(keep.shape[0]), "joints_kept": int(keep.sum()), "rounds_max": int(rounds.max()),
                      "rounds_mean": round(float(rounds.float().mean()), 3), "max_joints": dev[name][2]}
    e2e_s()
    times = {name: [] for name in scenes}
    for _ in range(5):
        for name in scenes:
            times[name].append(window(lambda: kernel(name)))
    e2e = []
    for _ in range(5):
        t, (res, report) = e2e_s()
        e2e.append(t)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for name in scenes:
        legs[name]["kernel_ms"] = stats(times[name])
    P = legs["radius_1cm"]["joints"]
    result = {"strands": args.strands, "points_per_strand": args.points, "tol": args.tol, "gpu": torch.cuda.get_device_name(0), "legs": legs,
              "ragged_over_uniform": round(med["ragged_1cm"] / med["radius_1cm"], 3), "report_radius_1cm": report, "device_e2e_s": stats(e2e),
              "bytes_read_and_written_per_launch": 13 * P,
              "traffic_gb_per_s_at_kernel_median_radius_1cm": round(13 * P / (med["radius_1cm"] * 1e-3) / 1e9, 1)}
    if not args.device_only:
        host = []
        for _ in range(max(1, args.host_repeats)):
            t, (hres, hreport) = host_s()
            host.append(t)
        result["numpy_s"] = stats(host)
        result["paths_agree_bytewise"] = bool(all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(res, hres)) and report == hreport)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
