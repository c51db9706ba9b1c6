#!/usr/bin/env python3
"""Times one guide selection (scene/strand_guides.py, csrc/hgs_guides.hip): --strands strands (10^5) of --points points (100) generated
as clumps -- --locks locks (2000) of wavy strands around a lock centre line, a per-strand offset of a few millimetres and a jitter of
0.3 mm on every joint -- K = 1000 clusters, 16 samples, at most 10 iterations, and a second leg at K = 10^4; everything from seed 0.
After a warm-up of each path, in this one process: each of the three kernels on its own (device events around --repeats back-to-back
launches on resident buffers, the time per launch; five such windows; median and spread reported), the assignment's achieved float64
rate from its 9*N*K*S operations (3 subtractions, 3 products, 3 additions per sampled joint and centroid; no fused operation: the
contract rounds each), and, as the yardstick a user would otherwise write, torch.cdist in float64 on the same features followed by
argmin, on the same device and in the same windows, with the share of strands on which the two agree (cdist is free to round
differently; the kernel's labels are the contract's).  Then the device path end to end (select_guides(device="cuda"): uploads, the
loop with its one word read per iteration, the stable sorts, the results copied to host arrays, the guide strands and the report;
wall clock around a synchronised call, three calls) and the numpy path (wall clock, one run) on the first --host-strands strands
(10^4: at 10^5 one assignment alone is 1.6e9 differences squared in numpy, minutes for the ten), with a check that the two paths
agree byte for byte there.  --device-only skips the numpy path.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np


def scene(N, M, locks, seed=0):
    """A StrandExport of N strands of M points in `locks` clumps, strand i in lock i % locks."""
    from scene.strand_export import StrandExport
    rng = np.random.default_rng(seed)
    t = 2e-3 * np.arange(M)[None, :]
    root = rng.normal(size=(locks, 3))
    root = 0.1 * root / np.linalg.norm(root, axis=1, keepdims=True)
    r, w, ph = rng.uniform(0.005, 0.02, (locks, 1)), rng.uniform(10.0, 40.0, (locks, 1)), rng.uniform(0.0, 6.28, (locks, 1))
    line = root[:, None, :] + np.stack([r * np.cos(w * t + ph), r * np.sin(w * t + ph), np.broadcast_to(-0.9 * t, (locks, M))], axis=2)
    lock = np.arange(N) % locks
    pts = line[lock] + rng.normal(scale=2e-3, size=(N, 1, 3)) + rng.normal(scale=3e-4, size=(N, M, 3))
    pts = pts.astype(np.float32).reshape(-1, 3)
    return StrandExport(pts, np.zeros((pts.shape[0], 1), np.float32), np.arange(N + 1, dtype=np.int64) * M, np.arange(N, dtype=np.int64), np.zeros(N))


def head(strands, n, M):
    from scene.strand_export import StrandExport
    return StrandExport(strands.points[:n * M], strands.attrs[:n * M], strands.offsets[:n + 1], strands.strand_ids[:n], strands.length[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--locks", type=int, default=2000)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--k", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-strands", type=int, default=10000)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    from scene import strand_guides as SG
    N, M = args.strands, args.points
    S = min(args.samples, M)
    strands = scene(N, M, args.locks)
    pts = torch.as_tensor(strands.points, device="cuda")
    status = torch.zeros(N, dtype=torch.int32, device="cuda")
    joints = torch.as_tensor(SG.sample_joints(M, S), device="cuda")
    feats = pts.view(N, M, 3)[:, joints].to(torch.float64).reshape(N, 3 * S).contiguous()

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

    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    result = {"strands": N, "points_per_strand": M, "locks": args.locks, "samples": S, "iters": args.iters, "gpu": torch.cuda.get_device_name(0),
              "repeats_per_window": args.repeats, "legs": {}}
    for K in args.k:
        seeds = torch.as_tensor(SG.seed_strands(N, K), device="cuda")
        cent = feats[seeds].reshape(K, S, 3).contiguous()
        label, d2 = SG.assign_device(pts, N, M, S, status, cent)
        order, start = SG.member_list(label, K)
        work = cent.clone()
        changed = torch.zeros(1, dtype=torch.int32, device="cuda")
        legs = {"assign_ms": lambda: SG.assign_device(pts, N, M, S, status, cent, label, changed),
                "update_ms": lambda: SG.update_device(pts, N, M, S, order, start, work),
                "pick_ms": lambda: SG.pick_device(N, K, order, start, d2),
                "member_list_ms": lambda: SG.member_list(label, K),
                "cdist_argmin_ms": lambda: torch.cdist(feats, cent.view(K, 3 * S)).argmin(dim=1)}
        for fn in legs.values():                                                    # warm-up of everything that follows
            events(fn)
        times = {k: [] for k in legs}
        for _ in range(5):
            for k, fn in legs.items():
                times[k].append(window(fn))
        yard = torch.cdist(feats, cent.view(K, 3 * S)).argmin(dim=1)
        ops = 9 * N * K * S
        med = float(np.median(times["assign_ms"]))
        leg = {k: stats(v) for k, v in times.items()}
        leg.update({"assign_f64_operations": ops, "assign_f64_gops_per_s_at_median": round(ops / (med * 1e-3) / 1e9, 1),
                    "assign_over_cdist_argmin": round(med / float(np.median(times["cdist_argmin_ms"])), 3),
                    "labels_equal_to_cdist_argmin": round(float((yard == label.to(torch.int64)).double().mean()), 6),
                    "clusters_with_members_after_first_assignment": int(torch.count_nonzero(start[1:] - start[:-1]))})
        del yard
        e2e = []
        SG.select_guides(strands, K, S, args.iters, device="cuda")
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = SG.select_guides(strands, K, S, args.iters, device="cuda")
            e2e.append(time.perf_counter() - t0)
        leg["device_e2e_s"] = stats(e2e)
        leg["report"] = res[2]
        result["legs"][f"k{K}"] = leg
    if not args.device_only:
        n, K = min(args.host_strands, N), args.k[0]
        small = head(strands, n, M)
        t0 = time.perf_counter()
        host = SG.select_guides(small, K, S, args.iters)
        host_s = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = SG.select_guides(small, K, S, args.iters, device="cuda")
        dev_s = time.perf_counter() - t0
        same = all(a.tobytes() == b.tobytes() for a, b in zip(host[0], dev[0])) and host[2] == dev[2] and \
            all(host[1][key].tobytes() == dev[1][key].tobytes() for key in host[1])
        result["numpy"] = {"strands": n, "k": K, "numpy_s": round(host_s, 3), "device_e2e_s_same_input": round(dev_s, 3),
                           "iterations": host[2]["iterations"], "paths_agree_bytewise": bool(same)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
