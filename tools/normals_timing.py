#!/usr/bin/env python3
"""Times the point-cloud normals (utils/normals.py, csrc/hgs_normals.hip) on strand vertices (synthetic.strand_polylines, seed 0):
10^6 vertices (10^4 strands x 100, the size of a full USC-HairSalon model) and 2 x 10^5, K = 50.  For each size, after one warm-up
of each path, host and device alternate three times in this one process: host seconds (the cKDTree path, 16 workers), device end
to end (host float64 array in, host array out, synchronised) and device kernels only (events around the C call).  Also reports,
from the device's own neighbour lists, how many candidates per point a walk of the grid examines (every point of every cell that
the box of the final K-th distance touches: the lower bound of what the kernel reads).  --device-only skips the host path (for a
rocprofv3 --kernel-trace --stats run).  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np

K = 50


def grid_level(N, K):
    """normals_level of csrc/hgs_normals.hip."""
    L = 1
    while L < 7 and (1 << (3 * (L + 1))) * K <= 4 * N:
        L += 1
    return L


def candidates_per_point(p, nb):
    """Mean and largest number of points in the cells that the final search box of a point touches."""
    N = p.shape[0]
    G = 1 << grid_level(N, K)
    mn = p.min(axis=0)
    inv = G / (p.max(axis=0) - mn).max()
    cell = np.clip(((p - mn) * inv).astype(np.int64), 0, G - 1)
    counts = np.zeros((G, G, G), dtype=np.int64)
    np.add.at(counts, (cell[:, 0], cell[:, 1], cell[:, 2]), 1)
    sat = np.zeros((G + 1, G + 1, G + 1), dtype=np.int64)
    sat[1:, 1:, 1:] = counts.cumsum(0).cumsum(1).cumsum(2)
    r = np.sqrt(((p[nb[:, -1]] - p) ** 2).sum(axis=1))[:, None]
    lo = np.clip(((p - r - mn) * inv).astype(np.int64), 0, G - 1)
    hi = np.clip(((p + r - mn) * inv).astype(np.int64), 0, G - 1) + 1
    tot = (sat[hi[:, 0], hi[:, 1], hi[:, 2]] - sat[lo[:, 0], hi[:, 1], hi[:, 2]] - sat[hi[:, 0], lo[:, 1], hi[:, 2]]
           - sat[hi[:, 0], hi[:, 1], lo[:, 2]] + sat[lo[:, 0], lo[:, 1], hi[:, 2]] + sat[lo[:, 0], hi[:, 1], lo[:, 2]]
           + sat[hi[:, 0], lo[:, 1], lo[:, 2]] - sat[lo[:, 0], lo[:, 1], lo[:, 2]])
    return {"grid": G, "occupied_cells": int((counts > 0).sum()), "mean": round(float(tot.mean()), 1), "max": int(tot.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import synthetic
    import torch
    import hgs_runtime as rt
    from utils.normals import estimate_pointcloud_normals, estimate_pointcloud_normals_device
    L = rt.lib()
    result = {"K": K, "repeats": args.repeats, "sizes": {}}
    for n_strands in (2000, 10000):
        p = synthetic.strand_polylines(n_strands, 99, seed=0).reshape(-1, 3).astype(np.float64)
        N = p.shape[0]
        pd = torch.from_numpy(p).cuda()
        out = torch.empty((N, 3), dtype=torch.float64, device="cuda")
        scratch = torch.empty(int(L.hgs_pointcloud_normals_scratch_bytes(N, K)), dtype=torch.uint8, device="cuda")

        def kernels_ms():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            rt.check(L.hgs_pointcloud_normals(rt.current_stream(), N, K, rt.ptr(pd), rt.ptr(out), None, rt.ptr(scratch), scratch.numel()))
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])

        def e2e_s():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            estimate_pointcloud_normals(p, K, device="cuda")
            return time.perf_counter() - t0

        def host_s():
            t0 = time.perf_counter()
            estimate_pointcloud_normals(p, K)
            return time.perf_counter() - t0

        kernels_ms(), e2e_s()                                   # warm-up
        if not args.device_only:
            host_s()
        host, e2e, kern = [], [], []
        for _ in range(args.repeats):
            if not args.device_only:
                host.append(host_s())
            e2e.append(e2e_s())
            kern.append(kernels_ms())
        _, nb = estimate_pointcloud_normals_device(pd, K, return_neighbors=True)
        entry = {"device_e2e_s": [round(t, 4) for t in e2e], "device_kernels_ms": [round(t, 3) for t in kern],
                 "candidates_per_point": candidates_per_point(p, nb.cpu().numpy().astype(np.int64))}
        if host:
            entry["host_s"] = [round(t, 3) for t in host]
            entry["device_slowest_below_host_fastest"] = bool(max(e2e) < min(host))
        result["sizes"][str(N)] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
