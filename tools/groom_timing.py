#!/usr/bin/env python3
"""Times one groom interpolation (scene/groom.py, csrc/hgs_groom.hip): --roots roots (10^5) on a sphere cap of 10 cm against --guides
guides (10^4) of --points points (100) with --attrs attributes (5), k = --k (4), no distance limit, max_angle 60; everything from
seed 0.  After a warm-up of each path, in this one process: each kernel on its own (device events around --repeats back-to-back
launches, the time per launch; five such windows, the two kernels alternating; median and spread reported), the neighbour kernel alone
at every size of --search-roots (10^3 and 10^6 beside the main size: its brute force is N K float64 distance evaluations, and these
figures decide whether small N needs the candidate range split over workgroups and large N K a cell grid), the device path end to end
(interpolate_strands(device="cuda"): uploads, both kernels, the kept list, results copied to host arrays and their lengths; wall clock
around a synchronised call, five calls) and the numpy path on the same inputs (wall clock; --host-repeats runs).  Also checks that the
two paths agree bit for bit.  --device-only skips the numpy path.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np


def scene(n_roots, n_guides, M, C, seed=0):
    """(guides StrandExport, roots float64 [n_roots, 3]): guide roots and roots on the upper cap of a 10 cm sphere, guides falling 20 cm
    along the normal and then down, with a wave per guide."""
    from scene.strand_export import StrandExport
    rng = np.random.default_rng(seed)

    def cap(n):
        v = rng.normal(size=(n, 3))
        v[:, 2] = np.abs(v[:, 2])
        return 0.1 * v / np.linalg.norm(v, axis=1, keepdims=True)

    g0, roots = cap(n_guides), cap(n_roots)
    s = np.linspace(0.0, 1.0, M)[None, :, None]
    wave = 0.01 * np.sin(6.0 * s + rng.uniform(0, 6.28, size=(n_guides, 1, 1))) * rng.normal(size=(n_guides, 1, 3))
    gp = (g0[:, None, :] + 0.2 * (0.6 * s * g0[:, None, :] / 0.1 + 0.8 * s * s * np.array([0.0, 0.0, -1.0])) + s * wave).astype(np.float32)
    ga = rng.uniform(0, 1, size=(n_guides, M, C)).astype(np.float32)
    guides = StrandExport(gp.reshape(-1, 3), ga.reshape(-1, C), np.arange(n_guides + 1, dtype=np.int64) * M, np.arange(n_guides, dtype=np.int64),
                          np.zeros(n_guides))
    return guides, roots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, default=100000)
    ap.add_argument("--guides", type=int, default=10000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--attrs", type=int, default=5)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--search-roots", type=int, nargs="*", default=[1000, 1000000])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    from scene import groom as G
    guides, roots = scene(args.roots, args.guides, args.points, args.attrs)
    gp, ga = G.guide_arrays(guides)
    max_d2, cos_max = G.search_parameters(None, 60.0)
    gp_d, ga_d, roots_d = (torch.as_tensor(a, device="cuda") for a in (gp, ga, roots))

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

    def e2e_s(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = G.interpolate_strands(guides, roots[:n], k=args.k, max_angle=60.0, device="cuda")
        return time.perf_counter() - t0, res

    def host_s(n):
        t0 = time.perf_counter()
        res = G.interpolate_strands(guides, roots[:n], k=args.k, max_angle=60.0)
        return time.perf_counter() - t0, res

    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    _, (idx, _, w, count) = events(lambda: G.search_device(gp_d, roots_d, args.k, max_d2, cos_max))      # warm-up of everything that follows
    kept = torch.nonzero(count > 0).reshape(-1).to(torch.int32)
    events(lambda: G.blend_device(gp_d, ga_d, roots_d, idx, w, kept))
    e2e_s(args.roots)
    search, blend, e2e = [], [], []
    for _ in range(5):
        search.append(window(lambda: G.search_device(gp_d, roots_d, args.k, max_d2, cos_max)))
        blend.append(window(lambda: G.blend_device(gp_d, ga_d, roots_d, idx, w, kept)))
    for _ in range(5):
        t, dev = e2e_s(args.roots)
        e2e.append(t)
    K, M, C = ga.shape
    result = {"roots": args.roots, "guides": K, "points_per_strand": M, "attrs": C, "k": args.k, "gpu": torch.cuda.get_device_name(0),
              "kept_roots": int(kept.numel()), "mean_guides_per_root": round(float(dev.n_guides.mean()), 3),
              "neighbours_kernel_ms": stats(search), "blend_kernel_ms": stats(blend), "device_e2e_s": stats(e2e),
              "distance_evaluations": args.roots * K, "blend_written_bytes": int(kept.numel()) * M * (12 + 4 * C), "neighbours_by_roots": {}}
    for n in args.search_roots:
        r_d = torch.as_tensor(scene(n, 1, 2, 1, seed=1)[1], device="cuda")
        events(lambda: G.search_device(gp_d, r_d, args.k, max_d2, cos_max))
        v = [window(lambda: G.search_device(gp_d, r_d, args.k, max_d2, cos_max)) for _ in range(5)]
        result["neighbours_by_roots"][str(n)] = dict(stats(v), workgroups=(n + 255) // 256, distance_evaluations=n * K)
    if not args.device_only:
        host = []
        for _ in range(max(1, args.host_repeats)):
            t, hres = host_s(args.roots)
            host.append(t)
        result["numpy_s"] = stats(host)
        result["paths_agree_bitwise"] = bool(all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(dev.strands, hres.strands))
                                             and dev.root_ids.tobytes() == hres.root_ids.tobytes())
    print(json.dumps(result))


if __name__ == "__main__":
    main()
