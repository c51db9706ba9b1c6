#!/usr/bin/env python3
"""Times one push-out of exported strands from the head (scene/strand_collide.py, csrc/hgs_collide.hip): --strands strands (10^5) of
--points points (100) rooted on the upper cap of a head of 10 cm radius and falling 20 cm, a share of them tilted into the head,
against the exact distance to that sphere on a grid of --grid nodes (128), margin 1 mm, 8 pushes at most; everything from seed 0.
After a warm-up of each path, in this one process: the kernel on its own (device events around --repeats back-to-back launches on
resident buffers, the time per launch; five such windows; median and spread reported); the same kernel on the same strands against a
field whose box lies far from them, so that every joint is out of range and no field value is fetched -- what is left is the lanes'
walk over their own joints, 12 bytes at a stride of one strand, and the float64 arithmetic: the two figures side by side say whether
the point traffic or the dependent gathers of the field bound the kernel; the device path end to end (resolve_head(device="cuda"):
uploads, the kernel, the two distance passes of the report, results copied to host arrays, lengths and the report; wall clock around a
synchronised call, five calls) and the numpy path on the same inputs (wall clock; --host-repeats runs).  Also checks that the two
paths agree byte for byte.  --device-only skips the numpy path.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np

RADIUS = 0.1


def head(grid, pad=0.6, centre=(0.0, 0.0, 0.0)):
    """The exact distance to the sphere of 10 cm about `centre` on a cubic grid that reaches `pad` diameters beyond it."""
    from utils.head_sdf import HeadSDF
    lo = -(RADIUS + pad * 2.0 * RADIUS)
    h = -2.0 * lo / (grid - 1)
    ax = (lo + h * np.arange(grid)).astype(np.float32)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    phi = np.sqrt(x * x + y * y + z * z) - np.float32(RADIUS)
    return HeadSDF(np.array([lo, lo, lo]) + np.asarray(centre, np.float64), h, (grid, grid, grid), phi.astype(np.float32))


def scene(K, M, seed=0):
    """A StrandExport of K strands of M points: roots 2 mm above the upper cap (outside the margin), each strand 20 cm long, leaving along a
    direction between 0.6 into the head and 0.6 away from it per unit of tangent, then falling."""
    from scene.strand_export import StrandExport
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(K, 3))
    n[:, 2] = np.abs(n[:, 2])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    t = np.cross(n, rng.normal(size=(K, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    d = t + rng.uniform(-0.6, 0.6, size=(K, 1)) * n
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    s = np.linspace(0.0, 1.0, M)[None, :, None]
    pts = ((RADIUS + 2e-3) * n[:, None, :] + 0.2 * s * d[:, None, :] + 0.1 * s * s * np.array([0.0, 0.0, -1.0])).astype(np.float32)
    return StrandExport(pts.reshape(-1, 3), np.zeros((K * M, 1), np.float32), np.arange(K + 1, dtype=np.int64) * M, np.arange(K, dtype=np.int64),
                        np.zeros(K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--margin", type=float, default=1e-3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    import torch
    from scene import strand_collide as SC
    strands, sdf = scene(args.strands, args.points), head(args.grid)
    far = head(args.grid, centre=(10.0, 0.0, 0.0))
    pts_d, off_d = torch.as_tensor(strands.points, device="cuda"), torch.as_tensor(strands.offsets, device="cuda")

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

    def e2e_s():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = SC.resolve_head(strands, sdf, margin=args.margin, iters=args.iters, device="cuda")
        return time.perf_counter() - t0, res

    def host_s():
        t0 = time.perf_counter()
        res = SC.resolve_head(strands, sdf, margin=args.margin, iters=args.iters)
        return time.perf_counter() - t0, res

    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    kernel = lambda field: SC.resolve_device(pts_d, off_d, field, args.margin, None, args.iters)
    events(lambda: kernel(sdf))                                                  # warm-up of everything that follows
    events(lambda: kernel(far))
    e2e_s()
    full, walk, e2e = [], [], []
    for _ in range(5):
        full.append(window(lambda: kernel(sdf)))
        walk.append(window(lambda: kernel(far)))
    for _ in range(5):
        t, (dev, report) = e2e_s()
        e2e.append(t)
    _, moved, _ = kernel(sdf)
    P = int(strands.points.shape[0])
    result = {"strands": args.strands, "points_per_strand": args.points, "grid": args.grid, "margin": args.margin, "iters": args.iters,
              "gpu": torch.cuda.get_device_name(0), "report": report, "share_of_strands_touched": round(report["strands_touched"] / max(1, args.strands), 4),
              "kernel_ms": stats(full), "kernel_out_of_range_field_ms": stats(walk), "device_e2e_s": stats(e2e),
              "point_bytes_read_and_written": 24 * P, "field_bytes": 4 * args.grid ** 3,
              "point_traffic_gb_per_s_at_kernel_median": round(24 * P / (float(np.median(full)) * 1e-3) / 1e9, 1)}
    assert int(moved.sum()) == report["moved"]
    if not args.device_only:
        host = []
        for _ in range(max(1, args.host_repeats)):
            t, (hres, hreport) = host_s()
            host.append(t)
        result["numpy_s"] = stats(host)
        result["paths_agree_bytewise"] = bool(all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(dev, hres)) and report == hreport)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
