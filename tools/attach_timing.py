#!/usr/bin/env python3
"""Times the root attachment of exported strands (scene/strand_attach.py, csrc/hgs_attach.hip): --strands strands (10^5) of --points
points (100) rooted 0.5 to 3 cm above a head of 10 cm radius, the tangent tilted either way, against the exact distance to that sphere
on a grid of --grid nodes (128), with and without a direction volume (64 nodes an axis over the same box, directions around the
vertical axis leaning outward, full confidence); default knobs (step half a spacing, 256 steps at most); everything from seed 0.  After
a warm-up of each path, in this one process: each kernel on its own (device events around --repeats back-to-back launches on resident
buffers, the time per launch; five such windows; median and spread reported) -- hgs_root_attach without and with the volume,
hgs_strand_rejoin to --points points and in ragged mode; the device path end to end (attach_roots(device="cuda"): uploads, both
kernels, results copied to host arrays, lengths and the report; wall clock around a synchronised call, five calls) and the numpy path
on the same inputs (wall clock; --host-repeats runs), both with the volume.  Also checks that the two paths agree byte for byte.
--device-only skips the numpy path.  Prints one JSON line and writes it to --out (profiles/attach_timing.json)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "hair-gs_amd"))
sys.path.insert(0, os.path.join(HERE, ".."))

import numpy as np

from collide_timing import RADIUS, head


def scene(K, M, seed=0):
    """A StrandExport of K strands of M points: roots 0.5 to 3 cm above the sphere, each strand 20 cm long along a tangent tilted by up
    to 0.6 into or away from the head, then falling."""
    from scene.strand_export import StrandExport
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(K, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    t = np.cross(n, rng.normal(size=(K, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    d = t + rng.uniform(-0.6, 0.6, size=(K, 1)) * n
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    s = np.linspace(0.0, 1.0, M)[None, :, None]
    root = (RADIUS + rng.uniform(5e-3, 3e-2, size=(K, 1))) * n
    pts = (root[:, None, :] + 0.2 * s * d[:, None, :] + 0.1 * s * s * np.array([0.0, 0.0, -1.0])).astype(np.float32)
    attrs = rng.uniform(0.0, 1.0, size=(K * M, 5)).astype(np.float32)
    return StrandExport(pts.reshape(-1, 3), attrs, np.arange(K + 1, dtype=np.int64) * M, np.arange(K, dtype=np.int64), np.zeros(K))


def volume(sdf, grid=64):
    from utils.trace import Field
    span = (sdf.shape[0] - 1) * sdf.spacing
    h = span / (grid - 1)
    ax = sdf.origin[0] + h * np.arange(grid)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    pos = np.stack([x, y, z], axis=-1)
    d = np.cross(np.array([0.0, 0.0, 1.0]), pos) + 0.3 * pos
    ln = np.linalg.norm(d, axis=-1, keepdims=True)
    d = np.where(ln > 0, d / np.where(ln > 0, ln, 1.0), np.array([1.0, 0.0, 0.0]))
    return Field(sdf.origin, h, (grid, grid, grid), d, np.ones((grid, grid, grid)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strands", type=int, default=100000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--margin", type=float, default=0.0)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "attach_timing.json"))
    args = ap.parse_args()
    import torch
    from scene import strand_attach as SA
    strands, sdf = scene(args.strands, args.points), head(args.grid)
    vol = volume(sdf)
    vol_d = SA.volume_on(vol, "cuda")
    pts_d, att_d, off_d = (torch.as_tensor(v, device="cuda") for v in (strands.points, strands.attrs, strands.offsets))
    knobs = dict(margin=args.margin)

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

    def e2e_s(device):
        if device is not None:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = SA.attach_roots(strands, sdf, vol, points=args.points, device=device, **knobs)
        return time.perf_counter() - t0, res

    stats = lambda v: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "n": len(v)}
    march = lambda v: SA.attach_device(pts_d, off_d, sdf, v, **knobs)
    _, (ext, count, reason, landed) = events(lambda: march(vol_d))               # warm-up of everything that follows
    events(lambda: march(None))
    count_h, reason_h = count.cpu().numpy(), reason.cpu().numpy()
    offs = {M: SA.out_sizes(strands.offsets, count_h, reason_h, M)[1] for M in (0, args.points)}
    offs_d = {M: torch.as_tensor(o, device="cuda") for M, o in offs.items()}
    rejoin = lambda M: SA.rejoin_device(pts_d, att_d, off_d, ext, count, reason, M, offs_d[M], int(offs[M][-1]))
    events(lambda: rejoin(0))
    events(lambda: rejoin(args.points))
    e2e_s("cuda")
    plain, steered, resampled, ragged, e2e = [], [], [], [], []
    for _ in range(5):
        plain.append(window(lambda: march(None)))
        steered.append(window(lambda: march(vol_d)))
        resampled.append(window(lambda: rejoin(args.points)))
        ragged.append(window(lambda: rejoin(0)))
    for _ in range(5):
        t, (dev, report) = e2e_s("cuda")
        e2e.append(t)
    reached = reason_h == SA.REACHED
    result = {"strands": args.strands, "points_per_strand": args.points, "grid": args.grid, "volume_grid": 64, "margin": args.margin,
              "gpu": torch.cuda.get_device_name(0), "report": {k: v for k, v in report.items() if k != "reason"},
              "mean_joints_added_per_attached_strand": round(float(count_h[reached].mean()) if reached.any() else 0.0, 2),
              "most_joints_added": int(count_h.max()), "root_attach_ms": stats(plain), "root_attach_with_volume_ms": stats(steered),
              "strand_rejoin_resampled_ms": stats(resampled), "strand_rejoin_ragged_ms": stats(ragged), "device_e2e_s": stats(e2e),
              "ext_bytes": int(ext.numel()) * 8}
    if not args.device_only:
        host = []
        for _ in range(max(1, args.host_repeats)):
            t, (hres, hreport) = e2e_s(None)
            host.append(t)
        result["numpy_s"] = stats(host)
        same_report = all(np.array_equal(report[k], hreport[k]) if k == "reason" else report[k] == hreport[k] for k in report)
        result["paths_agree_bytewise"] = bool(all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(dev, hres)) and same_report)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
