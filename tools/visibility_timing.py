"""Timing of the hull's ray march and the gated lift (include/hgs.h hgs_hull_visibility, hgs_lift_moments_gated; utils/visibility.py,
utils/lift.py).

The workload is tools/lift_timing.py's: 2 10^5 points on an ellipsoid against 32 views of 1920x1080 whose masks are its analytic
silhouettes and whose orientation maps show a combed tangent field at the first hit of every pixel's ray, so that a far-side view
reports the near side's hair.  The grid is the carve of those masks, --grid (256) voxels along the side of the cube [-1.2, 1.2]^3,
min_views 3 and min_percent 100: the solid hull the driver would march.

  kernels  device events around single calls, the median of --reps after one warm-up, buffers resident: hgs_hull_visibility on the
           grid, and the same rays walked to their ends with an occupancy load at every step (max_blocked 3072) and with none (skip
           1024), which is what the loads cost; hgs_lift_moments and hgs_lift_moments_gated without and with a previous direction; the device loop of the rounds,
           plain and gated.  Also records, as measurements, the share of the pairs that are visible, the median angle between the
           lifted lines and the field for the plain and the gated lift after round 0 and after the last round, and the points that
           keep a direction.
  numpy    visibility_numpy on the same inputs, a host clock, once, and that its words equal the kernel's: the only baseline there is
           (the parent commit has no such step)
  bench    `python bench.py --gpus 1 --steps 100 --warmup 10` of the tree, in a child process: its result line

--root DIR runs the bench leg on another checkout (built there), --label names it in the rows.  Prints one JSON line per leg.  --out
FILE holds {"rows": [...]}; --append adds to the rows already there, so that profiles/visibility_timing.json is what these write, one
after the other, in one session on one box:
  python tools/visibility_timing.py --out profiles/visibility_timing.json
  python tools/visibility_timing.py --root <parent checkout> --label "parent commit" --legs bench --append --out profiles/visibility_timing.json
  python tools/visibility_timing.py --legs bench --append --out profiles/visibility_timing.json     (alternated with the line above)"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [HERE, os.path.join(HERE, "hair-gs_amd"), os.path.dirname(os.path.abspath(__file__))]


def kernel_legs(args, emit):
    import numpy as np
    import torch
    from carve_timing import AXES, H, W, capture, events
    from lift_timing import field, median_angle, orientation_maps
    from utils import carve, lift, visibility
    views, masks = capture(args.views)
    orients, confs = orientation_maps(views, masks)
    rng = np.random.default_rng(0)
    u = rng.normal(size=(args.points, 3))
    u[:, 2] *= 0.8                                               # (lift_timing.py's points: fewer at the poles, where the field is singular)
    pts = np.ascontiguousarray(u / np.linalg.norm(u, axis=1, keepdims=True) * AXES)
    truth = field(pts)
    packed = lift.pack(views, masks, orients, confs, "cuda")
    n = args.grid
    origin, h = np.full(3, -1.2), 2.4 / n
    occ = carve.grid_device(origin, h, (n, n, n), packed.carve, 3, 100)
    dev = torch.from_numpy(pts).cuda()
    centres = visibility.upload_centres(visibility.camera_centres(views), "cuda")
    s2 = lift.sin2(args.sigma_deg)

    def march():
        return visibility.visibility_device(dev, centres, occ, origin, h, args.skip, args.max_blocked)
    words = march()
    host_words = words.cpu().numpy()
    vis = visibility.unpack_bits(host_words, args.views)
    row = dict(leg="kernels", device=torch.cuda.get_device_name(0), points=args.points, views=args.views, view_size=[W, H], grid=[n, n, n],
               occupied_voxels=int(occ.sum()), occ_bytes=int(occ.numel()), skip=args.skip, max_blocked=args.max_blocked, reps=args.reps)
    ms = events(march, args.reps)
    emit(dict(row, what="hgs_hull_visibility", median_ms=ms, pairs=args.points * args.views, pairs_per_s=round(args.points * args.views / ms * 1e3),
              visible_share=float(vis.mean()), visible_views_median=int(np.median(vis.sum(axis=1)))))
    # what the occupancy loads cost: the same rays walked to the end of the grid or to the camera, with a load at every step
    # (max_blocked above any ray's length: nothing stops early) and with none (skip above any distance: no voxel is tested)
    every = events(lambda: visibility.visibility_device(dev, centres, occ, origin, h, args.skip, visibility.MAX_BLOCKED), args.reps)
    none = events(lambda: visibility.visibility_device(dev, centres, occ, origin, h, visibility.MAX_SKIP, 0), args.reps)
    emit(dict(leg="kernels", what="hgs_hull_visibility, every ray walked to its end: a load at every step / no load at all",
              every_load_ms=every, no_load_ms=none))
    d_plain0 = lift.solve_device(*lift.moments_device(dev, packed)[::2])[0]
    d_gated0 = lift.solve_device(*lift.moments_device(dev, packed, visible=words)[::2])[0]
    d_plain = lift.directions_device(dev, packed, args.rounds, args.sigma_deg)[0]
    d_gated = lift.directions_device(dev, packed, args.rounds, args.sigma_deg, visible=words)[0]
    for name, d0, d in (("plain", d_plain0, d_plain), ("gated", d_gated0, d_gated)):
        a0, _ = median_angle(d0.cpu().numpy(), truth)
        a, kept = median_angle(d.cpu().numpy(), truth)
        emit(dict(leg="kernels", what=f"the {name} lift's lines against the field", median_angle_deg_round_0=a0, median_angle_deg_last_round=a,
                  rounds=args.rounds, points_with_a_direction=kept))
    for what, fn in (("hgs_lift_moments", lambda: lift.moments_device(dev, packed)),
                     ("hgs_lift_moments_gated", lambda: lift.moments_device(dev, packed, visible=words)),
                     ("hgs_lift_moments with prev", lambda: lift.moments_device(dev, packed, d_plain0, s2)),
                     ("hgs_lift_moments_gated with prev", lambda: lift.moments_device(dev, packed, d_gated0, s2, visible=words)),
                     ("directions_device, plain", lambda: lift.directions_device(dev, packed, args.rounds, args.sigma_deg)),
                     ("directions_device, gated", lambda: lift.directions_device(dev, packed, args.rounds, args.sigma_deg, visible=words))):
        emit(dict(leg="kernels", what=what, median_ms=events(fn, args.reps)))
    return pts, visibility.camera_centres(views), occ.cpu().numpy(), origin, h, host_words


def numpy_leg(args, emit, inputs):
    from utils import visibility
    pts, C, occ, origin, h, words = inputs
    t0 = time.perf_counter()
    host = visibility.visibility_numpy(pts, C, occ, origin, h, args.skip, args.max_blocked)
    emit(dict(leg="numpy", what="visibility_numpy on the same inputs", seconds=time.perf_counter() - t0,
              words_equal=bool(host.tobytes() == words.tobytes())))


def bench_leg(args, emit):
    """bench.py of the tree in a child process."""
    root = os.path.abspath(args.root)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10"],
                         cwd=root, stdout=subprocess.PIPE, text=True, check=True).stdout.strip().splitlines()[-1]
    d = json.loads(out)
    emit(dict(leg="bench", what="bench.py --gpus 1 --steps 100 --warmup 10", iters_per_sec=d["value"], repeats=d.get("repeats")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernels,numpy")
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--skip", type=int, default=1)
    ap.add_argument("--max_blocked", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sigma_deg", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default=None, help="name of the tree in the rows (default: 'this tree', or --root as given)")
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds")
    ap.add_argument("--root", default=HERE, help="checkout whose bench.py the bench leg runs (default: this one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("visibility_timing.py measures on the GPU; there is none")
    rows = []
    label = args.label or ("this tree" if os.path.abspath(args.root) == HERE else args.root)

    def emit(row):
        row["tree"] = label
        for k, v in list(row.items()):
            if isinstance(v, float):
                row[k] = round(v, 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    legs = args.legs.split(",")
    try:
        inputs = None
        for leg in legs:
            if leg == "bench":
                bench_leg(args, emit)
                continue
            if inputs is None:
                inputs = kernel_legs(args, emit if "kernels" in legs else (lambda row: None))
            if leg == "numpy":
                numpy_leg(args, emit, inputs)
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            old = []
            if args.append and os.path.exists(args.out):
                with open(args.out) as f:
                    old = json.load(f)["rows"]
            with open(args.out, "w") as f:
                json.dump({"rows": old + rows}, f, indent=1)


if __name__ == "__main__":
    main()
