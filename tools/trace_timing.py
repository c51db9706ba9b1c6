"""Timing of the strand tracer (include/hgs.h hgs_field_splat, hgs_field_solve, hgs_strand_trace; utils/trace.py, trace_strands.py).

The workload: a directed cloud of 2 10^5 points (a combed shell over the upper half of a head of radius 0.1: hair lines that run down
the meridians), a direction volume of 128 nodes along its longest side, radius 1.5 and step 0.5 voxels, 10^4 roots on the head.

  kernels  each kernel alone: device events around single launches, the median of --reps after one warm-up (uploads and read-backs are
           not in it; the splat's row includes the memset of its sums)
  numpy    the numpy path on the same inputs, a host clock, once: the only baseline there is (the parent commit has no such step)
  driver   trace_strands.py end to end on a capture directory written for it (--device cuda; reading the cloud, both kernels'
           uploads and read-backs, the filters, the resampling and the PLY): a host clock, the median of --reps runs after one warm-up
  bench    `python bench.py --gpus 1 --steps 100 --warmup 10` of the tree, in a child process: its result line

--root DIR runs the bench leg on another checkout (built there), --label names it in the rows.  Prints one JSON line per leg.  --out
FILE holds {"rows": [...]}; --append adds to the rows already there, so that profiles/trace_timing.json is what these write, one after
the other, in one session on one box:
  python tools/trace_timing.py --out profiles/trace_timing.json
  python tools/trace_timing.py --root <parent checkout> --label "parent commit" --legs bench --append --out profiles/trace_timing.json
  python tools/trace_timing.py --legs bench --append --out profiles/trace_timing.json     (alternated with the line above)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
POINTS, GRID, ROOTS, RADIUS, STEP_VOX = 200000, 128, 10000, 1.5, 0.5
KNOBS = dict(max_steps=400, cos_max=0.5, min_conf=0.5, max_gap=4)


def workload(n_points=POINTS, n_roots=ROOTS, seed=0):
    """(points, dirs, roots, head_verts) float64."""
    import numpy as np
    rng = np.random.default_rng(seed)

    def upper(n, r_lo, r_hi, z_min):
        v = rng.normal(size=(3 * n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v = v[v[:, 2] > z_min][:n]
        return v * rng.uniform(r_lo, r_hi, size=(v.shape[0], 1))
    pts = upper(n_points, 0.1, 0.17, -0.2)
    radial = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    down = np.array([0.0, 0.0, -1.0])[None, :] + radial * radial[:, 2:3] + np.array([0.2, 0.0, 0.0])
    dirs = down / np.linalg.norm(down, axis=1, keepdims=True)
    head = rng.normal(size=(5000, 3))
    head = 0.1 * head / np.linalg.norm(head, axis=1, keepdims=True)
    return pts, dirs, upper(n_roots, 0.1, 0.1, 0.3), head


def _event_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts)}


def kernel_legs(args, emit):
    import numpy as np
    import torch
    from utils import trace as T
    pts, dirs, roots, head = workload()
    origin, h, shape = T.grid_box(pts, roots, GRID, RADIUS)
    nodes = int(shape[0] * shape[1] * shape[2])
    p, d = torch.from_numpy(pts).cuda(), torch.from_numpy(dirs).cuda()
    acc = torch.zeros((shape[2], shape[1], shape[0], 7), dtype=torch.int64, device="cuda")
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")

    def splat():
        acc.zero_()
        skipped.zero_()
        T.splat_device(p, d, origin, h, shape, RADIUS * h, acc=acc, skipped=skipped)
    row = dict(leg="kernels", points=int(pts.shape[0]), grid=list(shape), nodes=nodes, radius_voxels=RADIUS)
    emit(dict(row, what="hgs_field_splat (scatter, int64 atomics) + the memset of the sums", **_event_ms(splat, args.reps)))
    emit(dict(row, what="the memset of the sums alone", **_event_ms(lambda: (acc.zero_(), skipped.zero_()), args.reps)))
    splat()
    emit(dict(row, what="hgs_field_solve", nonempty=int((acc[..., 0] != 0).sum()), **_event_ms(lambda: T.solve_device(acc, shape), args.reps)))
    fd, fc = T.solve_device(acc, shape)
    r, p0 = torch.from_numpy(roots).cuda(), torch.from_numpy(T.initial_directions(roots, head)).cuda()

    def trace():
        return T.trace_device(r, p0, fd, fc, origin, h, shape, STEP_VOX * h, **KNOBS)
    joints, count, reason = trace()
    count = count.cpu().numpy()
    emit(dict(leg="kernels", what="hgs_strand_trace", roots=int(roots.shape[0]), max_steps=KNOBS["max_steps"], mean_joints=float(count.mean()),
              reasons={n: int((reason == c).sum()) for c, n in enumerate(T.REASONS)}, **_event_ms(trace, args.reps)))
    return pts, dirs, roots, head, (origin, h, shape), T.Field(origin, h, shape, fd.cpu().numpy(), fc.cpu().numpy()), np.asarray(count)


def numpy_leg(args, emit, inputs):
    from utils import trace as T
    pts, dirs, roots, head, (origin, h, shape), field, count = inputs
    t0 = time.perf_counter()
    acc, _ = T.splat_numpy(pts, dirs, origin, h, shape, RADIUS * h)
    t1 = time.perf_counter()
    T.solve_numpy(acc)
    t2 = time.perf_counter()
    _, c, _ = T.trace_numpy(roots, T.initial_directions(roots, head), field, STEP_VOX * h, **KNOBS)
    t3 = time.perf_counter()
    emit(dict(leg="numpy", what="splat_numpy / solve_numpy / trace_numpy on the same inputs (the trace through the device's field)",
              splat_s=t1 - t0, solve_s=t2 - t1, trace_s=t3 - t2, counts_equal=bool((c == count).all())))


def write_capture(root, pts, dirs, roots, head):
    """The smallest capture directory the driver reads: two 32 x 32 views, the directed cloud, the head side file."""
    import numpy as np
    from PIL import Image
    from data import colmap
    from data.dataset_readers import storePly
    sparse = os.path.join(root, "sparse", "0")
    for d in (sparse, os.path.join(root, "images")):
        os.makedirs(d, exist_ok=True)
    cams = {1: colmap.Camera(id=1, model="PINHOLE", width=32, height=32, params=np.array([40.0, 40.0, 16.0, 16.0]))}
    images = {}
    for i in range(2):
        name = f"v{i:02d}.png"
        images[i + 1] = colmap.Image(id=i + 1, qvec=np.array([1.0, 0.0, 0.0, 0.0]), tvec=np.array([0.05 * i, 0.0, 1.0]), camera_id=1, name=name,
                                     xys=np.zeros((0, 2)), point3D_ids=np.zeros(0, np.int64))
        Image.fromarray(np.zeros((32, 32, 3), np.uint8)).save(os.path.join(root, "images", name))
    colmap.write_cameras_binary(cams, os.path.join(sparse, "cameras.bin"))
    colmap.write_images_binary(images, os.path.join(sparse, "images.bin"))
    storePly(os.path.join(sparse, "points3D.ply"), pts.astype(np.float32), np.full((pts.shape[0], 3), 128, np.uint8), dirs.astype(np.float32))
    np.savez(os.path.join(root, "head_reconstruction_data.npz"), head_verts=head, scalp_verts=roots)


def driver_leg(args, emit, inputs):
    import contextlib
    import io
    import torch
    import trace_strands
    pts, dirs, roots, head = inputs[:4]
    with tempfile.TemporaryDirectory() as tmp:
        write_capture(tmp, pts, dirs, roots, head)
        ts, n = [], 0
        for k in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                n = trace_strands.main(["-s", tmp, "-m", os.path.join(tmp, "model"), "--grid", str(GRID), "--overwrite"])
            torch.cuda.synchronize()
            if k:
                ts.append(time.perf_counter() - t0)
    emit(dict(leg="driver", what="trace_strands.py --device cuda end to end (defaults, --grid 128)", strands=int(n), median_s=statistics.median(ts),
              min_s=min(ts)))


def bench_leg(args, emit):
    """bench.py of the tree in a child process."""
    root = os.path.abspath(args.root)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10"],
                         cwd=root, stdout=subprocess.PIPE, text=True, check=True).stdout.strip().splitlines()[-1]
    d = json.loads(out)
    emit(dict(leg="bench", what="bench.py --gpus 1 --steps 100 --warmup 10", iters_per_sec=d["value"], repeats=d.get("repeats")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernels,numpy,driver")
    ap.add_argument("--label", default=None, help="name of the tree in the rows (default: 'this tree', or --root as given)")
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds")
    ap.add_argument("--root", default=HERE, help="checkout whose bench.py the bench leg runs (default: this one)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    sys.path[:0] = [HERE, os.path.join(HERE, "hair-gs_amd")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trace_timing.py measures on the GPU; there is none")
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
            elif leg == "driver":
                driver_leg(args, emit, inputs)
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
