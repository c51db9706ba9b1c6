"""Timing of the direction volume's fill (include/hgs.h hgs_field_fill; utils/field_fill.py, trace_strands.py --fill).

The workload: tools/trace_timing.py's directed cloud of 2 10^5 points (a combed shell over the upper half of a head of radius 0.1) moved
outward by --gap (0.05: half the head's radius) so that a gap separates it from the scalp, a direction volume of 128 nodes along its
longest side, radius 1.5 voxels; the 10^4 scalp points splatted with their outward directions; the head an analytic ball; the box
domain (every node outside the head is FREE or FIXED).

  kernels  hgs_field_fill with resident buffers: device events around one call of --sweeps sweeps (one launch a sweep, no host
           synchronisation between them), the median of --reps after one warm-up; a call of one sweep likewise; the bytes a sweep must
           move are counted as F * (6*8 read + 6*8 written + 4 of the index + 1 of the kind byte): every FREE node's six values read once
           (the neighbours' re-reads are left to the caches) and written once
  numpy    fill_numpy on the same inputs, a host clock, --numpy_sweeps sweeps (the sweeps cost the same, one after the other); its result
           is compared with the kernel's bit for bit at that count.  The only baseline there is: the parent commit has no such step
  bench    `python bench.py --gpus 1 --steps 100 --warmup 10` of the tree, in a child process: its result line (tools/trace_timing.py's leg)

--root DIR runs the bench leg on another checkout (built there), --label names it in the rows.  Prints one JSON line per leg.  --out
FILE holds {"rows": [...]}; --append adds to the rows already there, so that profiles/fill_timing.json is what these write, one after
the other, in one session on one box:
  python tools/fill_timing.py --out profiles/fill_timing.json
  python tools/fill_timing.py --legs bench --append --out profiles/fill_timing.json
  python tools/fill_timing.py --root <parent checkout> --label "parent commit" --legs bench --append --out profiles/fill_timing.json"""
import argparse
import json
import os
import sys
import time

HERE = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trace_timing as TT  # noqa: E402

HEAD_R, FIXED_CONF = 0.1, 0.5
BYTES_PER_FREE_NODE = 6 * 8 + 6 * 8 + 4 + 1


def inputs(gap):
    """(field with the scalp's nodes taken in and the head's cleared, kind, seed) as host arrays."""
    import numpy as np
    from utils import field_fill as FF
    from utils import trace as T
    pts, dirs, roots, head = TT.workload()
    pts = pts + gap * pts / np.linalg.norm(pts, axis=1, keepdims=True)
    origin, h, shape = T.grid_box(pts, roots, TT.GRID, TT.RADIUS)
    field = T.build_field(pts, dirs, origin, h, shape, TT.RADIUS * h, device="cuda")
    scalp = T.build_field(roots, T.initial_directions(roots, head), origin, h, shape, TT.RADIUS * h, device="cuda")
    take = (scalp.conf >= FIXED_CONF) & (field.conf < FIXED_CONF)
    field.dir[take], field.conf[take] = scalp.dir[take], scalp.conf[take]
    outside = np.linalg.norm(field.nodes(), axis=1).reshape(field.conf.shape) >= HEAD_R
    field.conf[~outside] = 0.0
    kind = FF.classify(field, FIXED_CONF, outside)
    return field, kind, FF.seed(field, kind), h


def kernel_leg(args, emit, data):
    import torch
    import hgs_runtime as rt
    from utils import field_fill as FF
    field, kind, seed, h = data
    nx, ny, nz = field.shape
    k, t = torch.from_numpy(kind).cuda(), torch.from_numpy(seed).cuda()
    a, b = t.clone(), t.clone()
    index = torch.nonzero(k.reshape(-1) == FF.FREE).reshape(-1).to(torch.int32)
    F = rt.fill_check(field.shape, k, a, b, index)
    fixed, free, out = FF.counts(kind)
    row = dict(leg="kernels", grid=list(field.shape), nodes=nx * ny * nz, fixed=fixed, free=free, out=out, gap_voxels=args.gap / h,
               bytes_per_sweep=F * BYTES_PER_FREE_NODE, bytes_counted="F * (48 read + 48 written + 4 index + 1 kind)",
               buffers_bytes=2 * 6 * 8 * nx * ny * nz)

    def call(sweeps):
        def fn():
            rt.check(rt.lib().hgs_field_fill(rt.current_stream(), nx, ny, nz, rt.ptr(k), rt.ptr(index), F, rt.ptr(a), rt.ptr(b), sweeps))
        return fn
    for sweeps in (args.sweeps, 1):
        a.copy_(t)
        b.copy_(t)
        ms = TT._event_ms(call(sweeps), args.reps)
        per = ms["median_ms"] / sweeps
        emit(dict(row, what=f"hgs_field_fill, {sweeps} sweep(s) in one call", sweeps=sweeps, per_sweep_us=1e3 * per,
                  achieved_TB_per_s=F * BYTES_PER_FREE_NODE / (per * 1e-3) / 1e12, **ms))
    res, prev = FF.fill_device(t, k, args.sweeps)
    emit(dict(leg="kernels", what=f"the result after {args.sweeps} sweeps", last_change=float((res - prev).abs().max()),
              free_at_min_conf=_reached(field, kind, res)))
    return t, k


def _reached(field, kind, res):
    from utils import field_fill as FF
    from utils import trace as T
    d, conf = T.solve_device(FF.quantise_device(res), field.shape)
    return int(((conf.cpu().numpy() >= FIXED_CONF) & (kind == FF.FREE)).sum())


def numpy_leg(args, emit, data, dev):
    from utils import field_fill as FF
    field, kind, seed, h = data
    t0 = time.perf_counter()
    res, prev = FF.fill_numpy(seed, kind, args.numpy_sweeps)
    dt = time.perf_counter() - t0
    got = FF.fill_device(dev[0], dev[1], args.numpy_sweeps)
    same = res.tobytes() == got[0].cpu().numpy().tobytes() and prev.tobytes() == got[1].cpu().numpy().tobytes()
    emit(dict(leg="numpy", what=f"fill_numpy on the same inputs, {args.numpy_sweeps} sweeps (the neighbour tables built once, in the time)",
              sweeps=args.numpy_sweeps, total_s=dt, per_sweep_s=dt / args.numpy_sweeps, projected_s_at_kernel_sweeps=dt / args.numpy_sweeps * args.sweeps,
              bits_equal_to_the_kernel=bool(same)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernels,numpy")
    ap.add_argument("--label", default=None, help="name of the tree in the rows (default: 'this tree', or --root as given)")
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds")
    ap.add_argument("--root", default=HERE, help="checkout whose bench.py the bench leg runs (default: this one)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gap", type=float, default=0.05, help="how far the shell is moved outward, in scene units")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--numpy_sweeps", type=int, default=3)
    args = ap.parse_args()
    sys.path[:0] = [HERE, os.path.join(HERE, "hair-gs_amd")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fill_timing.py measures on the GPU; there is none")
    rows = []
    label = args.label or ("this tree" if os.path.abspath(args.root) == HERE else args.root)

    def emit(row):
        row["tree"] = label
        for k, v in list(row.items()):
            if isinstance(v, float):
                row[k] = float(f"{v:.4g}")
        rows.append(row)
        print(json.dumps(row), flush=True)
    legs = args.legs.split(",")
    try:
        data = dev = None
        for leg in legs:
            if leg == "bench":
                TT.bench_leg(args, emit)
                continue
            if data is None:
                data = inputs(args.gap)
                dev = kernel_leg(args, emit if "kernels" in legs else (lambda row: None), data)
            if leg == "numpy":
                numpy_leg(args, emit, data, dev)
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
