"""Timing of the 3-D direction term's device op (include/hgs.h hgs_direction_loss_*) and of the iteration that carries it.

  op      the op alone at 10^5 and 4 10^5 segments (strands of 20 segments) on a volume of 128^3 nodes, forward and forward +
          backward, and hgs_head_penalty_forward at the same number of points in the same session (the yardstick: the same
          dependent-latency shape, a quarter of the gather bytes): device events around replays of a captured graph that holds
          --calls calls, medians of --reps replays after one warm-up replay
  step    the north_star captured step (1 step per graph launch) with the term on (lambda_direction 1, an analytic swirl of 129^3
          nodes around the joints) and off: a host clock around --steps optimizer steps that end in a synchronise, after --warmup
          steps, --regions times; the launches the term adds are listed with the "on" row
  bench   `python bench.py --gpus 1 --steps 100 --warmup 10` of the tree, in a child process: its result line

--root DIR imports the package of another checkout (built there) instead of this one, --label names it in the rows: the parent
commit's numbers come from its own tree; legs that need the term are skipped where the tree has none.
Prints one JSON line per leg.  --out FILE holds {"rows": [...]}; --append adds to the rows already there, so that
profiles/direction_timing.json is what these write, one after the other, in one session on one box:
  python tools/direction_timing.py --out profiles/direction_timing.json
  python tools/direction_timing.py --legs bench --append --out profiles/direction_timing.json
  python tools/direction_timing.py --root <parent checkout> --label "parent commit" --legs bench --append --out profiles/direction_timing.json
  (repeat the last two for the alternated bench.py lines)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ADDED_LAUNCHES = ["direction_loss_kernel", "direction_reduce_kernel", "direction_bwd_kernel",
                  "torch: lambda_direction * term, loss + it, and their backward (scalar multiplies); the two endpoint gradients added",
                  "hgs_adam_step (Adam leaves the backward's lanes, as with the magnet and head terms)"]


def _events(fn_capture, calls, reps):
    """Median / min ms per call of `fn_capture` (enqueues one call) from replays of a graph that holds `calls` of them."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn_capture()                                   # warm-up: allocator, code objects
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn_capture()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts)}


def _box(points, nodes):
    lo, hi = points.min(axis=0), points.max(axis=0)
    L = float((hi - lo).max())
    return lo - 0.1 * L, 1.2 * L / (nodes - 1), L


def _swirl(points, nodes=128):
    """An analytic swirl about `points` (numpy [E, 3]): line ~ (-y, x, -0.5) about their centre with a random sign per node, conf 1,
    as a DirectionVolume of nodes^3 over their box."""
    import numpy as np
    from utils.direction_term import DirectionVolume
    from utils.trace import Field
    c = points.mean(axis=0)
    origin, h, L = _box(points, nodes)
    z, y, x = np.meshgrid(*(origin[k] + h * np.arange(nodes) for k in (2, 1, 0)), indexing="ij")
    d = np.stack([-(y - c[1]), x - c[0], np.full_like(x, -0.5 * L)], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d *= np.random.default_rng(8).choice([-1.0, 1.0], size=x.shape)[..., None]
    return DirectionVolume(Field(origin, h, (nodes,) * 3, d, np.ones_like(x)))


def _ball(points, share, nodes=128):
    """tools/head_sdf_timing.py's field: an analytic ball about `points` that holds about `share` of them, nodes^3."""
    import numpy as np
    from utils.head_sdf import HeadSDF
    c = points.mean(axis=0)
    radius = float(np.quantile(np.linalg.norm(points - c, axis=1), share))
    origin, h, _ = _box(points, nodes)
    z, y, x = np.meshgrid(*(origin[k] + h * np.arange(nodes) for k in (2, 1, 0)), indexing="ij")
    return HeadSDF(origin, h, (nodes,) * 3, (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius).astype(np.float32))


def op_legs(args, emit):
    import torch
    from hgs_runtime import fused as F
    from synthetic import strand_polylines
    for segments in (100000, 400000):
        n = segments // 20
        pts = torch.as_tensor(strand_polylines(n, 20, seed=3), dtype=torch.float32).reshape(-1, 3)
        pairs = (torch.arange(n)[:, None] * 21 + torch.arange(20)[None, :]).reshape(-1)
        pairs = torch.stack([pairs, pairs + 1], dim=1).cuda()
        host = pts.numpy().astype("float64")
        vol, sdf = _swirl(host), _ball(host, 0.2)
        ep = pts.cuda().requires_grad_(True)
        table = F.DirectionTable(pairs, ep.shape[0])
        scratch = F.DirectionScratch(table.S, table.E, "cuda")
        info = {}
        F.direction_loss(ep, table, vol, 0.5, info, scratch)
        active = F.direction_active(info)
        calls = max(2, min(args.calls, 4000000 // segments))
        # as many points as there are segments for the yardstick: the same number of lanes, each with eight dependent gathers
        hp = ep.detach()[:table.S].contiguous()
        head_scratch = F.HeadScratch(hp.shape[0], "cuda")

        def fwd():
            with torch.no_grad():
                F.direction_loss(ep, table, vol, 0.5, None, scratch)

        def fwd_bwd():
            ep.grad = None
            F.direction_loss(ep, table, vol, 0.5, None, scratch).backward()

        def head_fwd():
            with torch.no_grad():
                F.head_penalty(hp, sdf, 0.0, None, head_scratch)
        common = dict(leg="op", segments=table.S, endpoints=table.E, active=active, nodes=128 ** 3, calls_per_graph=calls)
        emit(dict(what="direction_loss forward", **common, **_events(fwd, calls, args.reps)))
        emit(dict(what="direction_loss forward + backward", **common, **_events(fwd_bwd, calls, args.reps)))
        emit(dict(what="head_penalty forward (yardstick)", leg="op", points=int(hp.shape[0]), nodes=128 ** 3, calls_per_graph=calls,
                  **_events(head_fwd, calls, args.reps)))


def step_legs(args, emit):
    import torch
    from arguments import OptimizationParams
    from diff_gaussian_rasterization import _C as raster
    from synthetic import build_workload
    from train import GraphedStep, ViewSampler
    from utils.general import safe_state
    have_term = hasattr(OptimizationParams(), "lambda_direction")
    for name, lam in (("captured step, term off", 0.0), ("captured step, term on", 1.0)):
        if lam > 0 and not have_term:
            continue
        safe_state(True)
        model, cams, extent = build_workload("north_star", device="cuda", seed=0)
        opt = OptimizationParams()
        opt.enable_topology = False
        if have_term:
            opt.lambda_direction = lam
        if lam > 0:
            model.direction_volume = _swirl(model._endpoints.detach().cpu().numpy().astype("float64"), 129)
        model.training_setup(opt)
        bg = torch.zeros(3, dtype=torch.float32, device="cuda")
        sampler = ViewSampler(cams, seed=0)
        it = 0
        try:
            gs = GraphedStep(model, cams, opt, bg, extent=extent, steps_per_graph=1)
            gs.capture(cams, iteration=1)

            def run(n):
                nonlocal it
                for _ in range(n):
                    it += 1
                    gs.step(sampler.next(), it)
            run(args.warmup)
            regions = []
            for _ in range(args.regions):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize()
                regions.append(args.steps / (time.perf_counter() - t0))
            gs.check()
            row = dict(leg="step", what=name, workload="north_star", segments=int(model.endpoint_pairs.shape[0]), lambda_direction=lam,
                       adam_in_backward_lanes=bool(gs.inline_adam), steps=args.steps, iters_per_sec_median=statistics.median(regions),
                       iters_per_sec_min=min(regions), iters_per_sec_max=max(regions))
            if lam > 0:
                row["launches_added"] = ADDED_LAUNCHES
            emit(row)
        finally:
            raster.set_async(False)
        del model, cams
        torch.cuda.empty_cache()


def bench_leg(args, emit):
    """bench.py of the tree in a child process (this one holds no GPU memory by then that the child would miss)."""
    root = os.path.abspath(args.root)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10"],
                         cwd=root, stdout=subprocess.PIPE, text=True, check=True).stdout.strip().splitlines()[-1]
    d = json.loads(out)
    emit(dict(leg="bench", what="bench.py --gpus 1 --steps 100 --warmup 10", iters_per_sec=d["value"], repeats=d.get("repeats")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="op,step")
    ap.add_argument("--label", default=None, help="name of the tree in the rows (default: 'this tree', or --root as given)")
    ap.add_argument("--append", action="store_true", help="keep the rows --out already holds")
    ap.add_argument("--root", default=HERE, help="checkout whose package is imported (default: this one)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--regions", type=int, default=3)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "hair-gs_amd")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("direction_timing.py measures on the GPU; there is none")
    rows = []
    label = args.label or ("this tree" if root == HERE else args.root)

    def emit(row):
        row["tree"] = label
        for k, v in list(row.items()):
            if isinstance(v, float):
                row[k] = round(v, 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    try:
        for leg in args.legs.split(","):
            {"op": op_legs, "step": step_legs, "bench": bench_leg}[leg](args, emit)
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
