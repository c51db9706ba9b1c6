"""Timing of the magnet term's device op (include/hgs.h hgs_magnet_*) and of the iteration that carries it.

  op      the op alone at 2 10^3, 2 10^4 and 2 10^5 strand ends (strands of 4 segments rooted on a sphere), forward and
          forward + backward, under both search paths, and hgs_knn3 alone on the same valid ends: device events around
          replays of a captured graph that holds --calls calls, medians of --reps replays after one warm-up replay
  step    the north_star iteration with lambda_magnet = 0.1: op-by-op eager (training_step: what training() runs without
          --fused_magnet, launch by launch), fused eager, fused captured (1 and 8 steps per graph launch); the fused captured
          step with the term off, and the same with Adam as a launch of its own (opt.inline_adam off: what Adam leaving the
          backward's lanes costs, apart from the term): a host clock around --steps optimizer steps that end in a
          synchronise, after --warmup steps, --regions times
  bench   `python bench.py --gpus 1 --steps 100 --warmup 10` of the tree, in a child process: its result line

The captured op-by-op iteration with the term is NOT among the legs: its statement picks rows on the host, a capture refuses it
(hipErrorStreamCaptureUnsupported; recorded once), and training() does not try.

--root DIR imports the package of another checkout (built there) instead of this one, --label names it in the rows: the parent
commit's numbers come from its own tree; legs that need --fused_magnet are skipped where the tree has no such option.
Prints one JSON line per leg.  --out FILE holds {"rows": [...]}; --append adds to the rows already there, so that
profiles/magnet_timing.json is what these write, one after the other, in one session on one box:
  python tools/magnet_timing.py --out profiles/magnet_timing.json
  python tools/magnet_timing.py --root <parent checkout> --label "parent commit" --append --out profiles/magnet_timing.json
  (repeat both with --legs bench --append for the alternated bench.py lines)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


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


def op_legs(args, emit):
    import torch
    import hgs_runtime as rt
    from scene.hair_gaussian_model import HairGaussianModel
    from synthetic import strand_polylines
    have_op = "hgs_magnet_forward" in rt.SIGNATURES
    for n_ends in (2000, 20000, 200000):
        m = HairGaussianModel.from_strands(strand_polylines(n_ends // 2, 4, seed=3), device="cuda")
        ep = m._endpoints
        u, c = torch.unique(m.endpoint_pairs, return_counts=True)
        ends = u[c == 1]
        pts = ep.detach()[ends].contiguous()
        calls = max(2, min(args.calls, 2000000 // n_ends))
        idx = torch.empty((pts.shape[0], 3), dtype=torch.int32, device="cuda")
        d2 = torch.empty((pts.shape[0], 3), dtype=torch.float32, device="cuda")

        def knn():
            rt.check(rt.lib().hgs_knn3(rt.current_stream(), pts.shape[0], rt.ptr(pts), rt.ptr(idx), rt.ptr(d2)))
        emit(dict(leg="op", what="hgs_knn3 alone", ends=n_ends, calls_per_graph=calls, **_events(knn, calls, args.reps)))
        if not have_op:
            continue
        from hgs_runtime import fused as F
        table = F.MagnetTable(m)
        for mode, name in ((0, "tiles"), (1, "grid")):
            was = F.set_magnet_search(mode)
            try:
                def fwd():
                    with torch.no_grad():
                        F.magnet_loss(ep, table, m.min_val)

                def fwd_bwd():
                    ep.grad = None
                    F.magnet_loss(ep, table, m.min_val).backward()
                emit(dict(leg="op", what="magnet forward", search=name, ends=n_ends, calls_per_graph=calls,
                          **_events(fwd, calls, args.reps)))
                emit(dict(leg="op", what="magnet forward + backward", search=name, ends=n_ends, calls_per_graph=calls,
                          **_events(fwd_bwd, calls, args.reps)))
            finally:
                F.set_magnet_search(was)


def step_legs(args, emit):
    import torch
    from arguments import OptimizationParams
    from diff_gaussian_rasterization import _C as raster
    from synthetic import build_workload
    from train import GraphedStep, ViewSampler, fused_step_applicable, training_step
    from utils.general import safe_state
    have_flag = hasattr(OptimizationParams(), "fused_magnet")
    legs = [("op-by-op eager", 0.1, False, False, 1, True)]
    if have_flag:
        legs += [("fused eager", 0.1, True, False, 1, True), ("fused captured", 0.1, True, True, 1, True),
                 ("fused captured, 8 steps per launch", 0.1, True, True, 8, True)]
    legs += [("fused captured, term off", 0.0, False, True, 1, True),
             ("fused captured, term off, Adam as its own launch", 0.0, False, True, 1, False),
             ("fused captured, term off, 8 steps per launch", 0.0, False, True, 8, True),
             ("fused captured, term off, 8 steps per launch, Adam as its own launch", 0.0, False, True, 8, False)]
    for name, lam, flag, graph, spg, inline in legs:
        if (args.only and args.only != name) or name in args.skip:
            continue
        safe_state(True)
        model, cams, extent = build_workload("north_star", device="cuda", seed=0)
        opt = OptimizationParams()
        opt.enable_topology = False
        opt.lambda_magnet = lam
        if have_flag:
            opt.fused_magnet = flag
        opt.inline_adam = inline
        model.training_setup(opt)
        bg = torch.zeros(3, dtype=torch.float32, device="cuda")
        sampler = ViewSampler(cams, seed=0)
        fused_ok = bool(fused_step_applicable(model, opt))
        it = 0
        try:
            if graph:
                gs = GraphedStep(model, cams, opt, bg, extent=extent, steps_per_graph=spg if fused_ok else 1)
                gs.capture(cams, iteration=1)

                def run(n):
                    nonlocal it
                    K = gs.steps_per_graph
                    while K > 1 and n >= K:
                        gs.step_many([sampler.next() for _ in range(K)], it + 1)
                        it += K
                        n -= K
                    for _ in range(n):
                        it += 1
                        gs.step(sampler.next(), it)
            else:
                fused = None
                if fused_ok:
                    from hgs_runtime.strand_step import fused_step_for
                    fused = fused_step_for(model, cams, opt, bg)
                    fused.defer_tail = True

                def run(n):
                    nonlocal it
                    for _ in range(n):
                        it += 1
                        training_step(model, sampler.next(), opt, bg, it, extent=extent, fused=fused)
            run(args.warmup)
            regions = []
            for _ in range(args.regions):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize()
                regions.append(args.steps / (time.perf_counter() - t0))
            inline_on = bool(gs.inline_adam) if graph else False
            if graph:
                gs.check()
            emit(dict(leg="step", what=name, adam_in_backward_lanes=inline_on, workload="north_star", lambda_magnet=lam, fused_iteration=fused_ok, steps=args.steps,
                      iters_per_sec_median=statistics.median(regions), iters_per_sec_min=min(regions),
                      iters_per_sec_max=max(regions)))
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
    ap.add_argument("--only", default=None, help="step legs: run the one with this name")
    ap.add_argument("--skip", action="append", default=[], help="step legs: leave the one with this name out (repeatable)")
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
        raise SystemExit("magnet_timing.py measures on the GPU; there is none")
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
        _write(args, rows)


def _write(args, rows):
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
