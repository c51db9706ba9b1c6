"""Command-line driver of the training loop (scene/training.py, which holds the step, the captured-graph step, the loop and the
view-parallel exchange).  The benchmark, the tools and the tests reach the loop through this module's names, so they are imported
here by name; main() is this file's own."""
import os

import torch
import torch.distributed as dist

from scene.training import (GraphedStep, ViewParallel, ViewSampler, _EventInfo, _training_step,  # noqa: F401
                            fused_step_applicable, topology_due, training, training_step)


def main(argv=None):
    """Command-line driver (reference train.py:38-131, 256-265 without logger / viewer / evaluation):
      python train.py -s <colmap scene> -m <model dir> [--iterations N] [--save_frequency K]
    Resumes from the newest <model dir>/point_cloud/iteration_*/point_cloud.ply (Gaussian cloud = Stage I, strand model =
    Stage III) or starts Stage I from the sparse COLMAP points; saves every save_frequency iterations and at the end.
    --lambda_head L (this package's own, off by default) adds the head-penetration term to a strand model's loss; it needs
    <scene>/head_sdf.npz, which head_sdf.py builds (utils/head_sdf.py).
    --lambda_direction L --direction_field PATH [--direction_min_conf 0.5] (this package's own, off by default) adds the 3-D direction
    term to a strand model's loss: every segment is aligned with the hair line that the capture's direction volume, the .npz that
    trace_strands.py --field PATH [--fill N] writes, holds at its midpoint (utils/direction_term.py)."""
    from argparse import ArgumentParser
    from arguments import GeneralParams, ModelParams, OptimizationParams
    from scene import Scene
    from utils.general import safe_state
    parser = ArgumentParser(description="Training script parameters")
    mp, op, gp = ModelParams(parser), OptimizationParams(parser), GeneralParams(parser)
    args = parser.parse_args(argv)
    head_sdf = None
    if float(args.lambda_head) > 0:
        # the head-penetration term needs the head's distance field: looked for before anything is loaded or written
        from utils.head_sdf import load_sdf, scene_sdf_path
        path = scene_sdf_path(os.path.abspath(args.source_path))
        if not os.path.exists(path):
            raise SystemExit(f"train.py: --lambda_head {args.lambda_head} needs {path}: head_sdf.py -s <scene> builds it from the "
                             "capture's head mesh")
        try:
            head_sdf = load_sdf(path)
        except ValueError as e:
            raise SystemExit(f"train.py: {e}") from None
    direction_volume = None
    if float(args.lambda_direction) > 0:
        # the 3-D direction term needs the capture's direction volume: looked for before anything is loaded or written
        from utils.direction_term import DirectionVolume
        path = os.path.abspath(args.direction_field) if args.direction_field else ""
        if not path or not os.path.isfile(path):
            raise SystemExit(f"train.py: --lambda_direction {args.lambda_direction} needs --direction_field PATH, the direction volume "
                             f"that trace_strands.py --field PATH writes ({path or 'no path given'}: no such file)")
        try:
            direction_volume = DirectionVolume.load(path)
        except ValueError as e:
            raise SystemExit(f"train.py: {e}; trace_strands.py --field PATH writes a direction volume") from None
    # view-parallel run (python -m torch.distributed.run ... train.py): one process per GPU, initialised before anything
    # touches the GPU; every rank seeds identically (replicated topology operators draw the same random numbers), rank 0
    # alone writes to the model directory
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        # (HGS_DIST_BACKEND=gloo: ranks may share a GPU -- RCCL needs one per rank --, which is how the tests run this path
        # on a one-GPU box)
        backend = os.environ.get("HGS_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
        if torch.cuda.is_available():
            local = local % torch.cuda.device_count() if backend == "gloo" else local
            torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
    safe_state(args.quiet or rank != 0)
    if rank == 0:
        os.makedirs(args.model_path, exist_ok=True)
        with open(os.path.join(args.model_path, "cfg_args"), "w") as fh:   # what render.py's get_combined_args reads back
            fh.write(str(args))
    # Every rank loads the capture at the same time: the one shared file a first run creates -- sparse/0/points3D.ply -- is
    # written under a private name and renamed into place (data/dataset_readers.py: whoever converts, every reader sees a
    # complete file), and the model directory's input.ply / cameras.json are rank 0's alone (scene/scene.py).
    scene = Scene(mp.extract(args))
    if world > 1:
        dist.barrier()
    opt = op.extract(args)
    g = scene.gaussians
    if head_sdf is not None:
        g.head_sdf = head_sdf    # rides on the model: loss/losses.py and hgs_runtime/strand_step.py read gaussians.head_sdf
    if direction_volume is not None:
        from scene.hair_gaussian_model import HairGaussianModel
        if isinstance(g, HairGaussianModel):
            g.direction_volume = direction_volume    # rides on the model like head_sdf: the same two readers
        elif rank == 0:
            print("train.py: --lambda_direction applies to strand models only; this Stage-I run goes on without the term")
    g.training_setup(opt)
    cams = scene.getCameras()
    vp = ViewParallel()
    sampler = ViewSampler(cams, seed=0, rank=vp.rank, world=vp.world)   # ONE view order for the whole run
    # As in the reference (train.py:91-92, 251-253), `iteration` counts from 1 in EVERY invocation -- the learning-rate
    # schedule, the SH-degree bumps and the operators' intervals restart with each stage of the workflow -- and only the
    # name of a saved iteration adds what the model had when it was loaded.
    base, total, every = scene.loaded_iter, int(opt.iterations), max(1, int(args.save_frequency))
    eval_every = max(1, int(getattr(args, "eval_frequency", 30000)))

    def evaluate(iteration):
        """The reference's evaluation hook (train.py:229-246): strand metrics against the capture's ground truth, where it
        has one (hair_eval_data.npz), every eval_frequency iterations and at the end; rank 0 only.  On the CPU (cKDTree) unless
        --eval_device names a GPU (csrc/hgs_metrics.hip: the same dict)."""
        import numpy as np
        from loss.metrics import compute_eval_data_from_gs, compute_eval_data_from_hair_gs, compute_metrics
        from scene.hair_gaussian_model import HairGaussianModel
        pred = compute_eval_data_from_hair_gs(g) if isinstance(g, HairGaussianModel) else compute_eval_data_from_gs(g)
        dev = getattr(args, "eval_device", "cpu")
        scene.eval_metrics, scene.eval_thresholds = compute_metrics(pred=pred, gt=scene.gt, bidirectional=bool(opt.bidirectional_eval),
                                                                    device=None if dev == "cpu" else dev)
        if not args.quiet:
            print(f"[it {iteration}] " + "  ".join(f"{k} {np.round(np.asarray(v), 3).tolist()}" for k, v in scene.eval_metrics.items())
                  + f"  at {scene.eval_thresholds}")

    it = 0
    while it < total:
        n = min(every - it % every, total - it)
        if scene.gt is not None:
            n = min(n, eval_every - it % eval_every)
        ema = training(g, cams, opt, iterations=n, extent=scene.cameras_extent, start_iteration=it, vp=vp, sampler=sampler,
                       log_every=0 if (args.quiet or rank != 0) else max(1, n // 4))
        it += n
        if rank == 0 and scene.gt is not None and (it % eval_every == 0 or it == total):
            evaluate(base + it)
        if rank == 0 and (it % every == 0 or it == total):
            scene.save(it)                  # (Scene.save adds the loaded iteration, like the reference's)
            if not args.quiet:
                print(f"[it {base + it}] saved; loss(ema) {float(ema):.6f}")
        if world > 1:
            dist.barrier()
    if world > 1:
        dist.destroy_process_group()
    return scene


if __name__ == "__main__":
    main()
