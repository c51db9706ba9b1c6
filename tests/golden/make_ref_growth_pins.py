"""Generates tests/golden/ref_growth_pins.npz by RUNNING the reference's own growing() (scene/hair_gaussian_model.py:1098-1200) on
the CPU of the authoring container (never on the GPU box).  Only numeric inputs and outputs are stored.

Two stages, two processes, as in make_ref_topology_pins.py (both packages are called `scene` / `utils` / `arguments`):
  --stage inputs     (this repository's package) tests/test_growth_cpu.py's `growth_model` -- test_topology_restatement_cpu's
                     `_random_model` with degree-3 f_rest rows, cut tips, collapsed last segments, every segment in the
                     foreground -- dumped as arrays;
  --stage reference  (/root/reference only on sys.path) each state is loaded into the REFERENCE's HairGaussianModel
                     (make_ref_topology_pins._ref_model), which runs its own compute_strands_info() and growing(), unedited, for
                     growth_averaging_points in {1, 3, 5, 10} and growth_length in {0.002, None}.
The reference's growing() cannot complete on its own: on a CPU model it calls .numpy() on parameters that require grad (so the six
parameters are set to requires_grad_(False) first), and it calls cat_segments without `new_masks` (a TypeError).  The instance's
cat_segments is therefore replaced by a recorder that keeps the six arrays the reference passes, and the masks it computed and
left out are read from the caller's local `new_masks`.  What is stored is exactly what the reference computed.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "ref_growth_pins.npz")
TMP_IN = os.path.join(HERE, "_growth_inputs.npz")

SEEDS = list(range(6))
KS = [1, 3, 5, 10]
LENGTHS = [0.002, None]
NOTHING = 6                 # a model whose every strand is at num_points_strand = 1: nothing grows


def stage_inputs():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "hair-gs_amd")]
    from tests import test_growth_cpu as G
    out = {}
    for seed in SEEDS + [NOTHING]:
        m = G.growth_model(seed)
        k = f"s{seed}_"
        out[k + "pairs"] = m.endpoint_pairs.numpy().astype(np.int64)
        for g in m.optimizer.param_groups:
            p = g["params"][0]
            st = m.optimizer.state.get(p, {})
            out[k + g["name"]] = p.detach().numpy()
            out[k + g["name"] + "_exp_avg"] = st["exp_avg"].numpy()
            out[k + g["name"] + "_exp_avg_sq"] = st["exp_avg_sq"].numpy()
        out[k + "has_state"] = np.bool_(True)
        out[k + "grad_accum"] = m.xyz_gradient_accum.numpy()
        out[k + "denom"] = m.denom.numpy()
        out[k + "max_radii2D"] = m.max_radii2D.numpy()
        out[k + "ref_strand_root"] = np.asarray(m.ref_strand_root, dtype=np.float64)
        out[k + "root_idx"] = m.strand_root_endpoint_idx.numpy().astype(np.int64)
        out[k + "active_sh_degree"] = np.int64(m.active_sh_degree)
        out[k + "num_points_strand"] = np.int64(1 if seed == NOTHING else m.training_args.num_points_strand)
    np.savez_compressed(TMP_IN, **out)
    print("inputs:", len(out), "arrays")


class _Info:
    def __init__(self):
        self.densification_info = {}


def stage_reference():
    sys.path.insert(0, HERE)
    from _ref_harness import enter_reference
    enter_reference()
    import torch
    from arguments import OptimizationParams
    from scene.hair_gaussian_model import HairGaussianModel
    from make_ref_topology_pins import _ref_model
    opt = OptimizationParams(argparse.ArgumentParser())
    inp = np.load(TMP_IN)
    out = {}
    for k in inp.files:                   # (the model inputs the test rebuilds and checks: pairs and parameters)
        if k.split("_", 1)[1] in ("pairs", "endpoints", "f_dc", "f_rest", "opacity", "mask", "width"):
            out[k] = inp[k]
    cases = []
    runs = [(s, kk, gl) for s in SEEDS for kk in KS for gl in LENGTHS] + [(NOTHING, 3, 0.002)]
    for seed, kk, gl in runs:
        tag = f"s{seed}"
        opt.num_points_strand = int(inp[tag + "_num_points_strand"])
        opt.growth_averaging_points = kk
        m = _ref_model(inp, tag, torch, HairGaussianModel, opt)
        m.compute_strands_info()
        for p in (m._endpoints, m._features_dc, m._features_rest, m._opacity, m._mask, m._width):
            p.requires_grad_(False)
        rec = {}

        def recorder(*args):
            rec["args"] = [a.detach().numpy().copy() for a in args]
            rec["masks"] = np.asarray(sys._getframe(1).f_locals["new_masks"]).copy()
        m.cat_segments = recorder
        info = _Info()
        m.growing(info, growth_length=gl)
        pairs, ep, dc, rest, op, wd = rec["args"]
        c = int(info.densification_info["grow"])
        case = f"{tag}_k{kk}_{'none' if gl is None else 'fixed'}"
        key = f"case_{case}_"
        out[key + "model"] = np.array(tag)
        out[key + "k"] = np.int64(kk)
        out[key + "num_points_strand"] = np.int64(opt.num_points_strand)
        out[key + "growth_length"] = np.float64(np.nan if gl is None else gl)
        out[key + "grow"] = np.int64(c)
        out[key + "pairs"] = pairs.astype(np.int64).reshape(c, 2)
        out[key + "endpoints"] = ep.astype(np.float32).reshape(c, 3)
        out[key + "f_dc"] = dc.astype(np.float32).reshape((c,) + inp[tag + "_f_dc"].shape[1:])
        out[key + "f_rest"] = rest.astype(np.float32).reshape((c,) + inp[tag + "_f_rest"].shape[1:])
        out[key + "opacity"] = op.astype(np.float32).reshape(c, 1)
        out[key + "mask"] = rec["masks"].astype(np.float32).reshape(c, 1)
        out[key + "width"] = wd.astype(np.float32).reshape(c, 1)
        # (an empty growth gives float64 arrays of shape (0,): only then may the dtype change above)
        assert c == 0 or all(a.dtype == (np.int64 if i == 0 else np.float32) for i, a in enumerate(rec["args"] + [rec["masks"]]))
        cases.append(case)
    out["meta_cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    os.remove(TMP_IN)
    print(f"reference runs: {len(cases)}; wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KB, {len(out)} arrays)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", choices=["all", "inputs", "reference"], default="all")
    a = ap.parse_args()
    if a.stage == "inputs":
        stage_inputs()
    elif a.stage == "reference":
        stage_reference()
    else:
        for st in ("inputs", "reference"):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", st], check=True)
