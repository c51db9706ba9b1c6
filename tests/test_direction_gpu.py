"""The 3-D direction term on the GPU (csrc/hgs_direction.hip): hgs_runtime.fused.direction_loss on every case of
tests/direction_cases.py against the numpy path of utils/direction_term.py (per-segment term, weight and gradient and the endpoint
gradient bit for bit, the value within one ulp); the term inside the fused and the captured iteration against the op-by-op one, at
tests/test_head_sdf_gpu.py's bars; after a topology change; and through train.py."""
import os

import numpy as np
import pytest
import torch

from tests import direction_cases as DC
from tests.test_direction_cpu import numpy_path
from utils import direction_term as D
from utils.trace import Field, save_field

pytestmark = pytest.mark.gpu


# ---- the op --------------------------------------------------------------------------------------------------------------
def _run(name, upstream=None, own_scratch=False):
    from hgs_runtime import fused as F
    vol, pts, pairs, min_conf = DC.case(name)
    p = torch.tensor(pts, dtype=torch.float32, device="cuda").reshape(-1, 3).requires_grad_(True)
    table = F.DirectionTable(torch.as_tensor(pairs, device="cuda").reshape(-1, 2), p.shape[0])
    scratch = F.DirectionScratch(table.S, table.E, "cuda") if own_scratch else None
    info = {}
    v = F.direction_loss(p, table, vol, min_conf, info, scratch)
    (v if upstream is None else v * upstream).backward()
    torch.cuda.synchronize()
    return dict(value=np.float32(v.detach().cpu().numpy()), d_points=p.grad.cpu().numpy(), term=info["term"].cpu().numpy(),
                w=info["w"].cpu().numpy(), gs=info["gs"].cpu().numpy(), active=F.direction_active(info),
                offsets=table.offsets.cpu().numpy(), entries=table.entries.cpu().numpy())


@pytest.mark.parametrize("name", DC.NAMES)
def test_direction_loss_against_the_numpy_path(name):
    want = numpy_path(name)
    _, pts, pairs, _ = DC.case(name)
    got, again = _run(name), _run(name)
    offsets, entries = D.incidence(pairs, pts.shape[0])
    assert got["offsets"].tobytes() == offsets.tobytes() and got["entries"].tobytes() == entries.tobytes()
    for k in ("term", "w", "gs", "d_points"):
        assert got[k].dtype == np.float32 and got[k].tobytes() == want[k].tobytes(), k
    assert got["active"] == want["active"]
    # the float64 sum's order is the only difference: at most S 2^-53 of the sum before the one rounding, so one float32 ulp at most
    print(f"value | direction_loss | {name} | kernel {got['value']!r} | numpy {want['value']!r} | active {got['active']} |")
    assert abs(float(got["value"]) - float(want["value"])) <= float(np.spacing(np.float32(want["value"])))
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k           # two calls: equal bits
    up = _run(name, upstream=0.37)
    assert up["d_points"].tobytes() == numpy_path(name, upstream=0.37)["d_points"].tobytes()  # one float32 multiplication
    kept = _run(name, own_scratch=True)
    assert kept["d_points"].tobytes() == got["d_points"].tobytes() and kept["value"] == got["value"]


def test_stale_scratch_bad_pairs_and_cpu_tensors_are_refused():
    import hgs_runtime as rt
    from hgs_runtime import fused as F
    vol = DC.volume("vol2")
    pairs = torch.tensor([[0, 1], [1, 2], [2, 3]], device="cuda")
    table = F.DirectionTable(pairs, 5)
    pts = torch.zeros(5, 3, device="cuda")
    for stale in (F.DirectionScratch(2, 5, "cuda"), F.DirectionScratch(3, 4, "cuda")):
        with pytest.raises(rt.HgsError, match="topology event"):
            F.direction_loss(pts, table, vol, 0.5, None, stale)
    with pytest.raises(rt.HgsError, match="topology event"):
        F.direction_loss(torch.zeros(6, 3, device="cuda"), table, vol, 0.5)
    with pytest.raises(rt.HgsError):
        F.direction_loss(torch.zeros(5, 3), table, vol, 0.5)
    with pytest.raises(rt.HgsError):
        F.DirectionTable(pairs.cpu(), 5)
    for bad in ([[0, 5]], [[-1, 0]]):
        with pytest.raises(rt.HgsError, match="endpoint ids"):
            F.DirectionTable(torch.tensor(bad, device="cuda"), 5)
    assert float(F.direction_loss(pts, table, vol, 0.5)) == 0.0                            # zero-length segments: inactive


# ---- the step ------------------------------------------------------------------------------------------------------------
def _volume_around(model):
    """An analytic swirl of 33^3 nodes over the box of the model's joints: line ~ (-y, x, -0.5) about their centre with a random sign
    per node, conf 1 everywhere."""
    ep = model._endpoints.detach().cpu().numpy().astype(np.float64)
    c = ep.mean(axis=0)
    lo, hi = ep.min(axis=0), ep.max(axis=0)
    L = float((hi - lo).max())
    origin, h = lo - 0.1 * L, 1.2 * L / 32
    z, y, x = np.meshgrid(*(origin[k] + h * np.arange(33) for k in (2, 1, 0)), indexing="ij")
    d = np.stack([-(y - c[1]), x - c[0], np.full_like(x, -0.5 * L)], axis=-1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    d = d * np.random.default_rng(8).choice([-1.0, 1.0], size=x.shape)[..., None]
    return D.DirectionVolume(Field(origin, h, (33, 33, 33), d, np.ones_like(x)))


def _tiny(lambda_direction, perturb=True, volume=True):
    from arguments import OptimizationParams
    from synthetic import build_workload
    from utils.general import safe_state
    safe_state(True)
    model, cams, extent = build_workload("tiny", device="cuda", with_targets=True)
    opt = OptimizationParams()
    opt.enable_topology = False
    opt.lambda_direction = lambda_direction
    model.training_setup(opt)
    if perturb:      # off the point the synthetic targets were rendered at (tests/test_gpu_train.py: the L1 term's sign)
        g = torch.Generator(device="cuda").manual_seed(5)
        with torch.no_grad():
            model._features_dc.add_(0.2 * torch.randn(model._features_dc.shape, device="cuda", generator=g))
            model._endpoints.add_(0.003 * torch.randn(model._endpoints.shape, device="cuda", generator=g))
            model._opacity.add_(0.3 * torch.randn(model._opacity.shape, device="cuda", generator=g))
            model._mask.add_(0.3 * torch.randn(model._mask.shape, device="cuda", generator=g))
    if volume:
        model.direction_volume = _volume_around(model)
    return model, cams, extent, opt, torch.zeros(3, device="cuda")


def test_switch_and_step_surface():
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import loss_function_single_pass
    from train import fused_step_applicable
    model, cams, _, opt, bg = _tiny(0.0, perturb=False)
    assert fused_step_applicable(model, opt)
    off = FusedStrandStep(model, cams, opt, bg)
    assert off.direction is None and off.inline_adam_possible()                            # the volume alone switches nothing on
    off.views.select(0)
    off.loss()
    assert "direction" not in off.terms()
    _, terms, _ = loss_function_single_pass(model, cams[0], opt, bg)
    assert "direction" not in terms
    opt.lambda_direction = 0.5
    assert fused_step_applicable(model, opt)
    step = FusedStrandStep(model, cams, opt, bg)
    assert step.direction_volume is model.direction_volume and step.direction.S == model.endpoint_pairs.shape[0] == 1200
    assert step.direction_scratch.S == 1200 and step.direction_scratch.E == model._endpoints.shape[0]
    assert step.direction is FusedStrandStep(model, cams, opt, bg).direction               # remembered on the model
    assert not step.inline_adam_possible() and step.enable_inline_adam(True) is False
    step.views.select(0)
    loss, _ = step.loss()
    value = float(step.terms()["direction"])
    assert torch.isfinite(loss) and np.isfinite(value) and value > 0
    _, terms, _ = loss_function_single_pass(model, cams[0], opt, bg)
    assert "direction" in terms
    del model.direction_volume                                                           # no volume on the model: no term
    assert FusedStrandStep(model, cams, opt, bg).direction is None


def test_fused_iteration_with_the_term_matches_op_by_op():
    """tests/test_head_sdf_gpu.py's comparison with the direction term in the head term's place: 2e-5 on the loss and the terms, 2e-4
    of scale on every gradient.  lambda_direction is set from the op-by-op gradients so that the term's largest endpoint gradient is of
    the order of the rasterizer's."""
    from hgs_runtime import fused as F
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import loss_function_single_pass, strand_direction_loss
    model, cams, _, opt, bg = _tiny(0.0)
    params = [model._endpoints, model._width, model._opacity, model._mask, model._features_dc, model._features_rest]

    def clear():
        for p in params:
            p.grad = None
    cam = cams[2]
    clear()
    loss, _, _ = loss_function_single_pass(model, cam, opt, bg)
    loss.backward()
    g_raster = float(model._endpoints.grad.abs().max())
    clear()
    strand_direction_loss(model, model.direction_volume, opt.direction_min_conf).backward()
    g_term = model._endpoints.grad.clone()
    lam = g_raster / float(g_term.abs().max())
    assert np.isfinite(lam) and lam > 0
    clear()
    table = F.DirectionTable.of(model)
    F.direction_loss(model._endpoints, table, model.direction_volume, opt.direction_min_conf).backward()
    g_op = model._endpoints.grad.clone()
    assert (g_op - g_term).abs().max() <= 2e-4 * float(g_term.abs().max())
    clear()
    plain = FusedStrandStep(model, cams, opt, bg)
    plain.views.select(plain.views.index[id(cam)])
    l0, _ = plain.loss()
    plain.backward(l0)
    g_without = model._endpoints.grad.clone()
    opt.lambda_direction = lam
    fused = FusedStrandStep(model, cams, opt, bg)
    assert fused.direction is table
    for ci in (2, 0):
        cam = cams[ci]
        clear()
        loss, terms, _ = loss_function_single_pass(model, cam, opt, bg)
        loss.backward()
        ref = dict(loss=float(loss.detach()), terms={k: float(v.detach()) for k, v in terms.items()}, grads=[p.grad.clone() for p in params])
        assert ref["terms"]["direction"] > 0
        clear()
        fused.views.select(fused.views.index[id(cam)])
        floss, _ = fused.loss()
        if ci == 2:
            fused.backward(floss)
        else:
            floss.backward()
        fterms = {k: float(v) for k, v in fused.terms().items()}
        total = float(floss.detach())
        print(f"step | total {total!r} vs {ref['loss']!r} | direction {fterms['direction']!r} vs {ref['terms']['direction']!r} | lambda {lam!r}")
        assert abs(total - ref["loss"]) <= 2e-5 * abs(ref["loss"]), (total, ref["loss"])
        for k, v in ref["terms"].items():
            assert abs(fterms[k] - v) <= 2e-5 * max(abs(v), 1e-3), (k, fterms[k], v)
        assert abs(fterms["direction"] - ref["terms"]["direction"]) <= 2e-5 * abs(ref["terms"]["direction"])
        for name, p, gref in zip(("endpoints", "width", "opacity", "mask", "f_dc", "f_rest"), params, ref["grads"]):
            if gref.numel() == 0:
                continue
            scale = float(gref.abs().max())
            assert (p.grad - gref).abs().max() <= 2e-4 * max(scale, 1e-12), (name, float((p.grad - gref).abs().max()), scale)
        if ci == 2:
            # with the term minus without it = lambda times the op's own gradient.  Float32 roundings between the two sides: the
            # upstream enters as (lambda / S) against lambda * (1 / S) and the product (2 of the term's part), autograd's sum of the two
            # gradients (1 of the sum), the subtraction here (1 of the difference): 4 ulp of the largest summed entry bound them all
            want = lam * g_op
            with_term = model._endpoints.grad
            err = float((with_term - g_without - want).abs().max())
            bar = 4 * 2.0 ** -23 * max(float(with_term.abs().max()), float(g_without.abs().max()), float(want.abs().max()))
            print(f"step | with - without - lambda * op | worst {err!r} | bar {bar!r}")
            assert err <= bar, (err, bar)
            assert float(want.abs().max()) >= 0.5 * g_raster


def test_graphed_step_with_the_term_matches_eager_steps():
    """tests/test_head_sdf_gpu.py's graph-against-eager comparison with the direction term on, asserted as that file asserts it."""
    from diff_gaussian_rasterization import _C as raster
    from hgs_runtime.strand_step import FusedStrandStep
    from train import GraphedStep, training_step
    order = [1, 3, 0, 2, 1, 0, 3, 2]
    results = {}
    try:
        for mode in ("eager", "graph", "without"):
            model, cams, extent, opt, bg = _tiny(0.0 if mode == "without" else 0.05, perturb=False)
            losses = []
            if mode != "graph":
                fused = FusedStrandStep(model, cams, opt, bg)
                assert (fused.direction is not None) == (mode == "eager")
                for it, ci in enumerate(order, 1):
                    loss, terms, _ = training_step(model, cams[ci], opt, bg, it, extent=extent, fused=fused)
                    assert ("direction" in terms) == (mode == "eager")
                    losses.append(float(loss))
            else:
                gs = GraphedStep(model, cams, opt, bg, extent=extent, steps_per_graph=1)
                assert gs.fused is not None and gs.fused.direction is not None
                gs.capture(cams)
                assert not gs.inline_adam
                for it, ci in enumerate(order, 1):
                    losses.append(float(gs.step(cams[ci], it)))
                assert min(gs.check()) > 0
                raster.set_async(False)
            results[mode] = (losses, model._endpoints.detach().clone(), model._opacity.detach().clone(), model.denom.clone(),
                             model.xyz_gradient_accum.clone())
    finally:
        raster.set_async(False)
    le, lg = results["eager"][0], results["graph"][0]
    assert np.allclose(le, lg, rtol=1e-4, atol=1e-6), (le, lg)
    for a, b in zip(results["eager"][1:], results["graph"][1:]):
        assert (a - b).abs().max() <= 1e-4 * max(1e-6, float(a.abs().max()))
    assert (results["without"][1] - results["eager"][1]).abs().max() > 0                  # the term did move the joints


def test_term_follows_a_topology_change():
    """A prune that changes S and E, then refresh(): table and scratch follow, the fused term equals the op-by-op term on the changed
    model, and the stale scratch is refused."""
    from hgs_runtime import fused as F
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import strand_direction_loss
    model, cams, _, opt, bg = _tiny(1.0, perturb=False)
    step = FusedStrandStep(model, cams, opt, bg)
    before, table_before = step.direction_scratch, step.direction
    E0, S0 = model._endpoints.shape[0], model.endpoint_pairs.shape[0]
    mask = torch.zeros(S0, dtype=torch.bool, device="cuda")
    mask[7::30] = True                       # segment 7 of every strand: 40 strands become 80
    mask[29] = True                          # and strand 0's last segment: its tip endpoint goes
    model.prune_segments(mask)
    model.compute_strands_info()
    step.refresh()
    E, S = model._endpoints.shape[0], model.endpoint_pairs.shape[0]
    assert E == E0 - 1 and S == S0 - 41
    assert step.direction is not table_before and (step.direction.S, step.direction.E) == (S, E)
    assert step.direction_scratch is not before and (step.direction_scratch.S, step.direction_scratch.E) == (S, E)
    offsets, entries = D.incidence(model.endpoint_pairs.cpu().numpy(), E)
    assert step.direction.offsets.cpu().numpy().tobytes() == offsets.tobytes() and step.direction.entries.cpu().numpy().tobytes() == entries.tobytes()
    model._endpoints.grad = None
    ref = strand_direction_loss(model, model.direction_volume, opt.direction_min_conf)
    ref.backward()
    g_ref = model._endpoints.grad.clone()
    model._endpoints.grad = None
    step.views.select(1)
    step.loss()
    got, want = float(step.terms()["direction"]), float(ref.detach())
    assert want > 0 and abs(got - want) <= 2e-5 * want
    F.direction_loss(model._endpoints, step.direction, model.direction_volume, opt.direction_min_conf, None, step.direction_scratch).backward()
    assert (model._endpoints.grad - g_ref).abs().max() <= 2e-4 * float(g_ref.abs().max())
    with pytest.raises(Exception, match="topology event"):
        F.direction_loss(model._endpoints, step.direction, model.direction_volume, opt.direction_min_conf, None, before)
    with pytest.raises(Exception, match="topology event"):
        F.direction_loss(model._endpoints, table_before, model.direction_volume, opt.direction_min_conf)


# ---- through the drivers ---------------------------------------------------------------------------------------------------
def test_train_cli_with_a_direction_field(tmp_path, capsys):
    """A field written with utils.trace.save_field on a synthetic scene, a few Stage-III iterations of train.py with
    --lambda_direction: the loss dict has a finite direction entry."""
    import train as train_cli
    from scene.hair_gaussian_model import HairGaussianModel
    from tests.test_dataset_io_cpu import _write_capture, _write_side_files
    from train import training_step
    src, model = tmp_path / "capture", tmp_path / "out"
    _write_capture(src, n_views=3, W=64, H=48)
    _write_side_files(src)
    rng = np.random.default_rng(0)
    pts = np.cumsum(rng.normal(size=(24, 10, 3)) * 0.02, axis=1).astype(np.float32) + rng.normal(size=(24, 1, 3)).astype(np.float32) * 0.2
    hair = HairGaussianModel.from_strands(pts, sh_degree=0, device="cuda", ref_strand_root=pts[:, 0])
    os.makedirs(model / "point_cloud" / "iteration_7")
    hair.save_ply(str(model / "point_cloud" / "iteration_7" / "point_cloud.ply"))
    flat = pts.reshape(-1, 3).astype(np.float64)
    lo, L = flat.min(axis=0), float((flat.max(axis=0) - flat.min(axis=0)).max())
    d = np.zeros((17, 17, 17, 3))
    d[..., 1] = 1.0
    save_field(str(tmp_path / "field.npz"), Field(lo - 0.1 * L, 1.2 * L / 16, (17, 17, 17), d, np.ones((17, 17, 17))))
    scene = train_cli.main(["-s", str(src), "-m", str(model), "--iterations", "8", "--save_frequency", "8", "--quiet",
                            "--lambda_direction", "0.1", "--direction_field", str(tmp_path / "field.npz")])
    g = scene.gaussians
    assert isinstance(g, HairGaussianModel) and g.direction_volume.shape == (17, 17, 17) and torch.isfinite(g._endpoints).all()
    assert os.path.isdir(model / "point_cloud" / "iteration_15")
    from arguments import OptimizationParams
    opt = OptimizationParams()
    opt.enable_topology = False
    opt.lambda_direction = 0.1
    _, terms, _ = training_step(g, scene.getCameras()[0], opt, torch.zeros(3, device="cuda"), 9, extent=scene.cameras_extent)
    assert "direction" in terms and np.isfinite(float(terms["direction"].detach())) and float(terms["direction"].detach()) > 0
