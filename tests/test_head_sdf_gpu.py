"""The head's distance field and the penetration term on the GPU (csrc/hgs_sdf.hip): hgs_mesh_sdf on every mesh case of
tests/head_sdf_cases.py against the numpy path (|phi| bit for bit, signs by decision); hgs_runtime.fused.head_penalty on every point
case (per-point penalty and gradient bit for bit, the value within one ulp, the float64 comparator); the term inside the fused and the
captured iteration against the op-by-op one, at tests/test_magnet_gpu.py's bars; and through head_sdf.py and train.py."""
import os

import numpy as np
import pytest
import torch

from tests import head_sdf_cases as HC
from tests import head_sdf_reference as HR
from tests.test_head_sdf_cpu import built, point_case
from utils import head_sdf as H

pytestmark = pytest.mark.gpu


# ---- the field -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HC.MESH_NAMES)
def test_mesh_sdf_against_the_numpy_path(name):
    verts, faces, grid, pad = HC.mesh_cases()[name]
    cpu, cpu_stats, _, w, _, _ = built(name)
    runs = []
    for _ in range(2):
        stats = {"winding": None}
        runs.append((H.build_sdf(verts, faces, grid=grid, pad=pad, device="cuda", stats=stats), stats))
    sdf, stats = runs[0]
    assert sdf.shape == cpu.shape and sdf.spacing == cpu.spacing and sdf.origin.tobytes() == cpu.origin.tobytes()
    assert np.abs(sdf.phi).tobytes() == np.abs(cpu.phi).tobytes()                         # |phi|: equal bits
    sure = HR.decided(w, HC.NEAR)
    assert (~sure).sum() <= HC.NEAR_SHARE * w.size
    assert ((sdf.phi < 0) == (w > 0.5))[sure].all()
    assert not np.signbit(sdf.phi[sdf.phi == 0]).any()
    assert np.abs(stats["winding"] - w).max() < 1e-9
    assert (stats["dropped"], stats["degenerate"], stats["faces"]) == (cpu_stats["dropped"], cpu_stats["degenerate"], cpu_stats["faces"])
    assert runs[1][0].phi.tobytes() == sdf.phi.tobytes() and runs[1][1]["winding"].tobytes() == stats["winding"].tobytes()


# ---- the op --------------------------------------------------------------------------------------------------------------
def _run(pts, sdf, margin, upstream=None, scratch=None):
    from hgs_runtime.fused import head_penalty
    p = torch.tensor(pts, dtype=torch.float32, device="cuda").reshape(-1, 3).requires_grad_(True)
    info = {}
    v = head_penalty(p, sdf, margin, info, scratch)
    (v if upstream is None else v * upstream).backward()
    torch.cuda.synchronize()
    E = p.shape[0]
    grad = p.grad.cpu().numpy() if E else np.zeros((0, 3), np.float32)
    return dict(value=np.float32(v.detach().cpu().numpy()), grad=grad, pen=info["pen"].cpu().numpy(), dist=info["dist"].cpu().numpy(),
                g=info["g"].cpu().numpy())


@pytest.mark.parametrize("name", HC.POINT_NAMES)
def test_head_penalty_against_the_numpy_path(name):
    sdf, pts, margin = point_case(name)
    E = pts.shape[0]
    pen, g, d, _ = H.sample(pts, sdf, margin)
    L, grad = H.penalty(pts, sdf, margin)
    got, again = _run(pts, sdf, margin), _run(pts, sdf, margin)
    assert got["pen"].tobytes() == pen.tobytes() and got["dist"].tobytes() == d.tobytes() and got["g"].tobytes() == g.tobytes()
    assert got["grad"].tobytes() == grad.tobytes()
    # the float64 sum's order is the only difference: at most E 2^-53 of the sum before the one rounding, so one float32 ulp at most
    print(f"value | head_penalty | {name} | kernel {got['value']!r} | numpy {L!r} |")
    assert abs(float(got["value"]) - float(L)) <= float(np.spacing(np.float32(L)))
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k           # two calls: equal bits
    up = _run(pts, sdf, margin, upstream=0.37)
    assert up["grad"].tobytes() == H.penalty(pts, sdf, margin, 0.37)[1].tobytes()         # one float32 multiplication
    rv, rg = HR.ratios(got["value"], got["grad"], pts, sdf, margin)
    print(f"ratio | head_penalty | {name} | value {rv:.2f} | gradient {rg:.2f} |")
    assert HR.accepts(got["value"], got["grad"], pts, sdf, margin), (rv, rg)
    if name == "ball_all_outside":
        assert got["value"] == 0 and not got["grad"].any()
    if E:
        from hgs_runtime.fused import HeadScratch
        kept = _run(pts, sdf, margin, scratch=HeadScratch(E, "cuda"))
        assert kept["grad"].tobytes() == got["grad"].tobytes() and kept["value"] == got["value"]


def test_stale_scratch_and_cpu_tensors_are_refused():
    import hgs_runtime as rt
    from hgs_runtime.fused import HeadScratch, head_penalty
    sdf = HC.ball_field()
    with pytest.raises(rt.HgsError, match="topology event"):
        head_penalty(torch.zeros(5, 3, device="cuda"), sdf, 0.0, None, HeadScratch(4, "cuda"))
    with pytest.raises(rt.HgsError):
        head_penalty(torch.zeros(5, 3), sdf, 0.0)
    st_dev = H.penetration_stats(HC.special_points(), sdf, device="cuda")
    assert st_dev == H.penetration_stats(HC.special_points(), sdf) and st_dev["inside"] >= 6 and st_dev["joints"] == 28


# ---- the step ------------------------------------------------------------------------------------------------------------
def _field_around(model, share=0.2):
    """An analytic ball about the model's joints that holds about `share` of them: a HeadSDF of 33^3 nodes over their box."""
    ep = model._endpoints.detach().cpu().numpy().astype(np.float64)
    c = ep.mean(axis=0)
    radius = float(np.quantile(np.linalg.norm(ep - c, axis=1), share))
    lo, hi = ep.min(axis=0), ep.max(axis=0)
    L = float((hi - lo).max())
    origin, h = lo - 0.1 * L, 1.2 * L / 32
    z, y, x = np.meshgrid(*(origin[k] + h * np.arange(33) for k in (2, 1, 0)), indexing="ij")
    phi = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius
    return H.HeadSDF(origin, h, (33, 33, 33), phi.astype(np.float32))


def _tiny(lambda_head, margin=0.0, perturb=True, field=True):
    from arguments import OptimizationParams
    from synthetic import build_workload
    from utils.general import safe_state
    safe_state(True)
    model, cams, extent = build_workload("tiny", device="cuda", with_targets=True)
    opt = OptimizationParams()
    opt.enable_topology = False
    opt.lambda_head, opt.head_margin = lambda_head, margin
    model.training_setup(opt)
    if perturb:      # off the point the synthetic targets were rendered at (tests/test_gpu_train.py: the L1 term's sign)
        g = torch.Generator(device="cuda").manual_seed(5)
        with torch.no_grad():
            model._features_dc.add_(0.2 * torch.randn(model._features_dc.shape, device="cuda", generator=g))
            model._endpoints.add_(0.003 * torch.randn(model._endpoints.shape, device="cuda", generator=g))
            model._opacity.add_(0.3 * torch.randn(model._opacity.shape, device="cuda", generator=g))
            model._mask.add_(0.3 * torch.randn(model._mask.shape, device="cuda", generator=g))
    if field:
        model.head_sdf = _field_around(model)
    return model, cams, extent, opt, torch.zeros(3, device="cuda")


def test_switch_and_step_surface():
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import loss_function_single_pass
    from train import fused_step_applicable
    model, cams, _, opt, bg = _tiny(0.0, perturb=False)
    assert fused_step_applicable(model, opt)
    off = FusedStrandStep(model, cams, opt, bg)
    assert off.head_sdf is None and off.inline_adam_possible()                             # the field alone switches nothing on
    off.views.select(0)
    off.loss()
    assert "head" not in off.terms()
    _, terms, _ = loss_function_single_pass(model, cams[0], opt, bg)
    assert "head" not in terms
    opt.lambda_head = 0.5
    assert fused_step_applicable(model, opt)
    step = FusedStrandStep(model, cams, opt, bg)
    assert step.head_sdf is model.head_sdf and step.head_scratch.E == model._endpoints.shape[0]
    assert not step.inline_adam_possible() and step.enable_inline_adam(True) is False
    step.views.select(0)
    loss, _ = step.loss()
    assert "head" in step.terms() and torch.isfinite(loss) and float(step.terms()["head"]) > 0
    _, terms, _ = loss_function_single_pass(model, cams[0], opt, bg)
    assert "head" in terms
    del model.head_sdf                                                                    # no field on the model: no term
    assert FusedStrandStep(model, cams, opt, bg).head_sdf is None


def test_fused_iteration_with_the_term_matches_op_by_op():
    """tests/test_magnet_gpu.py's comparison with the head term in the magnet's place: 2e-5 on the loss and the terms, 2e-4 of scale on
    every gradient.  lambda_head is set from the op-by-op gradients so that the term's largest endpoint gradient is of the order of
    the rasterizer's."""
    from hgs_runtime import fused as F
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import head_penetration_loss, loss_function_single_pass
    model, cams, _, opt, bg = _tiny(0.0, margin=0.002)
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
    head_penetration_loss(model, model.head_sdf, opt.head_margin).backward()
    g_term = model._endpoints.grad.clone()
    lam = g_raster / float(g_term.abs().max())
    assert np.isfinite(lam) and lam > 0
    clear()
    F.head_penalty(model._endpoints, model.head_sdf, opt.head_margin).backward()
    g_op = model._endpoints.grad.clone()
    clear()
    plain = FusedStrandStep(model, cams, opt, bg)
    plain.views.select(plain.views.index[id(cam)])
    l0, _ = plain.loss()
    plain.backward(l0)
    g_without = model._endpoints.grad.clone()
    opt.lambda_head = lam
    fused = FusedStrandStep(model, cams, opt, bg)
    assert fused.head_sdf is not None
    for ci in (2, 0):
        cam = cams[ci]
        clear()
        loss, terms, _ = loss_function_single_pass(model, cam, opt, bg)
        loss.backward()
        ref = dict(loss=float(loss.detach()), terms={k: float(v.detach()) for k, v in terms.items()}, grads=[p.grad.clone() for p in params])
        assert ref["terms"]["head"] > 0
        clear()
        fused.views.select(fused.views.index[id(cam)])
        floss, _ = fused.loss()
        if ci == 2:
            fused.backward(floss)
        else:
            floss.backward()
        fterms = {k: float(v) for k, v in fused.terms().items()}
        total = float(floss.detach())
        print(f"step | total {total!r} vs {ref['loss']!r} | head {fterms['head']!r} vs {ref['terms']['head']!r}")
        assert abs(total - ref["loss"]) <= 2e-5 * abs(ref["loss"]), (total, ref["loss"])
        for k, v in ref["terms"].items():
            assert abs(fterms[k] - v) <= 2e-5 * max(abs(v), 1e-3), (k, fterms[k], v)
        assert abs(fterms["head"] - ref["terms"]["head"]) <= 2e-5 * abs(ref["terms"]["head"])
        for name, p, gref in zip(("endpoints", "width", "opacity", "mask", "f_dc", "f_rest"), params, ref["grads"]):
            if gref.numel() == 0:
                continue
            scale = float(gref.abs().max())
            assert (p.grad - gref).abs().max() <= 2e-4 * max(scale, 1e-12), (name, float((p.grad - gref).abs().max()), scale)
        if ci == 2:
            # with the term minus without it = lambda_head times the op's own gradient (4 ulp of its scale, times K)
            want = lam * g_op
            err = float((model._endpoints.grad - g_without - want).abs().max())
            assert err <= HR.K * HR.R.ULP4 * float(want.abs().max()), (err, float(want.abs().max()))
            assert float(want.abs().max()) >= 0.5 * g_raster


def test_graphed_step_with_the_term_matches_eager_steps():
    """tests/test_magnet_gpu.py::_graph_vs_eager with the head term on, asserted as that file asserts it."""
    from diff_gaussian_rasterization import _C as raster
    from hgs_runtime.strand_step import FusedStrandStep
    from train import GraphedStep, training_step
    order = [1, 3, 0, 2, 1, 0, 3, 2]
    results = {}
    try:
        for mode in ("eager", "graph", "without"):
            model, cams, extent, opt, bg = _tiny(0.0 if mode == "without" else 20.0, margin=0.002, perturb=False)
            losses = []
            if mode != "graph":
                fused = FusedStrandStep(model, cams, opt, bg)
                assert (fused.head_sdf is not None) == (mode == "eager")
                for it, ci in enumerate(order, 1):
                    loss, terms, _ = training_step(model, cams[ci], opt, bg, it, extent=extent, fused=fused)
                    assert ("head" in terms) == (mode == "eager")
                    losses.append(float(loss))
            else:
                gs = GraphedStep(model, cams, opt, bg, extent=extent, steps_per_graph=1)
                assert gs.fused is not None and gs.fused.head_sdf is not None
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
    """A prune that changes E, then refresh(): the scratch follows, the fused term equals the op-by-op term on the changed model."""
    from hgs_runtime import fused as F
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import head_penetration_loss
    model, cams, _, opt, bg = _tiny(1.0, margin=0.002, perturb=False)
    step = FusedStrandStep(model, cams, opt, bg)
    before = step.head_scratch
    E0 = model._endpoints.shape[0]
    mask = torch.zeros(model.endpoint_pairs.shape[0], dtype=torch.bool, device="cuda")
    mask[7::30] = True                       # segment 7 of every strand: 40 strands become 80
    mask[29] = True                          # and strand 0's last segment: its tip endpoint goes
    model.prune_segments(mask)
    model.compute_strands_info()
    step.refresh()
    E = model._endpoints.shape[0]
    assert E == E0 - 1 and step.head_scratch is not before and step.head_scratch.E == E
    model._endpoints.grad = None
    ref = head_penetration_loss(model, model.head_sdf, opt.head_margin)
    ref.backward()
    g_ref = model._endpoints.grad.clone()
    model._endpoints.grad = None
    step.views.select(1)
    step.loss()
    got = step.terms()["head"]
    assert float(ref) > 0 and abs(float(got) - float(ref)) <= 2e-5 * float(ref)
    F.head_penalty(model._endpoints, model.head_sdf, opt.head_margin, None, step.head_scratch).backward()
    assert (model._endpoints.grad - g_ref).abs().max() <= 2e-4 * float(g_ref.abs().max())
    with pytest.raises(Exception, match="topology event"):
        F.head_penalty(model._endpoints, model.head_sdf, opt.head_margin, None, before)


# ---- through the drivers ---------------------------------------------------------------------------------------------------
def test_head_sdf_and_train_clis(tmp_path, capsys):
    """head_sdf.py on a synthetic scene, a few Stage-III iterations of train.py with --lambda_head: the loss dict has a finite head
    entry, and the report's share of joints inside does not grow."""
    import head_sdf as driver
    import train as train_cli
    from scene.hair_gaussian_model import HairGaussianModel
    from tests.scalp_cases import write_ply
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
    verts, faces = HC.uv_sphere(radius=0.2, centre=(0.0, 0.0, 0.0))                        # a head that some of the strands run through
    write_ply(str(src / "head_mesh.ply"), verts, faces)
    sdf = driver.main(["-s", str(src), "--grid", "33"])
    assert os.path.exists(src / "head_sdf.npz") and (sdf.phi < 0).any()
    before = driver.main(["-s", str(src), "--report", str(model)])
    assert before["joints"] == 240 and before["inside"] > 0
    scene = train_cli.main(["-s", str(src), "-m", str(model), "--iterations", "8", "--save_frequency", "8", "--quiet",
                            "--lambda_head", "50", "--head_margin", "0.01"])
    g = scene.gaussians
    assert isinstance(g, HairGaussianModel) and g.head_sdf.shape == sdf.shape and torch.isfinite(g._endpoints).all()
    after = driver.main(["-s", str(src), "--report", str(model)])
    print(f"report | inside before {before['inside']} ({before['share']:.4f}) | after {after['inside']} ({after['share']:.4f}) |")
    assert os.path.isdir(model / "point_cloud" / "iteration_15") and after["share"] <= before["share"]
    from arguments import OptimizationParams
    opt = OptimizationParams()
    opt.enable_topology = False
    opt.lambda_head, opt.head_margin = 50.0, 0.01
    _, terms, _ = training_step(g, scene.getCameras()[0], opt, torch.zeros(3, device="cuda"), 9, extent=scene.cameras_extent)
    assert "head" in terms and np.isfinite(float(terms["head"]))
