"""The magnet term as a device op (include/hgs.h hgs_magnet_*, hgs_runtime.fused.magnet_loss) and inside the fused, captured
iteration (--fused_magnet): every case of tests/magnet_cases.py under both search paths against hgs_knn3's route (bit for bit),
against float64 (the comparator of tests/magnet_reference.py, K = 8 of the fp32 statement's own error, floor 4 ulp), path
against path and call against call (bit for bit); the fused iteration against the op-by-op one; GraphedStep against eager
steps; and after a topology change."""
import numpy as np
import pytest
import torch

from tests import magnet_cases as MC
from tests import magnet_reference as MR

pytestmark = pytest.mark.gpu

TILES, GRID = 0, 1
_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = MR.reference(MC.cases()[name])
    return _REF[name]


def _run(model, mode):
    """One forward + backward of magnet_loss on a fresh table under a forced search path; everything as numpy."""
    from hgs_runtime import fused as F
    was = F.set_magnet_search(mode)
    try:
        table = F.MagnetTable(model)
        info = {}
        model._endpoints.grad = None
        v = F.magnet_loss(model._endpoints, table, model.min_val, info)
        v.backward()
        torch.cuda.synchronize()
        nv, rows = F.magnet_valid(info), F.magnet_rows(info)
        E = model._endpoints.shape[0]
        grad = model._endpoints.grad.cpu().numpy() if E else np.zeros((0, 3), np.float32)
        return dict(value=np.float32(v.detach().cpu().numpy()), grad=grad, nv=nv, rows=rows, n=table.n,
                    sel=info["sel"].cpu().numpy(), sq=info["sq"].cpu().numpy(), nn_idx=info["nn_idx"].cpu().numpy(),
                    nn_d2=info["nn_d2"].cpu().numpy())
    finally:
        F.set_magnet_search(was)


def _same_bits(a, b):
    for k in ("value", "grad", "sel", "sq", "nn_idx", "nn_d2"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert (a["nv"], a["rows"]) == (b["nv"], b["rows"])


def _knn3_route(model):
    """The op-by-op route on the GPU model: the statement with loss.losses.knn3_self (hgs_knn3) -- its selection, and the
    neighbours / squared distances of the valid ends."""
    from loss.losses import knn3_self
    seen = {}

    def knn(pts):
        d2, idx = knn3_self(pts)
        seen["d2"], seen["idx"] = d2.cpu().numpy(), idx.cpu().numpy()
        return d2, idx
    _, info = MR.torch_statement(model, knn=knn)
    return info, seen


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_case_under_both_search_paths(name):
    ref = _ref(name)
    model = MR.model_of(MC.cases()[name], "cuda")
    got = {mode: _run(model, mode) for mode in (TILES, GRID)}
    again = _run(model, GRID)
    _same_bits(got[TILES], got[GRID])          # the two paths: identical bits in everything
    _same_bits(got[GRID], again)               # two calls: identical bits
    g = got[TILES]
    nv = g["nv"]
    assert g["n"] == len(ref.ends) and nv == ref.r64.nv
    assert (g["sel"][nv:] == -1).all() and (g["nn_idx"][nv:] == -1).all() and np.isinf(g["nn_d2"][nv:]).all()
    if len(ref.ends):
        route, seen = _knn3_route(model)
        assert route.nv == nv and route.rows == g["rows"]
        np.testing.assert_array_equal(g["sel"][:nv, 0], route.sel)
        if nv >= 3:                            # (the statement searches only then)
            np.testing.assert_array_equal(g["nn_idx"][:nv], seen["idx"])
            assert g["nn_d2"][:nv].tobytes() == seen["d2"].astype(np.float32).tobytes()
            kept = g["sel"][:nv, 0] >= 0
            second = g["nn_idx"][:nv, 1] == g["sel"][:nv, 0]
            chosen = np.where(second, g["nn_d2"][:nv, 1], g["nn_d2"][:nv, 2])
            assert g["sq"][:nv][kept].tobytes() == chosen[kept].tobytes() and (g["sq"][:nv][~kept] == 0).all()
        # the index into the list of ends: the valid ends in order
        np.testing.assert_array_equal(g["sel"][:nv, 1], np.nonzero(ref.r64.valid)[0])
    rv, rg = MR.ratios(g["value"], g["grad"], ref)
    print(f"ratio | magnet_loss | {name} | value {rv:.2f} | gradient {rg:.2f} |")
    assert MR.accepts(g["value"], g["grad"], g["sel"][:nv, 0], g["rows"], ref), (rv, rg)


def test_grid_path_at_20000_clustered_ends():
    """The grid at a size near the measured crossover of the two paths: selection and neighbours against hgs_knn3's route, bit
    for bit; the automatic choice at this size gives the same bits (whichever path it is)."""
    model = MR.model_of(MC.big_clustered(), "cuda")
    g = _run(model, GRID)
    route, seen = _knn3_route(model)
    nv = g["nv"]
    assert g["n"] == 20000 and nv == route.nv and g["rows"] == route.rows and nv > 19000
    np.testing.assert_array_equal(g["nn_idx"][:nv], seen["idx"])
    assert g["nn_d2"][:nv].tobytes() == seen["d2"].astype(np.float32).tobytes()
    np.testing.assert_array_equal(g["sel"][:nv, 0], route.sel)
    auto = _run(model, None)
    _same_bits(g, auto)


@pytest.mark.parametrize("n", MC.LEVEL_EDGE_SIZES)
@pytest.mark.parametrize("family", MC.LEVEL_EDGE_FAMILIES)
def test_grid_path_where_its_level_changes(family, n):
    """n ends on both sides of the sizes at which the grid takes its next level (1024: L = 2, 8192: L = 3;
    tests/test_magnet_f64_cpu.py checks that the inputs have n ends, all valid): forced grid against forced tiles bit for bit
    in everything, neighbours and squared distances against hgs_knn3's route bit for bit."""
    model = MR.level_edge_model(MC.level_edge(family, n), n, "cuda")
    g = _run(model, GRID)
    _same_bits(_run(model, TILES), g)
    route, seen = _knn3_route(model)
    nv = g["nv"]
    assert g["n"] == n and nv == route.nv and g["rows"] == route.rows and nv >= n - 1
    np.testing.assert_array_equal(g["nn_idx"][:nv], seen["idx"])
    assert g["nn_d2"][:nv].tobytes() == seen["d2"].astype(np.float32).tobytes()
    np.testing.assert_array_equal(g["sel"][:nv, 0], route.sel)


def _tiny(lambda_magnet, fused_magnet, perturb=True):
    from arguments import OptimizationParams
    from synthetic import build_workload
    from utils.general import safe_state
    safe_state(True)
    model, cams, extent = build_workload("tiny", device="cuda", with_targets=True)
    opt = OptimizationParams()
    opt.enable_topology = False
    opt.lambda_magnet = lambda_magnet
    opt.fused_magnet = fused_magnet
    model.training_setup(opt)
    if perturb:      # off the point the synthetic targets were rendered at (tests/test_gpu_train.py: the L1 term's sign)
        g = torch.Generator(device="cuda").manual_seed(5)
        with torch.no_grad():
            model._features_dc.add_(0.2 * torch.randn(model._features_dc.shape, device="cuda", generator=g))
            model._endpoints.add_(0.003 * torch.randn(model._endpoints.shape, device="cuda", generator=g))
            model._opacity.add_(0.3 * torch.randn(model._opacity.shape, device="cuda", generator=g))
            model._mask.add_(0.3 * torch.randn(model._mask.shape, device="cuda", generator=g))
    return model, cams, extent, opt, torch.zeros(3, device="cuda")


def test_switch_and_step_surface():
    from hgs_runtime.strand_step import FusedStrandStep
    from train import fused_step_applicable
    model, cams, _, opt, bg = _tiny(0.1, False, perturb=False)
    assert not fused_step_applicable(model, opt)
    opt.fused_magnet = True
    assert fused_step_applicable(model, opt)
    step = FusedStrandStep(model, cams, opt, bg)
    assert step.magnet is not None and step.magnet.n == 80 and not step.inline_adam_possible()
    assert step.enable_inline_adam(True) is False
    step.views.select(0)
    loss, _ = step.loss()
    assert "magnet" in step.terms() and torch.isfinite(loss)
    opt.lambda_magnet = 0.0
    off = FusedStrandStep(model, cams, opt, bg)
    assert fused_step_applicable(model, opt) and off.magnet is None and off.inline_adam_possible()
    assert getattr(model, "_magnet_table_cache", None) is step.magnet      # (remembered on the model, not rebuilt)
    off.views.select(0)
    off.loss()
    assert "magnet" not in off.terms()


def test_fused_iteration_with_the_term_matches_op_by_op():
    """tests/test_gpu_train.py::test_fused_iteration_matches_op_by_op_path with the magnet term on: 2e-5 on the loss and the
    terms, 2e-4 of scale on every gradient.  lambda_magnet is set from the op-by-op gradients so that the term's largest
    endpoint gradient is of the order of the rasterizer's (at 0.1 it would hide under the bar)."""
    from hgs_runtime import fused as F
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import loss_function_single_pass, strand_joints_magnet_loss
    model, cams, _, opt, bg = _tiny(0.0, True)
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
    strand_joints_magnet_loss(model).backward()
    g_term = model._endpoints.grad.clone()
    lam = g_raster / float(g_term.abs().max())
    assert np.isfinite(lam) and lam > 0
    # the op's own gradient, and the fused iteration without the term
    clear()
    F.magnet_loss(model._endpoints, F.MagnetTable.of(model), model.min_val).backward()
    g_op = model._endpoints.grad.clone()
    clear()
    plain = FusedStrandStep(model, cams, opt, bg)
    plain.views.select(plain.views.index[id(cam)])
    l0, _ = plain.loss()
    plain.backward(l0)
    g_without = model._endpoints.grad.clone()
    opt.lambda_magnet = lam
    fused = FusedStrandStep(model, cams, opt, bg)
    assert fused.magnet is not None
    for ci in (2, 0):
        cam = cams[ci]
        clear()
        loss, terms, _ = loss_function_single_pass(model, cam, opt, bg)
        loss.backward()
        ref = dict(loss=float(loss), terms={k: float(v) for k, v in terms.items()}, grads=[p.grad.clone() for p in params])
        assert "magnet" in ref["terms"]
        clear()
        fused.views.select(fused.views.index[id(cam)])
        floss, _ = fused.loss()
        if ci == 2:
            fused.backward(floss)
        else:
            floss.backward()
        fterms = {k: float(v) for k, v in fused.terms().items()}
        assert abs(float(floss) - ref["loss"]) <= 2e-5 * abs(ref["loss"]), (float(floss), ref["loss"])
        for k, v in ref["terms"].items():
            assert abs(fterms[k] - v) <= 2e-5 * max(abs(v), 1e-3), (k, fterms[k], v)
        assert abs(fterms["magnet"] - ref["terms"]["magnet"]) <= 2e-5 * abs(ref["terms"]["magnet"])
        for name, p, gref in zip(("endpoints", "width", "opacity", "mask", "f_dc", "f_rest"), params, ref["grads"]):
            if gref.numel() == 0:
                continue
            scale = float(gref.abs().max())
            assert (p.grad - gref).abs().max() <= 2e-4 * max(scale, 1e-12), (name, float((p.grad - gref).abs().max()), scale)
        if ci == 2:
            # with the term minus without it = lambda_magnet times the op's own gradient (4 ulp of its scale, times K)
            want = lam * g_op
            err = float((model._endpoints.grad - g_without - want).abs().max())
            assert err <= MR.K * MR.R.ULP4 * float(want.abs().max()), (err, float(want.abs().max()))
            assert float(want.abs().max()) >= 0.5 * g_raster


def _graph_vs_eager(steps_per_graph):
    from diff_gaussian_rasterization import _C as raster
    from hgs_runtime.strand_step import FusedStrandStep
    from train import GraphedStep, training_step
    order = [1, 3, 0, 2, 1, 0, 3, 2]
    results = {}
    try:
        for mode in ("eager", "graph"):
            model, cams, extent, opt, bg = _tiny(50.0, True, perturb=False)
            losses = []
            if mode == "eager":
                fused = FusedStrandStep(model, cams, opt, bg)
                assert fused.magnet is not None
                for it, ci in enumerate(order, 1):
                    loss, terms, _ = training_step(model, cams[ci], opt, bg, it, extent=extent, fused=fused)
                    assert "magnet" in terms
                    losses.append(float(loss))
            else:
                gs = GraphedStep(model, cams, opt, bg, extent=extent, steps_per_graph=steps_per_graph)
                assert gs.fused is not None and gs.fused.magnet is not None
                gs.capture(cams)
                assert not gs.inline_adam
                if steps_per_graph == 1:
                    for it, ci in enumerate(order, 1):
                        losses.append(float(gs.step(cams[ci], it)))
                else:
                    for s in range(0, len(order), steps_per_graph):
                        losses += [float(l) for l in gs.step_many([cams[ci] for ci in order[s:s + steps_per_graph]], s + 1)]
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
    return results


def test_graphed_step_with_the_term_matches_eager_steps():
    """tests/test_gpu_train.py::test_graphed_step_matches_eager_steps with the term and the flag on (same bars)."""
    res = _graph_vs_eager(1)
    # the term did move the ends: against a run without it the endpoints differ
    model, cams, extent, opt, bg = _tiny(0.0, True, perturb=False)
    from hgs_runtime.strand_step import FusedStrandStep
    from train import training_step
    fused = FusedStrandStep(model, cams, opt, bg)
    for it, ci in enumerate([1, 3, 0, 2, 1, 0, 3, 2], 1):
        training_step(model, cams[ci], opt, bg, it, extent=extent, fused=fused)
    assert (model._endpoints.detach() - res["eager"][1]).abs().max() > 0


def test_eight_steps_per_graph_with_the_term_match_eager_steps():
    _graph_vs_eager(8)


def test_several_steps_per_graph_with_the_term_equal_single_step_replays():
    """tests/test_gpu_train.py::test_several_steps_per_graph_equal_single_step_replays with the term on: bit for bit."""
    from diff_gaussian_rasterization import _C as raster
    from train import GraphedStep
    order = [1, 3, 0, 2, 1, 0, 3, 2]
    results = {}
    try:
        for mode in ("single", "many"):
            model, cams, extent, opt, bg = _tiny(50.0, True, perturb=False)
            gs = GraphedStep(model, cams, opt, bg, extent=extent, steps_per_graph=8 if mode == "many" else 1)
            gs.capture(cams)
            if mode == "single":
                losses = [gs.step(cams[ci], it).clone() for it, ci in enumerate(order, 1)]
            else:
                losses = [l.clone() for l in gs.step_many([cams[ci] for ci in order], 1)]
            assert min(gs.check()) > 0
            raster.set_async(False)
            results[mode] = (torch.stack(losses), model._endpoints.detach().clone(), model._opacity.detach().clone(),
                             model._features_dc.detach().clone(), model.denom.clone(), model.xyz_gradient_accum.clone())
    finally:
        raster.set_async(False)
    for a, b in zip(results["single"], results["many"]):
        assert torch.equal(a, b)


def test_term_follows_a_topology_change():
    """A prune that cuts every strand in two (new ends, endpoint ids renumbered), then refresh(): the fused term equals the
    op-by-op term on the changed model; a stale table would show here."""
    from hgs_runtime import fused as F
    from hgs_runtime.strand_step import FusedStrandStep
    from loss.losses import strand_joints_magnet_loss
    model, cams, _, opt, bg = _tiny(1.0, True, perturb=False)
    step = FusedStrandStep(model, cams, opt, bg)
    before = step.magnet
    assert before.n == 80
    mask = torch.zeros(model.endpoint_pairs.shape[0], dtype=torch.bool, device="cuda")
    mask[7::30] = True                       # segment 7 of every strand: 40 strands become 80
    mask[29] = True                          # and strand 0's last segment: its tip endpoint goes, the ids behind it shift
    model.prune_segments(mask)
    model.compute_strands_info()             # (as every topology operator ends: refresh() reads the strand tables)
    step.refresh()
    assert step.magnet is not before and step.magnet.n == 160 and step.magnet.E == model._endpoints.shape[0] == before.E - 1
    u, c = torch.unique(model.endpoint_pairs, return_counts=True)
    assert torch.equal(step.magnet.ends.long(), u[c == 1])
    model._endpoints.grad = None
    ref = strand_joints_magnet_loss(model)
    ref.backward()
    g_ref = model._endpoints.grad.clone()
    model._endpoints.grad = None
    step.views.select(1)
    step.loss()
    got = step.terms()["magnet"]
    assert float(ref) > 0 and abs(float(got) - float(ref)) <= 2e-5 * float(ref)
    F.magnet_loss(model._endpoints, step.magnet, model.min_val).backward()
    assert (model._endpoints.grad - g_ref).abs().max() <= 2e-4 * float(g_ref.abs().max())
    # a new step object after the event finds the same table again
    assert FusedStrandStep(model, cams, opt, bg).magnet is step.magnet
    # and the stale table is refused, not read out of bounds
    with pytest.raises(Exception, match="topology event"):
        F.magnet_loss(model._endpoints, before, model.min_val)


def test_training_loop_with_the_term_and_without_the_flag_runs_eagerly():
    """training() with lambda_magnet > 0 and no --fused_magnet: the op-by-op term synchronises with the host, which a graph
    capture refuses, so the loop launches every iteration eagerly; with the flag the same call replays captured graphs."""
    from diff_gaussian_rasterization import _C as raster
    from train import training
    try:
        for flag in (False, True):
            model, cams, extent, opt, _ = _tiny(0.1, flag, perturb=False)
            before = model._endpoints.detach().clone()
            training(model, cams, opt, iterations=3, extent=extent, use_graph=True)
            assert torch.isfinite(model._endpoints).all() and (model._endpoints.detach() - before).abs().max() > 0
    finally:
        raster.set_async(False)
