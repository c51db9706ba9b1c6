"""The endpoint gather folded into the preprocess backward by strand blocks (include/hgs.h HgsBlockPlan,
hgs_backward_multi_params_planned; csrc/hgs_preprocess.hip preprocess_bwd_kernel<., 1, true>): workgroups that own whole
strands sum and update their endpoints behind one barrier, and strand_gather_kernel's launch is gone.  Against the two
launches (hgs_backward_multi_params + hgs_hair_endpoint_gather) bit for bit -- where no wavefront streams its rows, or
row_reduce_kernel sums them; to the rounding of those sums where one does (the last test) -- on a model of strands of 1, 2, 63, 64, 65, 127,
128 and 255 segments (705 segments, 705 % 64 = 1: every workgroup has dead lanes, the chunks hold 195, 127, 128 and 255
segments) at 160 x 96; and dL_dsh of the chunks' last segments against the CPU oracle (a dead lane used to clear it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = (1, 2, 63, 64, 65, 127, 128, 255)
W, H = 160, 96


def _build(lens=LENS, n_seg=255, views=3):
    """The model (deterministic: two calls give the same bits), its cameras with targets, extent, options."""
    from arguments import OptimizationParams
    from scene.hair_gaussian_model import HairGaussianModel
    from synthetic import attach_targets, cameras_extent, make_cameras, strand_polylines
    cams = make_cameras(views, W, H, device="cuda")
    extent = cameras_extent(cams)
    pts = strand_polylines(len(lens), n_seg, seed=0, step=0.0006)
    rng = np.random.default_rng(1)
    P0 = len(lens) * n_seg
    model = HairGaussianModel.from_strands(pts, width=3e-4, opacity=rng.uniform(0.3, 0.95, (P0, 1)).astype(np.float32),
                                           colors=rng.uniform(0.2, 0.9, (P0, 3)).astype(np.float32), spatial_lr_scale=extent,
                                           device="cuda")
    opt = OptimizationParams()
    opt.enable_topology = False
    model.training_setup(opt)
    k = torch.arange(P0, device="cuda")
    drop = (k % n_seg) >= torch.tensor(lens, device="cuda")[k // n_seg]
    if bool(drop.any()):
        model.prune_segments(drop)          # the model's own operator: strands of the lengths above, ids compacted
    model.training_setup(opt)
    model.compute_strands_info(only_foreground=True)
    attach_targets(cams, model)
    return model, cams, extent, opt


def _state(model):
    out = []
    for g_ in model.optimizer.param_groups:
        for p in g_["params"]:
            st = model.optimizer.state.get(p, {})
            out += [p.detach().clone()] + [st[k].clone() for k in ("exp_avg", "exp_avg_sq", "step") if k in st]
    return out + [model.max_radii2D.clone(), model.xyz_gradient_accum.clone(), model.denom.clone()]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)


@pytest.fixture
def gather_calls(monkeypatch):
    """Counts the launches of hgs_hair_endpoint_gather: the planned form has none, the two-launch form one per backward."""
    import hgs_runtime as rt
    L = rt.lib()
    orig, calls = L.hgs_hair_endpoint_gather, []

    def counted(*a):
        calls.append(1)
        return orig(*a)
    monkeypatch.setattr(L, "hgs_hair_endpoint_gather", counted)
    return calls


def test_planned_backward_equals_the_two_launches(gather_calls):
    """Gradients (d_endpoints, d_width, d_opacity_raw, d_mask_raw, dL_dsh), the RGB-only screen-space gradient, the
    densification statistics and the loss terms, with and without the smoothness term and the deferred head tail; the planned
    step run twice gives the same bits twice."""
    from hgs_runtime.strand_step import FusedStrandStep, ViewTable
    model, cams, _, _ = _build()
    from arguments import OptimizationParams
    params = [model._endpoints, model._width, model._opacity, model._mask, model._features_dc]
    stats = lambda: [model.max_radii2D, model.xyz_gradient_accum, model.denom]
    for lam_smooth, defer in ((None, False), (None, True), (0.0, False)):
        opt = OptimizationParams()
        if lam_smooth is not None:
            opt.lambda_smooth = lam_smooth
        model.training_setup(opt)
        runs = []
        for fuse in (False, True, True):
            for t in stats():
                t.zero_()
            views = ViewTable(cams)
            step = FusedStrandStep(model, views, opt, torch.zeros(3, device="cuda"))
            step.fuse_endpoint_gather = fuse
            step.defer_tail = defer
            assert step.block_plan is not None and step.block_plan[0][:, 1].tolist() == [195, 127, 128, 255]
            assert (step.ep_pairs is not None) == (lam_smooth is None)      # (the default weight of the smoothness term is not 0)
            del gather_calls[:]
            seen = []
            for v in (0, 2, 1):
                for p in params:
                    p.grad = None
                views.prologue(v, ride=True)
                loss, terms = step.loss()
                step.backward(loss)
                assert step.last["stats_done"]
                seen.append([loss.detach().clone(), terms[:14].clone(), step.last["dmean2D"].clone()] +
                            [p.grad.clone() for p in params] + [t.clone() for t in stats()])
                # every strand is in view: each has a visible segment
                vis = (step.last["radii"] > 0).cpu()
                first = np.concatenate(([0], np.cumsum(LENS)))
                assert all(bool(vis[a:b].any()) for a, b in zip(first[:-1], first[1:]))
            assert len(gather_calls) == (0 if fuse else 3)
            runs.append(seen)
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                _same(a, b)
        for a in runs[0]:
            assert all(bool(t.abs().sum() > 0) for t in a[3:8]) and bool(a[-1].sum() > 0)


def test_planned_backward_with_adam_in_its_lanes_and_after_a_topology_event(gather_calls):
    """Three steps with the Adam update in the backward's lanes -- the endpoints' in the endpoint phase of the planned launch --:
    parameters, both moments, step counters and statistics as with the gather launch; then one topology event of the model's own
    operators, refresh() rebuilds the plan, and two more steps compare the same way."""
    from hgs_runtime.strand_step import ViewTable, fused_step_for
    from train import training_step
    bg = torch.zeros(3, device="cuda")
    runs = {}
    for fuse in (False, True):
        model, cams, extent, opt = _build()
        fused = fused_step_for(model, ViewTable(cams), opt, bg)
        fused.fuse_endpoint_gather = fuse
        assert fused.block_plan is not None and fused.enable_inline_adam(True)
        del gather_calls[:]
        for it, v in enumerate((0, 2, 1), start=1):
            training_step(model, cams[v], opt, bg, it, extent=extent, fused=fused)
        assert len(gather_calls) == (0 if fuse else 3)
        snap = _state(model)
        # the event: the tip of the 255-segment strand and the whole 2-segment strand go
        P = model.endpoint_pairs.shape[0]
        drop = torch.zeros(P, dtype=torch.bool, device="cuda")
        drop[P - 7:] = True
        drop[1:3] = True
        model.prune_segments(drop)
        model.compute_strands_info(only_foreground=True)     # (as the operators do: the strand tables name the new endpoint ids)
        fused.refresh()
        assert fused.block_plan is not None and int(fused.block_plan[0][:, 1].sum()) == P - 9
        assert fused.block_plan[0][:, 1].tolist() == [193, 127, 128, 248]      # (1 + 63 + 64 + 65; 127 + 128 have 257 endpoints)
        assert fused.enable_inline_adam(True)
        del gather_calls[:]
        for it, v in enumerate((1, 0), start=4):
            training_step(model, cams[v], opt, bg, it, extent=extent, fused=fused)
        assert len(gather_calls) == (0 if fuse else 2)
        torch.cuda.synchronize()
        runs[fuse] = (snap, _state(model))
    for a, b in zip(runs[False], runs[True]):
        _same(a, b)
    steps = sorted(float(t) for t in runs[True][1] if t.ndim == 0)
    assert steps and steps[-1] == 5.0 and set(steps) <= {0.0, 5.0}


@pytest.mark.parametrize("smooth", [False, True])
def test_planned_backward_on_a_pass_voided_by_a_capacity_overflow(gather_calls, smooth):
    """A forward that overflowed its binning capacity voids the pass: every gradient the rasterizer feeds is exactly zero -- with
    the smoothness term the endpoints keep that term's gradient alone, which does not come from the pass -- and the in-lane Adam
    update still decays the moments: the same bits in both forms."""
    from diff_gaussian_rasterization import _C as raster
    from hgs_runtime.strand_step import ViewTable, fused_step_for
    from train import training_step
    bg = torch.zeros(3, device="cuda")
    runs = {}
    try:
        for fuse in (False, True):
            raster.set_async(False)
            model, cams, extent, opt = _build()
            if not smooth:
                opt.lambda_smooth = 0.0
            raster.set_async(True)
            raster.reset_capacity(0)
            fused = fused_step_for(model, ViewTable(cams), opt, bg)
            fused.fuse_endpoint_gather = fuse
            assert fused.block_plan is not None and fused.enable_inline_adam(True)
            training_step(model, cams[0], opt, bg, 1, extent=extent, fused=fused)     # (moments that can decay)
            ep_state = lambda: [model.optimizer.state[model._endpoints][k].clone() for k in ("exp_avg", "step")]
            before, ep_before = _state(model), ep_state()
            raster.reset_capacity(64)
            model.optimizer.zero_grad(set_to_none=True)
            fused.views.prologue(1, ride=True)
            loss, _ = fused.loss()
            fused.backward(loss)
            with pytest.raises(raster.HgsCapacityOverflow):
                raster.check_async()
            grads = [p.grad.clone() for p in (model._endpoints, model._width, model._opacity, model._mask, model._features_dc)]
            assert all(bool((g_ == 0).all()) for g_ in grads[1:]) and bool((grads[0] == 0).all()) == (not smooth)
            model.optimizer.step()
            torch.cuda.synchronize()
            runs[fuse] = (before, _state(model), grads)
            ep_after = ep_state()
            assert not torch.equal(ep_before[0], ep_after[0]) and float(ep_after[1]) == 2.0   # the first moment decayed; step 2
        assert len(gather_calls) == 2          # (the two-launch run's two backwards)
    finally:
        raster.set_async(False)
        raster.reset_capacity(0)
    for a, b in zip(runs[False], runs[True]):
        _same(a, b)


def test_a_model_without_a_plan_keeps_its_two_launches(gather_calls):
    """Strands of 300 segments fit no chunk: the plan is None, the gather stays a launch of its own, and the gradients are those
    of the unfused parameter backward (hgs_backward + hgs_hair_params_backward) bit for bit, as before."""
    from hgs_runtime.strand_step import FusedStrandStep, ViewTable
    model, cams, _, opt = _build(lens=(300, 300, 300), n_seg=300)
    params = [model._endpoints, model._width, model._opacity, model._mask, model._features_dc]
    runs = {}
    for fuse in (False, True):
        for t in (model.max_radii2D, model.xyz_gradient_accum, model.denom):
            t.zero_()
        views = ViewTable(cams)
        step = FusedStrandStep(model, views, opt, torch.zeros(3, device="cuda"))
        step.fuse_param_backward = fuse
        assert step.block_plan is None and step.ep_segments is not None and step.fuse_endpoint_gather
        del gather_calls[:]
        seen = []
        for v in (0, 1):
            for p in params:
                p.grad = None
            views.prologue(v, ride=True)
            loss, terms = step.loss()
            step.backward(loss)
            seen.append([loss.detach().clone(), terms[:14].clone()] + [p.grad.clone() for p in params] +
                        [model.max_radii2D.clone(), model.xyz_gradient_accum.clone(), model.denom.clone()])
        assert len(gather_calls) == (2 if fuse else 0)
        runs[fuse] = seen
    for a, b in zip(runs[False], runs[True]):
        _same(a, b)
        assert bool(a[2].abs().sum() > 0)


def test_a_bad_plan_is_refused():
    """Sizes, pointers and alignment of a plan are checked on the host: an error, never a silent two-launch pass."""
    import ctypes as C
    import hgs_runtime as rt
    L = rt.lib()
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, dtype=torch.float32, device="cuda")

    def plan(**kw):
        bp = rt.BlockPlan()
        bp.n_chunks, bp.chunks, bp.ep_list, bp.n_segments, bp.n_endpoints = 1, buf.data_ptr(), buf.data_ptr(), 4, 5
        bp.ep_segments, bp.d_endpoints = buf.data_ptr(), out.data_ptr()
        for k, v in kw.items():
            setattr(bp, k, v)
        return bp
    pb = rt.ParamBackward()
    pb.kind = rt.PARAMS_HAIR

    def call(bp, P=4):
        return L.hgs_backward_multi_params_planned(None, P, 0, 1, 0, 16, 16, 0, *([None] * 8), 1.0, 1.0, *([None] * 7), C.byref(pb),
                                                   C.byref(bp))
    for bad in (dict(n_chunks=0), dict(n_segments=3), dict(chunks=buf.data_ptr() + 4), dict(ep_list=None), dict(d_endpoints=None),
                dict(ep_segments=buf.data_ptr() + 4), dict(ep_pairs=buf.data_ptr() + 8, n_smooth=2),
                dict(ep_pairs=buf.data_ptr(), n_smooth=2, head_out=out.data_ptr(), grad_out=out.data_ptr()),     # no pair gradients
                dict(n_chunks=5)):
        assert call(plan(**bad)) != 0, bad
        assert b"hgs_backward_multi_params_planned" in L.hgs_last_error()
    pb.kind = rt.PARAMS_CLOUD
    assert call(plan()) != 0 and b"HGS_PARAMS_HAIR" in L.hgs_last_error()


def test_last_segment_of_a_chunk_keeps_its_sh_gradient():
    """P % 64 != 0 and the chunks' last segments visible: dL_dsh of the planned launch against the CPU oracle's backward at the
    bars tests/test_gpu_raster.py holds dL_dsh to (_grad_check7).  Dead lanes share their index with a live lane of their
    workgroup and cleared its dL_dsh when it was invisible to them; with a plan that would be a segment of every chunk.  The
    oracle is the reference: the two-launch form shared the defect (lanes past P cleared dL_dsh[P - 1])."""
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    from hgs_runtime.strand_step import _adjacency, _block_plan
    from tests import gpu_util as G
    from tests.test_gpu_raster import _forward7, _grad_check7, _oracle_backward7, _oracle_three_passes, _scene_of
    model, cams, _, _ = _build()
    P, E = model.endpoint_pairs.shape[0], model._endpoints.shape[0]
    assert P == 705 and P % 64 == 1
    pairs = model.endpoint_pairs.contiguous()
    adj = _adjacency(pairs.reshape(-1), 2, E, 2)
    chunks, ep_list = _block_plan(adj, P)
    last = (chunks[:, 0] + chunks[:, 1] - 1).tolist()
    assert last == [194, 321, 449, 704]
    d = G.to_dev
    f32 = dict(dtype=torch.float32, device="cuda")
    bg7 = np.zeros(7, np.float32)
    checked = 0
    for cam in cams:
        s = _scene_of(model, cam)
        with torch.no_grad():
            extra = torch.cat((model.get_mask, model.get_orientation), dim=1).contiguous()
        fw = _forward7(s, extra, bg7, True)
        vis = (fw["radii"] > 0).cpu().numpy()
        if not vis[last].all():
            continue
        refs = _oracle_three_passes(s, extra.cpu().numpy(), bg7)
        fw_ref_lists = _forward7(s, extra, bg7, False)
        dplanes = np.random.default_rng(23).normal(size=(7, s["H"], s["W"])).astype(np.float32)
        gref = _oracle_backward7(refs, fw_ref_lists, dplanes)
        dp = d(dplanes)
        pb, bp = rt.ParamBackward(), rt.BlockPlan()
        g_means2D, d_ep = torch.empty((P, 3), **f32), torch.empty((E, 3), **f32)
        d_w, d_o, d_m = torch.empty((P, 1), **f32), torch.empty((P, 1), **f32), torch.empty((P, 1), **f32)
        endpoints = model._endpoints.detach()
        pb.kind, pb.endpoints, pb.endpoint_pairs = rt.PARAMS_HAIR, rt.ptr(endpoints), rt.ptr(pairs)
        pb.dist_to_scale_factor = float(model.dist_to_scale_factor)
        pb.extra4, pb.d_width, pb.d_opacity_raw, pb.d_mask_raw = rt.ptr(extra), rt.ptr(d_w), rt.ptr(d_o), rt.ptr(d_m)
        pb.dL_dmeans2D_rgb = rt.ptr(g_means2D)
        bp.n_chunks, bp.chunks, bp.ep_list = int(chunks.shape[0]), chunks.data_ptr(), ep_list.data_ptr()
        bp.n_segments, bp.n_endpoints, bp.ep_segments, bp.d_endpoints = P, E, adj.data_ptr(), rt.ptr(d_ep)
        g_sh = _C.rasterize_gaussians_multi_backward_params(
            None, d(s["means3D"]), fw["radii"], d(s["scales"]), d(s["rotations"]), d(s["viewmatrix"]), d(s["projmatrix"]),
            float(s["tanfovx"]), float(s["tanfovy"]), [dp[k] for k in range(7)], d(s["shs"]), int(s["sh_degree"]), d(s["campos"]),
            fw["geom"], fw["R"], fw["binning"], fw["img"], pb, plan=bp)
        torch.cuda.synchronize()
        got = g_sh.cpu().numpy()
        report = _grad_check7({"dL_dsh": got}, gref, refs[0][1])
        print("CHUNK_LAST_DSH", cam.image_name, report["dL_dsh"], np.abs(got[last]).max(axis=(1, 2)),
              np.abs(gref["dL_dsh"][last]).max(axis=(1, 2)))
        # the rows the defect cleared: graded by the blend (a nonzero reference), hence nonzero here
        assert (np.abs(gref["dL_dsh"][last]).reshape(len(last), -1).max(axis=1) > 0).all()
        assert (np.abs(got[last]).reshape(len(last), -1).max(axis=1) > 0).all()
        checked += 1
    assert checked >= 1, "no view shows the last segment of every chunk"


def _parameter_backward(model, s, extra, fw, dplanes, adj, tables):
    """One backward of the pass `fw` through the C ABI: with `tables` (chunks, ep_list) the planned launch, else
    hgs_backward_multi_params + hgs_hair_endpoint_gather.  Returns the gradients as numpy arrays by name."""
    import ctypes as C
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    d = G.to_dev
    f32 = dict(dtype=torch.float32, device="cuda")
    P, E = model.endpoint_pairs.shape[0], model._endpoints.shape[0]
    pairs, endpoints = model.endpoint_pairs.contiguous(), model._endpoints.detach()
    dp = d(dplanes)
    pb = rt.ParamBackward()
    g_means2D, d_ep, seg_contrib = torch.empty((P, 3), **f32), torch.empty((E, 3), **f32), torch.empty((P, 2, 4), **f32)
    d_w, d_o, d_m = torch.empty((P, 1), **f32), torch.empty((P, 1), **f32), torch.empty((P, 1), **f32)
    pb.kind, pb.endpoints, pb.endpoint_pairs = rt.PARAMS_HAIR, rt.ptr(endpoints), rt.ptr(pairs)
    pb.dist_to_scale_factor = float(model.dist_to_scale_factor)
    pb.extra4, pb.d_width, pb.d_opacity_raw, pb.d_mask_raw = rt.ptr(extra), rt.ptr(d_w), rt.ptr(d_o), rt.ptr(d_m)
    pb.dL_dmeans2D_rgb = rt.ptr(g_means2D)
    bp = None
    if tables is not None:
        bp = rt.BlockPlan()
        bp.n_chunks, bp.chunks, bp.ep_list = int(tables[0].shape[0]), tables[0].data_ptr(), tables[1].data_ptr()
        bp.n_segments, bp.n_endpoints, bp.ep_segments, bp.d_endpoints = P, E, adj.data_ptr(), rt.ptr(d_ep)
    else:
        pb.seg_contrib = rt.ptr(seg_contrib)
    g_sh = _C.rasterize_gaussians_multi_backward_params(
        None, d(s["means3D"]), fw["radii"], d(s["scales"]), d(s["rotations"]), d(s["viewmatrix"]), d(s["projmatrix"]),
        float(s["tanfovx"]), float(s["tanfovy"]), [dp[k] for k in range(7)], d(s["shs"]), int(s["sh_degree"]), d(s["campos"]),
        fw["geom"], fw["R"], fw["binning"], fw["img"], pb, plan=bp)
    if tables is None:
        fu = rt.StrandFusion()
        fu.ep_segments, fu.n_endpoints = adj.data_ptr(), E
        rt.check(rt.lib().hgs_hair_endpoint_gather(rt.current_stream(), E, rt.ptr(seg_contrib), rt.ptr(endpoints), rt.ptr(d_ep),
                                                   C.byref(fu), None))
    torch.cuda.synchronize()
    return dict(endpoints=d_ep.cpu().numpy(), width=d_w.cpu().numpy(), opacity_raw=d_o.cpu().numpy(), mask_raw=d_m.cpu().numpy(),
                dL_dsh=g_sh.cpu().numpy(), dL_dmeans2D_rgb=g_means2D.cpu().numpy())


def test_planned_wavefronts_with_dead_lanes_that_stream_their_rows():
    """Four segments of the model made thick enough to cover more than HGS_PPB_LIGHT_MAX = 32 tiles: their wavefronts stream
    their rows (hgs_stream_rows) -- in the planned mapping wavefronts WITH DEAD LANES among them (lane 194 of chunk 0: 3 live
    lanes of 64; lane 126 of chunk 1: 63 of 64; the last lane of chunk 3), which take part with zero rows.  A streamed sum's
    association depends on where the Gaussian's rows fall in its wavefront's run, i.e. on which 64 segments form the wavefront,
    and the two forms group the segments differently: there they hold the same terms in another order.  So
      * with the rows summed by row_reduce_kernel (HGS_ROWS_REDUCE), which knows no wavefronts of Gaussians, both forms are
        the same bits;
      * with the rows summed in the launch (HGS_ROWS_INLINE) each form meets the oracle at the bars of tests/test_gpu_raster.py
        (_grad_check7; the parameters' gradients at GRAD_MAX_OF_SCALE, against the oracle's gradients pushed through the model's
        getters), is bitwise reproducible, and the forms lie within twice that bar of each other: two results within 1e-4 of the
        scale of one reference.  (dL_dpix is zero on the oracle's near-threshold pixels, so no decision taken the other way
        enters.)"""
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    from hgs_runtime.strand_step import _adjacency, _block_plan
    from tests import gpu_util as G
    from tests.test_gpu_raster import (GRAD_MAX_OF_SCALE, _chain_rule_reference, _forward7, _fragile_pixels7, _grad_check7,
                                       _oracle_backward7, _oracle_three_passes, _scene_of)
    model, cams, _, _ = _build()
    thick = [100, 194, 321, 704]
    with torch.no_grad():
        model._width[thick] = float(np.log(0.25))
    P, E = model.endpoint_pairs.shape[0], model._endpoints.shape[0]
    adj = _adjacency(model.endpoint_pairs.reshape(-1), 2, E, 2)
    tables = _block_plan(adj, P)
    chunks = tables[0].cpu().numpy()
    cam = cams[0]
    s = _scene_of(model, cam)
    with torch.no_grad():
        extra = torch.cat((model.get_mask, model.get_orientation), dim=1).contiguous()
    bg7 = np.zeros(7, np.float32)
    fw = _forward7(s, extra, bg7, True)
    rows = G._view(fw["geom"], rt.layout("geom", P)["tiles_touched"], P, np.uint32).astype(np.int64)
    rows = np.where(fw["radii"].cpu().numpy() > 0, rows, 0)
    assert (rows[thick] > 32).all(), rows[thick]
    # wavefronts that stream, by mapping: the planned one has such wavefronts with dead lanes, and the sets differ
    planned_waves = [(s0 + 64 * w, min(s0 + 64 * w + 64, s0 + ns)) for s0, ns, _, _ in chunks for w in range((ns + 63) // 64)]
    plain_waves = [(a, min(a + 64, P)) for a in range(0, P, 64)]
    heavy = lambda waves: [(a, b) for a, b in waves if rows[a:b].max() > 32]
    assert any(b - a < 64 for a, b in heavy(planned_waves)) and heavy(planned_waves) != heavy(plain_waves)
    refs = _oracle_three_passes(s, extra.cpu().numpy(), bg7)
    fw_ref_lists = _forward7(s, extra, bg7, False)
    dplanes = np.random.default_rng(23).normal(size=(7, s["H"], s["W"])).astype(np.float32)
    dplanes = dplanes * ~_fragile_pixels7(refs, fw_ref_lists)
    gref = _oracle_backward7(refs, fw_ref_lists, dplanes)
    names = ["endpoints", "width", "opacity_raw", "mask_raw"]
    want = dict(zip(names, _chain_rule_reference(model, "hair", gref)))
    was = _C.set_row_reduce(True)
    try:
        a, b = _parameter_backward(model, s, extra, fw, dplanes, adj, None), _parameter_backward(model, s, extra, fw, dplanes, adj, tables)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        _C.set_row_reduce(False)
        two = _parameter_backward(model, s, extra, fw, dplanes, adj, None)
        planned = _parameter_backward(model, s, extra, fw, dplanes, adj, tables)
        again = _parameter_backward(model, s, extra, fw, dplanes, adj, tables)
    finally:
        _C.set_row_reduce(was)
    for k in planned:
        assert np.array_equal(planned[k], again[k]), k
    for form, got in (("two launches", two), ("planned", planned)):
        _grad_check7({k: got[k] for k in ("dL_dsh", "dL_dmeans2D_rgb")}, gref, refs[0][1])
        for k in names:
            ref = want[k].astype(np.float64).reshape(want[k].shape[0], -1)
            err = np.abs(got[k].astype(np.float64).reshape(ref.shape) - ref)
            scale = float(np.abs(ref).max())
            print("STREAMED_ROWS", form, k, "max error / scale", float(err.max()) / scale)
            assert scale > 0 and float(err.max()) <= GRAD_MAX_OF_SCALE * scale, (form, k)
    differ = 0
    for k in planned:
        ref = (want[k] if k in want else gref[k]).astype(np.float64)
        scale = float(np.abs(ref).max())
        diff = float(np.abs(planned[k].astype(np.float64) - two[k].astype(np.float64)).max())
        differ += diff > 0
        print("STREAMED_ROWS planned - two launches", k, "max / scale", diff / scale)
        assert diff <= 2 * GRAD_MAX_OF_SCALE * scale, k
    print("STREAMED_ROWS tensors that differ between the forms:", differ, "rows of the thick segments:", rows[thick].tolist())
