"""torch.autograd front-ends of the fused HIP kernels that replace PyTorch-side chains on the training-step path
(include/hgs.h: hgs_strand_geometry_*, hgs_ssim_l1_*, hgs_orientation_loss_*, hgs_magnet_*, hgs_head_penalty_*,
hgs_direction_loss_*).  GPU tensors only."""
import ctypes as C
import math

import torch

import hgs_runtime as rt

_WINDOW = None


def gaussian_window11():
    """The reference's 1-D window: fp32 exp(-(x-5)^2 / (2*1.5^2)), normalised in fp32 (loss/losses.py:24-31)."""
    global _WINDOW
    if _WINDOW is None:
        g = torch.tensor([math.exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)) for x in range(11)])
        g = (g / g.sum()).to(torch.float32)
        _WINDOW = (C.c_float * 11)(*[float(v) for v in g])
    return _WINDOW


def _strand_geometry_launch(endpoints, width, pairs, factor):
    endpoints = rt.require_gpu_tensor(endpoints, "endpoints", torch.float32)
    width = rt.require_gpu_tensor(width, "width", torch.float32)
    pairs = rt.require_gpu_tensor(pairs, "endpoint_pairs", torch.int64)
    P, dev = pairs.shape[0], endpoints.device
    # one allocation for the four outputs (13 floats per segment; every view 16-byte aligned)
    buf = torch.empty((13 * P + 12,), dtype=torch.float32, device=dev)
    o = [0, (3 * P + 3) // 4 * 4]
    o.append(o[1] + (3 * P + 3) // 4 * 4)
    o.append(o[2] + 4 * P)
    xyz, scale = buf[o[0]:o[0] + 3 * P].view(P, 3), buf[o[1]:o[1] + 3 * P].view(P, 3)
    quat, direction = buf[o[2]:o[2] + 4 * P].view(P, 4), buf[o[3]:o[3] + 3 * P].view(P, 3)
    with torch.cuda.device(dev):
        rt.check(rt.lib().hgs_strand_geometry_forward(rt.current_stream(), P, rt.ptr(endpoints), rt.ptr(pairs),
                                                      rt.ptr(width), float(factor), rt.ptr(xyz), rt.ptr(scale),
                                                      rt.ptr(quat), rt.ptr(direction)))
    return endpoints, width, pairs, (xyz, scale, quat, direction)


class _StrandGeometry(torch.autograd.Function):
    @staticmethod
    def forward(ctx, endpoints, width, pairs, factor):
        endpoints, width, pairs, out = _strand_geometry_launch(endpoints, width, pairs, factor)
        ctx.save_for_backward(endpoints, width, pairs)
        ctx.factor = float(factor)
        return out

    @staticmethod
    def backward(ctx, g_xyz, g_scale, g_quat, g_dir):
        endpoints, width, pairs = ctx.saved_tensors
        P, E, dev = pairs.shape[0], endpoints.shape[0], endpoints.device
        gs = [None if g is None else g.contiguous() for g in (g_xyz, g_scale, g_quat, g_dir)]
        d_ep = torch.empty((E, 3), dtype=torch.float32, device=dev)
        d_w = torch.empty((P, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rt.check(rt.lib().hgs_strand_geometry_backward(rt.current_stream(), P, E, rt.ptr(endpoints), rt.ptr(pairs),
                                                           rt.ptr(width), ctx.factor, rt.ptr(gs[0]), rt.ptr(gs[1]),
                                                           rt.ptr(gs[2]), rt.ptr(gs[3]), rt.ptr(d_ep), rt.ptr(d_w)))
        return d_ep, d_w, None, None


def strand_geometry(endpoints, width, pairs, factor):
    """(xyz[P,3], scale[P,3], quat[P,4], direction[P,3]) of every segment, differentiable w.r.t. endpoints/width."""
    if not torch.is_grad_enabled():          # forward-only (render loops): the launch without an autograd node around it
        return _strand_geometry_launch(endpoints, width, pairs, factor)[3]
    return _StrandGeometry.apply(endpoints, width, pairs, factor)


class _SsimL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt):
        img = rt.require_gpu_tensor(img, "image", torch.float32)
        gt = rt.require_gpu_tensor(gt, "gt_image", torch.float32)
        Cc, H, W = img.shape[-3], img.shape[-2], img.shape[-1]
        dev, L = img.device, rt.lib()
        nb = L.hgs_ssim_l1_num_blocks(Cc, H, W)
        dmaps = torch.empty((3, Cc, H, W), dtype=torch.float32, device=dev)
        partials = torch.empty((nb, 2), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rt.check(L.hgs_ssim_l1_forward(rt.current_stream(), Cc, H, W, gaussian_window11(), rt.ptr(img), rt.ptr(gt),
                                           rt.ptr(dmaps), rt.ptr(partials)))
        sums = partials.sum(dim=0) / float(Cc * H * W)
        ctx.save_for_backward(img, gt, dmaps)
        return sums[0], sums[1]  # mean SSIM, mean |img - gt|

    @staticmethod
    def backward(ctx, g_ssim, g_l1):
        img, gt, dmaps = ctx.saved_tensors
        Cc, H, W = img.shape[-3], img.shape[-2], img.shape[-1]
        g_ssim = g_ssim.contiguous().to(torch.float32)
        g_l1 = g_l1.contiguous().to(torch.float32)
        d_img = torch.empty_like(img)
        with torch.cuda.device(img.device):
            rt.check(rt.lib().hgs_ssim_l1_backward(rt.current_stream(), Cc, H, W, gaussian_window11(), rt.ptr(img),
                                                   rt.ptr(gt), rt.ptr(dmaps), rt.ptr(g_ssim), rt.ptr(g_l1), rt.ptr(d_img)))
        return d_img, None


def ssim_l1(img, gt):
    """(mean SSIM, mean L1) of [C,H,W] images in one fused pass (window 11, sigma 1.5, zero padding)."""
    return _SsimL1.apply(img, gt)


class _OrientationLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, omap, viewmatrix, bg, min_val, gt_theta, confidence, mask):
        omap = rt.require_gpu_tensor(omap, "orientation map", torch.float32)
        view = rt.require_gpu_tensor(viewmatrix, "world_view_transform", torch.float32)
        gt_theta = rt.require_gpu_tensor(gt_theta, "orientation_field", torch.float32)
        confidence = rt.require_gpu_tensor(confidence, "orientation_confidence", torch.float32)
        H, W, dev, L = omap.shape[1], omap.shape[2], omap.device, rt.lib()
        mask_u8 = None
        if mask is not None:
            mask = rt.require_gpu_tensor(mask, "mask")
            mask_u8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
        nb = L.hgs_orientation_loss_num_blocks(H, W)
        partials = torch.empty((nb, 2), dtype=torch.float32, device=dev)
        bg3 = (C.c_float * 3)(*bg)
        with torch.cuda.device(dev):
            rt.check(L.hgs_orientation_loss_forward(rt.current_stream(), H, W, rt.ptr(omap), rt.ptr(view), bg3, float(min_val),
                                                    rt.ptr(gt_theta), rt.ptr(confidence), rt.ptr(mask_u8), rt.ptr(partials)))
        sums = partials.sum(dim=0)
        ctx.save_for_backward(omap, view, gt_theta, confidence,
                              mask_u8 if mask_u8 is not None else torch.empty(0, device=dev), sums)
        ctx.consts = (bg3, float(min_val), mask_u8 is not None)
        return sums[0] / sums[1]

    @staticmethod
    def backward(ctx, g):
        omap, view, gt_theta, confidence, mask_u8, sums = ctx.saved_tensors
        bg3, min_val, has_mask = ctx.consts
        H, W = omap.shape[1], omap.shape[2]
        g = g.contiguous().to(torch.float32)
        count = sums[1:2].contiguous()
        d = torch.empty_like(omap)
        with torch.cuda.device(omap.device):
            rt.check(rt.lib().hgs_orientation_loss_backward(rt.current_stream(), H, W, rt.ptr(omap), rt.ptr(view), bg3,
                                                            min_val, rt.ptr(gt_theta), rt.ptr(confidence),
                                                            rt.ptr(mask_u8) if has_mask else None, rt.ptr(g), rt.ptr(count),
                                                            rt.ptr(d)))
        return d, None, None, None, None, None, None


def orientation_loss(omap, viewmatrix, bg3, min_val, gt_theta, confidence, mask):
    return _OrientationLoss.apply(omap, viewmatrix, bg3, min_val, gt_theta, confidence, mask)


class _SmoothnessLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, endpoints, index_pairs, cos_th, eps):
        endpoints = rt.require_gpu_tensor(endpoints, "endpoints", torch.float32)
        idx = rt.require_gpu_tensor(index_pairs, "index_pairs", torch.int64)
        N, dev, L = idx.shape[0], endpoints.device, rt.lib()
        partials = torch.empty((max(L.hgs_smoothness_num_blocks(N), 1), 2), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rt.check(L.hgs_smoothness_forward(rt.current_stream(), N, rt.ptr(endpoints), rt.ptr(idx), float(cos_th),
                                              float(eps), rt.ptr(partials)))
        sums = partials.sum(dim=0)
        ctx.save_for_backward(endpoints, idx, sums)
        ctx.consts = (float(cos_th), float(eps))
        return sums[0] / torch.clamp(sums[1], min=1.0)

    @staticmethod
    def backward(ctx, g):
        endpoints, idx, sums = ctx.saved_tensors
        cos_th, eps = ctx.consts
        g = g.contiguous().to(torch.float32)
        count = sums[1:2].contiguous()
        d = torch.empty_like(endpoints)
        with torch.cuda.device(endpoints.device):
            rt.check(rt.lib().hgs_smoothness_backward(rt.current_stream(), idx.shape[0], endpoints.shape[0],
                                                      rt.ptr(endpoints), rt.ptr(idx), cos_th, eps, rt.ptr(g),
                                                      rt.ptr(count), rt.ptr(d)))
        return d, None, None, None


def smoothness_loss(endpoints, index_pairs, cos_th, eps):
    """Mean squared bending angle over the consecutive-segment pairs bent beyond the threshold (0 if none)."""
    return _SmoothnessLoss.apply(endpoints, index_pairs, cos_th, eps)


class MagnetTable:
    """What the magnet term's device op (include/hgs.h hgs_magnet_*) needs of the topology, built on the host side of a
    topology event: `ends` (the degree-1 endpoint ids, ascending), `partner` (each end's segment partner), `mapping` (the
    zero-initialised id -> partner table of loss/losses.py:137-138), all int32 on the model's device, and the op's scratch.
    MagnetTable.of(model) remembers it on the model for as long as `endpoint_pairs` is the same tensor."""

    def __init__(self, model):
        pairs = model.endpoint_pairs
        ep = model._endpoints
        if not ep.is_cuda:
            raise rt.HgsError("MagnetTable: the model must live on the GPU (libhgs.so has no CPU path)")
        E = int(ep.shape[0])
        if pairs.numel() == 0:          # (no segments: no ends; get_complementary_endpoint_idx needs a non-empty table)
            ends = comp = torch.zeros(0, dtype=torch.long, device=ep.device)
        else:
            u, c = torch.unique(pairs, return_counts=True)
            ends = u[c == 1]
            comp, _ = model.get_complementary_endpoint_idx(ends)
        mapping = torch.zeros(E, device=ep.device, dtype=torch.int32)
        mapping[ends] = comp.to(torch.int32)
        self.pairs, self.E, self.n = pairs, E, int(ends.shape[0])
        self.ends, self.partner, self.mapping = ends.to(torch.int32).contiguous(), comp.to(torch.int32).contiguous(), mapping
        self.scratch_bytes = int(rt.lib().hgs_magnet_scratch_bytes(self.n, E))
        self.scratch = torch.empty((self.scratch_bytes + 256,), dtype=torch.uint8, device=ep.device)
        self.scratch_ptr = (self.scratch.data_ptr() + 255) // 256 * 256

    @classmethod
    def of(cls, model):
        cached = getattr(model, "_magnet_table_cache", None)
        if cached is None or cached.pairs is not model.endpoint_pairs or cached.E != int(model._endpoints.shape[0]):
            cached = model._magnet_table_cache = cls(model)
        return cached


class _MagnetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, endpoints, table, min_val, info):
        endpoints = rt.require_gpu_tensor(endpoints, "endpoints", torch.float32)
        E, n, dev = int(endpoints.shape[0]), table.n, endpoints.device
        if E != table.E:
            raise rt.HgsError(f"magnet_loss: the table was built for {table.E} endpoints, the model has {E}: a topology event "
                              "needs a new MagnetTable (FusedStrandStep.refresh())")
        out = torch.empty((4,), dtype=torch.float32, device=dev)
        ints = torch.empty((n, 5), dtype=torch.int32, device=dev).view(-1)        # sel [n,2] | nn_idx [n,3]
        flts = torch.empty((n, 4), dtype=torch.float32, device=dev).view(-1)      # sq [n] | nn_d2 [n,3]
        sel, nn_idx = ints[:2 * n], ints[2 * n:]
        sq, nn_d2 = flts[:n], flts[n:]
        with torch.cuda.device(dev):
            rt.check(rt.lib().hgs_magnet_forward(rt.current_stream(), E, n, rt.ptr(endpoints), rt.ptr(table.ends),
                                                 rt.ptr(table.partner), rt.ptr(table.mapping), float(min_val), table.scratch_ptr,
                                                 table.scratch_bytes, rt.ptr(out), rt.ptr(sel), rt.ptr(sq), rt.ptr(nn_idx),
                                                 rt.ptr(nn_d2)))
        ctx.save_for_backward(endpoints, out, sel, sq)
        ctx.table = table
        if info is not None:
            info.update(out=out, sel=sel.view(n, 2), sq=sq, nn_idx=nn_idx.view(n, 3), nn_d2=nn_d2.view(n, 3))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        endpoints, out, sel, sq = ctx.saved_tensors
        table = ctx.table
        E, dev = int(endpoints.shape[0]), endpoints.device
        g = g.contiguous().to(torch.float32)
        d = torch.empty_like(endpoints)
        with torch.cuda.device(dev):
            rt.check(rt.lib().hgs_magnet_backward(rt.current_stream(), E, table.n, rt.ptr(endpoints), rt.ptr(table.ends), rt.ptr(sel),
                                                  rt.ptr(sq), rt.ptr(out), rt.ptr(g), 1.0, table.scratch_ptr, table.scratch_bytes,
                                                  rt.ptr(d)))
        return d, None, None, None


def magnet_loss(endpoints, table, min_val, info=None):
    """strand_joints_magnet_loss (loss/losses.py) of `endpoints` under the topology of `table` (a MagnetTable) as one device op:
    the scalar, differentiable w.r.t. endpoints.  `info`: a dict that receives the op's other outputs (device tensors, no copy):
    "out" ([4]: the value; the rows of the mean and the valid ends as int32 bits in [1], [2] -- magnet_rows / magnet_valid read
    them), "sel" ([n,2]: per position of the compacted list the selected position or -1, and the index into table.ends),
    "sq" ([n]), "nn_idx" / "nn_d2" ([n,3]: the three nearest, what knn3_self gives on the valid ends)."""
    return _MagnetLoss.apply(endpoints, table, min_val, info)


def magnet_rows(info):
    """Rows in the mean of the magnet_loss call that filled `info` (one read-back: tests and tools)."""
    return int(info["out"].view(torch.int32)[1])


def magnet_valid(info):
    """Ends that survived the min_val test in the magnet_loss call that filled `info` (one read-back)."""
    return int(info["out"].view(torch.int32)[2])


def set_magnet_search(mode):
    """The neighbour search of magnet_loss, process-wide: None / -1 automatic (by the number of ends), 0 tiles, 1 grid.  Returns
    the previous mode.  A test and A/B switch: both paths give identical bits."""
    return rt.lib().hgs_set_magnet_search(-1 if mode is None else int(mode))


class HeadScratch:
    """What head_penalty keeps between its forward and its backward for E points: g [E, 3], pen and dist [E] (float32) and the
    forward's float64 partial sums.  The fused iteration holds one for the model's E and replaces it in refresh() after a topology
    event; a call without one allocates its own."""

    def __init__(self, E, device):
        E = int(E)
        f32 = dict(dtype=torch.float32, device=device)
        self.E = E
        self.g = torch.empty((E, 3), **f32)
        self.pen, self.dist = torch.empty((E,), **f32), torch.empty((E,), **f32)
        self.partials = torch.empty((max(1, int(rt.lib().hgs_head_penalty_num_blocks(E))),), dtype=torch.float64, device=device)


class _HeadPenalty(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, sdf, margin, info, scratch):
        points = rt.require_gpu_tensor(points, "points", torch.float32)
        if points.dim() != 2 or points.shape[1] != 3:
            raise rt.HgsError(f"head_penalty: points {tuple(points.shape)}: [E, 3] expected")
        E, dev = int(points.shape[0]), points.device
        if scratch is None:
            scratch = HeadScratch(E, dev)
        elif scratch.E != E or scratch.g.device != dev:
            raise rt.HgsError(f"head_penalty: the scratch was made for {scratch.E} points on {scratch.g.device}, the call has {E} on "
                              f"{dev}: a topology event needs a new one (FusedStrandStep.refresh())")
        field = sdf.on(dev)
        phi = field["phi"]
        nx, ny, nz = sdf.shape
        if phi.numel() != nx * ny * nz:
            raise rt.HgsError(f"head_penalty: a field of {phi.numel()} values for a grid of {nx} x {ny} x {nz} nodes")
        out = torch.empty((1,), dtype=torch.float32, device=dev)
        o = sdf.origin32
        with torch.cuda.device(dev):
            rt.check(rt.lib().hgs_head_penalty_forward(rt.current_stream(), E, rt.ptr(points), rt.ptr(phi), nx, ny, nz, float(o[0]),
                                                       float(o[1]), float(o[2]), float(sdf.inv_h32), float(margin), rt.ptr(scratch.g),
                                                       rt.ptr(scratch.pen), rt.ptr(scratch.dist), rt.ptr(scratch.partials), rt.ptr(out)))
        ctx.scratch, ctx.E = scratch, E
        if info is not None:
            info.update(out=out, pen=scratch.pen, dist=scratch.dist, g=scratch.g)
        return out[0]

    @staticmethod
    def backward(ctx, go):
        scratch, E = ctx.scratch, ctx.E
        go = go.contiguous().to(torch.float32)
        d = torch.empty_like(scratch.g)
        with torch.cuda.device(d.device):
            rt.check(rt.lib().hgs_head_penalty_backward(rt.current_stream(), E, rt.ptr(scratch.g), rt.ptr(go), rt.ptr(d)))
        return d, None, None, None, None


def head_penalty(points, sdf, margin, info=None, scratch=None):
    """The head-penetration term (utils/head_sdf.py states it; loss.losses.head_penetration_loss is the same statement in torch ops)
    of `points` [E, 3] against the HeadSDF `sdf` as one device op: the scalar, differentiable w.r.t. points, no host synchronisation.
    `info`: a dict that receives the op's other outputs (device tensors, no copy): "out" ([1]: the value), "pen" and "dist" ([E]: the
    per-point penalty and interpolated distance, +inf out of range), "g" ([E, 3]: the gradient for an upstream of E).  `scratch`: a
    HeadScratch for E points that the call works in (and that the next call overwrites); None: its own."""
    return _HeadPenalty.apply(points, sdf, margin, info, scratch)


class DirectionTable:
    """What the direction term's device op (include/hgs.h hgs_direction_loss_*) needs of the topology, built on the host side of a
    topology event: `pairs` (endpoint_pairs, int64 [S, 2], every entry checked to lie in [0, E) -- the kernels trust it) and the
    incidence CSR of utils/direction_term.py, `offsets` int32 [E + 1] and `entries` int32 [2S] (2 s + side, ascending within an
    endpoint's run), on the model's device.  DirectionTable.of(model) remembers it on the model for as long as `endpoint_pairs` is
    the same tensor."""

    def __init__(self, pairs, E):
        pairs = rt.require_gpu_tensor(pairs, "endpoint_pairs", torch.int64)
        if pairs.dim() != 2 or pairs.shape[1] != 2:
            raise rt.HgsError(f"DirectionTable: endpoint_pairs {tuple(pairs.shape)}: [S, 2] expected")
        E, S = int(E), int(pairs.shape[0])
        if E < 0 or E > (1 << 28) or S > (1 << 28):
            raise rt.HgsError(f"DirectionTable: {E} endpoints and {S} segments (at most 2^28 each)")
        flat = pairs.reshape(-1)
        if S > 0:
            lo, hi = int(flat.min()), int(flat.max())       # (one read-back, on the host side of a topology event)
            if lo < 0 or hi >= E:
                raise rt.HgsError(f"DirectionTable: endpoint_pairs holds endpoint ids from {lo} to {hi}, the model has {E} endpoints")
        self.pairs, self.E, self.S = pairs, E, S
        self.entries = torch.sort(flat, stable=True).indices.to(torch.int32).contiguous()
        offsets = torch.zeros(E + 1, dtype=torch.int64, device=pairs.device)
        if S > 0:
            offsets[1:] = torch.cumsum(torch.bincount(flat, minlength=E), dim=0)
        self.offsets = offsets.to(torch.int32).contiguous()

    @classmethod
    def of(cls, model):
        cached = getattr(model, "_direction_table_cache", None)
        E = int(model._endpoints.shape[0])
        if cached is None or cached[0] is not model.endpoint_pairs or cached[1].E != E:
            if not model._endpoints.is_cuda:
                raise rt.HgsError("DirectionTable: the model must live on the GPU (libhgs.so has no CPU path)")
            cached = model._direction_table_cache = (model.endpoint_pairs, cls(model.endpoint_pairs, E))
        return cached[1]


class DirectionScratch:
    """What direction_loss keeps between its forward and its backward for S segments among E endpoints: gs [S, 3], term and w [S]
    (float32), out [2] and the forward's float64 partial sums.  The fused iteration holds one for the model's topology and replaces
    it in refresh() after a topology event; a call without one allocates its own."""

    def __init__(self, S, E, device):
        S, E = int(S), int(E)
        f32 = dict(dtype=torch.float32, device=device)
        self.S, self.E = S, E
        self.gs = torch.empty((S, 3), **f32)
        self.term, self.w = torch.empty((S,), **f32), torch.empty((S,), **f32)
        self.partials = torch.empty((2 * max(1, int(rt.lib().hgs_direction_loss_num_blocks(S))),), dtype=torch.float64, device=device)


class _DirectionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, table, volume, min_conf, info, scratch):
        points = rt.require_gpu_tensor(points, "points", torch.float32)
        if points.dim() != 2 or points.shape[1] != 3:
            raise rt.HgsError(f"direction_loss: points {tuple(points.shape)}: [E, 3] expected")
        E, S, dev = int(points.shape[0]), table.S, points.device
        if E != table.E or table.pairs.device != dev:
            raise rt.HgsError(f"direction_loss: the table was built for {table.E} endpoints on {table.pairs.device}, the call has {E} on "
                              f"{dev}: a topology event needs a new DirectionTable (FusedStrandStep.refresh())")
        if scratch is None:
            scratch = DirectionScratch(S, E, dev)
        elif scratch.S != S or scratch.E != E or scratch.gs.device != dev:
            raise rt.HgsError(f"direction_loss: the scratch was made for {scratch.S} segments among {scratch.E} endpoints on "
                              f"{scratch.gs.device}, the call has {S} among {E} on {dev}: a topology event needs a new one "
                              "(FusedStrandStep.refresh())")
        vol = volume.on(dev)["vol"]
        nx, ny, nz = volume.shape
        if vol.numel() != 4 * nx * ny * nz:
            raise rt.HgsError(f"direction_loss: a volume of {vol.numel()} values for a grid of {nx} x {ny} x {nz} nodes of 4")
        out = torch.empty((2,), dtype=torch.float32, device=dev)
        o = volume.origin32
        with torch.cuda.device(dev):
            rt.check(rt.lib().hgs_direction_loss_forward(rt.current_stream(), S, rt.ptr(points), rt.ptr(table.pairs), rt.ptr(vol), nx, ny,
                                                         nz, float(o[0]), float(o[1]), float(o[2]), float(volume.inv_h32),
                                                         float(min_conf), rt.ptr(scratch.gs), rt.ptr(scratch.term), rt.ptr(scratch.w),
                                                         rt.ptr(scratch.partials), rt.ptr(out)))
        ctx.scratch, ctx.table = scratch, table
        if info is not None:
            info.update(out=out, term=scratch.term, w=scratch.w, gs=scratch.gs)
        return out[0]

    @staticmethod
    def backward(ctx, go):
        scratch, table = ctx.scratch, ctx.table
        go = go.contiguous().to(torch.float32)
        d = torch.empty((table.E, 3), dtype=torch.float32, device=scratch.gs.device)
        with torch.cuda.device(d.device):
            rt.check(rt.lib().hgs_direction_loss_backward(rt.current_stream(), table.E, table.S, rt.ptr(table.offsets),
                                                          rt.ptr(table.entries), rt.ptr(scratch.gs), rt.ptr(go), rt.ptr(d)))
        return d, None, None, None, None, None


def direction_loss(points, table, volume, min_conf, info=None, scratch=None):
    """The 3-D direction term (utils/direction_term.py states it; loss.losses.strand_direction_loss is the same statement in torch
    ops) of the segments `table` (a DirectionTable) of `points` [E, 3] against the DirectionVolume `volume` as one device op: the
    scalar, differentiable w.r.t. points, no host synchronisation.  `info`: a dict that receives the op's other outputs (device
    tensors, no copy): "out" ([2]: the value; the active segments as int32 bits -- direction_active reads them), "term" and "w" ([S]:
    the per-segment sin^2 and interpolated confidence), "gs" ([S, 3]: d term / d (b - a)).  `scratch`: a DirectionScratch for the
    table's S and E that the call works in (and that the next call overwrites); None: its own."""
    return _DirectionLoss.apply(points, table, volume, min_conf, info, scratch)


def direction_active(info):
    """Segments that passed the gate in the direction_loss call that filled `info` (one read-back: tests and tools)."""
    return int(info["out"].view(torch.int32)[1])


class FusedAdam(torch.optim.Optimizer):
    """Adam with the reference's settings (eps 1e-15, betas (0.9, 0.999), no weight decay, one group per tensor, per-group
    lr) whose whole update is ONE kernel launch (hgs_adam_step).  State layout (`exp_avg`, `exp_avg_sq`, `step` per
    parameter) is torch.optim.Adam's, so the models' optimizer-state surgery works unchanged.  `lr` of a group may be a
    Python float or a device scalar tensor (the latter is what graph capture needs)."""

    def __init__(self, params, lr=0.0, betas=(0.9, 0.999), eps=1e-15):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._lr_dev = {}
        self._call = None
        self._tickets = None   # the kernel's per-tensor ticket words: owned by this optimizer (include/hgs.h hgs_adam_step)
        self._plan = None      # _InlinePlan: the in-lane form of the update (include/hgs.h HgsAdamSlot)
        self._inline_done = False

    def ticket_words(self, dev):
        """The launch's per-tensor ticket words (zero between launches: the kernel wraps them).  Whoever captures step() into a
        graph calls this BEFORE the capture: words created here during a capture live in the graph's pool and are zeroed by that
        graph's replays alone -- a second graph captured after it (several steps per launch) that is replayed first would take
        its tickets from whatever the pool block held, and advance no step counter."""
        if self._tickets is None or self._tickets.device != dev:
            self._tickets = torch.zeros(8, dtype=torch.int32, device=dev)
        return self._tickets

    def inline_plan(self):
        """The plan of the in-lane update for the CURRENT parameter tensors (rebuilt when a tensor, a moment, a step counter or
        a learning-rate tensor has been replaced): device-resident HgsAdamPrep + coefficient table, slots per parameter."""
        rows = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.numel() == 0:
                    continue
                if not p.is_cuda:
                    raise rt.HgsError("FusedAdam runs on the GPU only")
                st = self._state_for(p)
                rows.append((p, st["exp_avg"], st["exp_avg_sq"], self._lr_tensor(gi, group, p.device), st["step"], group))
        key = tuple(t.data_ptr() for r in rows for t in r[:5])
        if self._plan is None or self._plan.key != key:
            if torch.cuda.is_current_stream_capturing():
                # a new plan allocates and uploads from pageable memory: not capturable -- and a graph captured with the OLD plan
                # would go on writing its (freed) tables.  Whoever captures builds the plan first (train.GraphedStep does).
                raise rt.HgsError("FusedAdam.inline_plan(): a parameter / moment / learning-rate tensor was replaced during a "
                                  "graph capture; build the plan (enable_inline_adam) before capturing")
            self._plan = _InlinePlan(self, rows, key)
        return self._plan

    def zero_grad(self, set_to_none=True):
        # an in-lane update that no step() consumed (a backward without an optimizer step) must not swallow a later step()
        self._inline_done = False
        return super().zero_grad(set_to_none=set_to_none)

    def _state_for(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _lr_tensor(self, gi, group, dev):
        lr = group["lr"]
        if torch.is_tensor(lr):
            return lr
        cached = self._lr_dev.get(gi)
        if cached is None or cached[0] != float(lr) or cached[1].device != dev:
            t = cached[1] if cached is not None and cached[1].device == dev else torch.empty((), dtype=torch.float32, device=dev)
            t.fill_(float(lr))
            cached = (float(lr), t)
            self._lr_dev[gi] = cached
        return cached[1]

    @torch.no_grad()
    def step(self, closure=None):
        if self._inline_done:
            # the backward that just ran applied the update in its own lanes (strand_step, _InlinePlan.applied): nothing to
            # launch; the parameters changed in place behind autograd's back, like after the launch below
            self._inline_done = False
            for group in self.param_groups:
                for p in group["params"]:
                    if p.numel():
                        torch.autograd.graph.increment_version(p)
            return None
        rows = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                if not p.is_cuda:
                    raise rt.HgsError("FusedAdam runs on the GPU only")
                st = self._state_for(p)
                rows.append((p, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], self._lr_tensor(gi, group, p.device),
                             st["step"], group))
        if not rows:
            return None
        beta1, beta2 = rows[0][6]["betas"]
        eps = rows[0][6]["eps"]
        key = tuple(t.data_ptr() for r in rows for t in r[:6]) + tuple(r[0].numel() for r in rows)
        if self._call is None or self._call[0] != key:
            n = len(rows)
            arrs = [(C.c_void_p * n)(*[r[j].data_ptr() for r in rows]) for j in range(6)]
            numel = (C.c_longlong * n)(*[r[0].numel() for r in rows])
            self._call = (key, n, arrs, numel)
        _, n, arrs, numel = self._call
        dev = rows[0][0].device
        with torch.cuda.device(dev):
            rt.check(rt.lib().hgs_adam_step(rt.current_stream(), n, arrs[0], arrs[1], arrs[2], arrs[3], arrs[4], arrs[5],
                                            numel, float(beta1), float(beta2), float(eps), self.ticket_words(dev).data_ptr()))
        # the kernel wrote the parameters through raw pointers: tell autograd that they changed in place
        for r in rows:
            torch.autograd.graph.increment_version(r[0])
        return None


class _InlinePlan:
    """FusedAdam.inline_plan(): what the kernels of an iteration with the in-lane update need of the optimizer (include/hgs.h
    HgsAdamPrep / HgsAdamSlot).  `prep_ptr`: the device-resident HgsAdamPrep the iteration's prologue works on."""

    def __init__(self, optimizer, rows, key):
        if len(rows) > rt.ADAM_MAX_TENSORS:
            raise rt.HgsError(f"in-lane Adam: at most {rt.ADAM_MAX_TENSORS} parameter tensors")
        self.optimizer, self.key = optimizer, key
        dev = rows[0][0].device
        beta1, beta2 = rows[0][5]["betas"]
        self.betas, self.eps = (float(beta1), float(beta2)), float(rows[0][5]["eps"])
        self.coef = torch.zeros((len(rows), 2), dtype=torch.float32, device=dev)
        prep = rt.AdamPrep()
        prep.n = len(rows)
        for k, r in enumerate(rows):
            prep.lr[k], prep.step[k] = r[3].data_ptr(), r[4].data_ptr()
        prep.beta1, prep.beta2, prep.coef = self.betas[0], self.betas[1], self.coef.data_ptr()
        self._prep = torch.frombuffer(bytearray(bytes(prep)), dtype=torch.uint8).to(dev)
        self.prep_ptr = self._prep.data_ptr()
        self._keep = rows
        self._slot = {id(r[0]): (r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), self.coef[k].data_ptr()) for k, r in enumerate(rows)}

    def fill(self, adam, params):
        """adam: rt.AdamInline; slot j <- the state of params[j]."""
        for j, p in enumerate(params):
            sl = adam.slot[j]
            sl.p, sl.m, sl.v, sl.coef = self._slot[id(p)]
        adam.beta1, adam.beta2, adam.eps = self.betas[0], self.betas[1], self.eps

    def applied(self):
        """The backward's launches that carry the update are enqueued: the optimizer's next step() launches nothing."""
        self.optimizer._inline_done = True
