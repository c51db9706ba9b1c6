"""Image metrics of rendered views against their capture: the per-view PSNR / SSIM report of 3DGS's metrics.py, plus the two
hair-specific images (foreground mask and orientation map).  Driver: view_metrics.py.

Every view is rendered once, forward only, by render_multi on a black background (render_planes): the RGB image, the foreground
channel of extra4 = (get_mask >= foreground_binarization_th).float() and the world-space direction channels of get_orientation --
what render.py types 0, 2 and 4 render.  pred = the RGB render clamped to [0, 1], gt = camera.original_image.

  psnr              10 log10(1 / MSE), MSE = mean over 3 H W of (pred - gt)^2; MSE = 0 gives inf.
  ssim, l1          mean SSIM and mean |pred - gt| as loss/losses.py ssim / l1_loss (reference loss/losses.py:16-17, 43-84); on
                    the GPU from the fused hgs_ssim_l1_forward, on the CPU from losses.ssim / l1_loss.
  psnr_hair         PSNR over the GT-mask pixels, all 3 channels.  None without a mask or when the mask is empty.
  mask_iou          |P & G| / |P | G|, P = rendered foreground channel >= fg_threshold (0.5), G = GT mask; 1.0 when both are
                    empty.  None without a mask (or without a foreground plane).
  orient_err_deg    mean bidirectional angle difference in degrees, unweighted, over the orientation mask.
  orient_within_10, orient_within_20
                    fraction of the orientation-mask pixels whose difference is <= float32(10 pi / 180) / float32(20 pi / 180).
  orient_loss       sum of diff * confidence / count over the orientation mask: the training term loss/losses.py::_orientation_term
                    (reference loss/losses.py:224-289).

The orientation mask and the angle follow _orientation_term statement by statement: the mask is the GT mask, or any(omap != 0)
where the view has none; pix = omap @ world_view_transform[:3, :3], [:2], normalised by (norm + min_val), y += min_val where
y < min_val, theta = atan2(x, y) wrapped into [0, pi), diff = pi/2 - | |theta - gt| - pi/2 |.  A missing confidence counts as
weight 1.  Every orientation key is None for a view without an orientation field, or whose orientation mask is empty.

CUDA tensors go through csrc/hgs_view_stats.hip (hgs_view_stats); CPU tensors through _cpu_stats, the same statements in torch:
float32 per pixel, in the same order (matrix product written out as (o0 w00 + o1 w10) + o2 w20, the norm as sqrt(x x + y y)),
summed in float64.  That restatement is what the kernel is tested against: per-pixel values agree bit for bit except where
atan2 rounds differently (one ulp), and the sums differ only in the order of their float64 additions.

These are fit scores: the capture has no held-out split (neither the reference nor this port reads --eval), so every view scored
is a view the model was trained on."""
import math

import numpy as np
import torch

# rows of hgs_view_stats' output (include/hgs.h HGS_VIEW_STATS_N)
STATS = ["sse", "sse_hair", "mask_count", "fg_count", "inter_count", "orient_abs_sum", "orient_weighted_sum", "orient_count",
         "orient_within_10_count", "orient_within_20_count"]
METRICS = ["psnr", "ssim", "l1", "psnr_hair", "mask_iou", "orient_err_deg", "orient_within_10", "orient_within_20", "orient_loss"]
MIN_VAL = 1e-7   # GaussianModel.min_val

_HALF_PI = np.float32(np.pi / 2)
_PI = np.float32(np.pi)
TH10 = np.float32(10 * np.pi / 180)
TH20 = np.float32(20 * np.pi / 180)


def _psnr(sse, n):
    mse = sse / n
    return math.inf if mse == 0 else 10.0 * math.log10(1.0 / mse)


def _check(name, t, shape, device):
    if t is None:
        return None
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"view_metrics: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if t.device != device:
        raise ValueError(f"view_metrics: {name} is on {t.device}, the render on {device}")
    return t


def _cpu_stats(pred, gt, fg, mask, omap, viewmats, gt_theta, confidence, min_val, fg_threshold):
    """[V, len(STATS)] float64: the statements the kernel restates, on CPU tensors (pred already clamped)."""
    V = pred.shape[0]
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    out = torch.zeros((V, len(STATS)), dtype=torch.float64)
    d = pred - gt
    e = (d * d).double()
    out[:, 0] = e.sum(dim=(1, 2, 3))
    m = None
    if mask is not None:
        m = mask != 0
        out[:, 1] = torch.where(m[:, None], e, torch.zeros((), dtype=torch.float64)).sum(dim=(1, 2, 3))
        out[:, 2] = m.sum(dim=(1, 2)).double()
    if fg is not None:
        p = fg >= f32(fg_threshold)
        out[:, 3] = p.sum(dim=(1, 2)).double()
        if m is not None:
            out[:, 4] = (p & m).sum(dim=(1, 2)).double()
    if omap is not None and gt_theta is not None:
        w = viewmats.reshape(V, 16)[:, :, None, None]
        o0, o1, o2 = omap[:, 0], omap[:, 1], omap[:, 2]
        mv = f32(min_val)
        px = o0 * w[:, 0] + o1 * w[:, 4] + o2 * w[:, 8]
        py = o0 * w[:, 1] + o1 * w[:, 5] + o2 * w[:, 9]
        n = torch.sqrt(px * px + py * py) + mv
        x, y = px / n, py / n
        y = torch.where(y < mv, y + mv, y)
        theta = torch.atan2(x, y)
        theta = torch.where(theta < 0, theta + f32(_PI), theta)
        diff = f32(_HALF_PI) - torch.abs(torch.abs(theta - gt_theta) - f32(_HALF_PI))
        wdiff = diff * confidence if confidence is not None else diff
        om = m if m is not None else (o0 != 0) | (o1 != 0) | (o2 != 0)
        zero = torch.zeros((), dtype=torch.float64)
        out[:, 5] = torch.where(om, diff.double(), zero).sum(dim=(1, 2))
        out[:, 6] = torch.where(om, wdiff.double(), zero).sum(dim=(1, 2))
        out[:, 7] = om.sum(dim=(1, 2)).double()
        out[:, 8] = ((diff <= f32(TH10)) & om).sum(dim=(1, 2)).double()
        out[:, 9] = ((diff <= f32(TH20)) & om).sum(dim=(1, 2)).double()
    return out


def _gpu_stats(pred, gt, fg, mask, omap, viewmats, gt_theta, confidence, min_val, fg_threshold):
    import hgs_runtime as rt
    V, _, H, W = pred.shape
    L = rt.lib()
    c = lambda t: None if t is None else t.contiguous()   # noqa: E731
    mask_u8 = None
    if mask is not None:
        mask_u8 = mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else (mask != 0).to(torch.uint8).contiguous()
    vm = None if viewmats is None else viewmats.reshape(V, 16).to(torch.float32).contiguous()
    nb = L.hgs_view_stats_num_blocks(H, W)
    partials = torch.empty((V, nb, len(STATS)), dtype=torch.float64, device=pred.device)
    out = torch.empty((V, len(STATS)), dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        rt.check(L.hgs_view_stats(rt.current_stream(), V, H, W, rt.ptr(pred), rt.ptr(gt), rt.ptr(mask_u8), rt.ptr(c(fg)),
                                  float(fg_threshold), rt.ptr(c(omap)), rt.ptr(vm), rt.ptr(c(gt_theta)), rt.ptr(c(confidence)),
                                  float(min_val), rt.ptr(partials), rt.ptr(out)))
    return out.cpu()


def _ssim_l1(pred, gt):
    """[V] mean SSIM and [V] mean L1, one view at a time (float64 host tensors)."""
    with torch.no_grad():
        if pred.is_cuda:
            from hgs_runtime.fused import ssim_l1
            pairs = [torch.stack(ssim_l1(pred[v], gt[v])) for v in range(pred.shape[0])]
        else:
            from loss.losses import l1_loss, ssim
            pairs = [torch.stack((ssim(pred[v], gt[v]), l1_loss(pred[v], gt[v]))) for v in range(pred.shape[0])]
        s = torch.stack(pairs).double().cpu()
    return s[:, 0], s[:, 1]


def metrics_from_stats(row, hw, ssim_v, l1_v, has_mask, has_fg, has_orient):
    """One view's dict from its stats row (STATS order), its pixel count and its SSIM / L1."""
    r = {k: float(row[i]) for i, k in enumerate(STATS)}
    m = {"psnr": _psnr(r["sse"], 3.0 * hw), "ssim": float(ssim_v), "l1": float(l1_v)}
    m["psnr_hair"] = _psnr(r["sse_hair"], 3.0 * r["mask_count"]) if has_mask and r["mask_count"] > 0 else None
    if has_mask and has_fg:
        union = r["fg_count"] + r["mask_count"] - r["inter_count"]
        m["mask_iou"] = 1.0 if union == 0 else r["inter_count"] / union
    else:
        m["mask_iou"] = None
    n = r["orient_count"]
    if has_orient and n > 0:
        m["orient_err_deg"] = math.degrees(r["orient_abs_sum"] / n)
        m["orient_within_10"] = r["orient_within_10_count"] / n
        m["orient_within_20"] = r["orient_within_20_count"] / n
        m["orient_loss"] = r["orient_weighted_sum"] / n
    else:
        for k in ("orient_err_deg", "orient_within_10", "orient_within_20", "orient_loss"):
            m[k] = None
    if not has_mask:
        r["sse_hair"] = r["mask_count"] = r["inter_count"] = None
    if not has_fg:
        r["fg_count"] = r["inter_count"] = None
    if not has_orient:
        for k in STATS[5:]:
            r[k] = None
    m.update(r)
    m["union_count"] = None if m["inter_count"] is None else r["fg_count"] + r["mask_count"] - r["inter_count"]
    m["pixels"] = int(hw)
    return m


def view_metrics(pred_rgb, gt_rgb, fg=None, gt_mask=None, omap=None, viewmats=None, gt_theta=None, confidence=None,
                 min_val=MIN_VAL, fg_threshold=0.5):
    """One dict per view (METRICS, then the raw sums and counts of STATS, union_count and pixels) for [V, ...] planes of one
    size: pred_rgb, gt_rgb [V,3,H,W]; fg [V,H,W] (rendered foreground channel); gt_mask [V,H,W] (bool or nonzero = set); omap
    [V,3,H,W] (rendered world-space directions); viewmats [V,4,4] (world_view_transform); gt_theta, confidence [V,H,W].  CUDA
    tensors go to the kernel, CPU tensors to the torch restatement; mixed devices are an error."""
    if pred_rgb.dim() != 4 or pred_rgb.shape[1] != 3:
        raise ValueError(f"view_metrics: pred_rgb must be [V,3,H,W], got {tuple(pred_rgb.shape)}")
    V, _, H, W = pred_rgb.shape
    dev = pred_rgb.device
    _check("gt_rgb", gt_rgb, (V, 3, H, W), dev)
    _check("fg", fg, (V, H, W), dev)
    _check("gt_mask", gt_mask, (V, H, W), dev)
    _check("omap", omap, (V, 3, H, W), dev)
    _check("gt_theta", gt_theta, (V, H, W), dev)
    _check("confidence", confidence, (V, H, W), dev)
    has_orient = omap is not None and gt_theta is not None
    if has_orient:
        if viewmats is None:
            raise ValueError("view_metrics: an orientation map needs viewmats")
        _check("viewmats", viewmats.reshape(V, -1), (V, 16), dev)
    f = lambda t: None if t is None else t.detach().to(torch.float32)   # noqa: E731
    with torch.no_grad():
        pred = pred_rgb.detach().to(torch.float32).clamp(0.0, 1.0).contiguous()
        gt = gt_rgb.detach().to(torch.float32).contiguous()
        args = (pred, gt, f(fg), None if gt_mask is None else gt_mask.detach(), f(omap) if has_orient else None,
                f(viewmats) if has_orient else None, f(gt_theta) if has_orient else None, f(confidence) if has_orient else None,
                min_val, fg_threshold)
        stats = _gpu_stats(*args) if dev.type == "cuda" else _cpu_stats(*args)
        ssim_v, l1_v = _ssim_l1(pred, gt)
    return [metrics_from_stats(stats[v], H * W, ssim_v[v], l1_v[v], gt_mask is not None, fg is not None, has_orient)
            for v in range(V)]


def render_planes(camera, gaussians):
    """(rgb [3,H,W], fg [H,W], omap [3,H,W]) of one camera from one forward-only render_multi pass on a black background; works
    for GaussianModel and HairGaussianModel.  fg: the blended (get_mask >= foreground_binarization_th).float(), omap: the
    blended get_orientation."""
    from gaussian_renderer import render_multi
    with torch.no_grad():
        th = gaussians.foreground_binarization_th
        extra = torch.cat(((gaussians.get_mask >= th).float(), gaussians.get_orientation), dim=1).contiguous()
        bg = torch.zeros(3, dtype=torch.float32, device=extra.device)
        pkg = render_multi(camera, gaussians, bg, extra, splits=(1, 3), black_background=True)
        rgb, (fg, omap) = pkg["render"], pkg["extra"]
    return rgb, fg, omap


def _group_key(cam):
    return (int(cam.image_height), int(cam.image_width), cam.mask is not None, cam.orientation_field is not None,
            cam.orientation_confidence is not None)


def score_cameras(cameras, gaussians, batch=8, fg_threshold=0.5):
    """{image_name: view_metrics dict} for every camera, in image-name order.  Cameras of one size and one set of planes are
    scored together, `batch` views per kernel launch; a view's numbers do not depend on its batch."""
    cams = sorted(cameras, key=lambda c: c.image_name)
    names = [c.image_name for c in cams]
    if len(set(names)) != len(names):
        raise ValueError("score_cameras: image names are not unique")
    groups = {}
    for c in cams:
        groups.setdefault(_group_key(c), []).append(c)
    res = {}
    step = max(1, int(batch))
    for (_, _, has_mask, has_orient, has_conf), group in groups.items():
        for b0 in range(0, len(group), step):
            chunk = group[b0:b0 + step]
            planes = [render_planes(c, gaussians) for c in chunk]
            with torch.no_grad():
                rgb = torch.stack([p[0] for p in planes])
                fg = torch.stack([p[1] for p in planes])
                omap = torch.stack([p[2] for p in planes]) if has_orient else None
                gt = torch.stack([c.original_image[0:3] for c in chunk]).to(rgb.device)
                mask = torch.stack([c.mask for c in chunk]).to(rgb.device) if has_mask else None
                theta = torch.stack([c.orientation_field for c in chunk]).to(rgb.device) if has_orient else None
                conf = torch.stack([c.orientation_confidence for c in chunk]).to(rgb.device) if has_orient and has_conf else None
                vms = torch.stack([c.world_view_transform for c in chunk]).to(rgb.device) if has_orient else None
            out = view_metrics(rgb, gt, fg=fg, gt_mask=mask, omap=omap, viewmats=vms, gt_theta=theta, confidence=conf,
                               min_val=gaussians.min_val, fg_threshold=fg_threshold)
            for c, m in zip(chunk, out):
                res[c.image_name] = m
    return {n: res[n] for n in names}
