"""The float64 statement of the per-pixel loss terms and the bars built on it (tests/test_pixel_f64_cpu.py,
tests/test_pixel_f64_gpu.py).

The orientation statement is the op-by-op form of `loss/losses.py::_orientation_term`, written once with a dtype argument
(the CPU file holds it to that function bit for bit in fp32); the mask term is `F.binary_cross_entropy_with_logits`.  float64
is the reference, fp32 on the CPU the yardstick of every bar.

The direction gradient is graded PER PIXEL, never against the plane's largest element: with g_i the pixel's 3-vector,
    kappa_i = max(1, |o_i| / r_i)            (r_i: float64 norm in the view plane; kappa = 1 where r_i = 0)
    rho_i   = |g_i - g64_i| / (kappa_i |g64_i|)
kappa carries the rounding of the inputs: px, py are sums of three products of size |o|, so an fp32 angle is good to
~kappa ulps.  A pixel is FRAGILE when it sits within DELTA * kappa_i of a kink of the bidirectional difference (e = 0 or
|e| = pi / 2, decided in float64): fp32 atan2 and the subtraction are good to a few ulps of pi, ~1e-6, DELTA = 1e-5 is
ten times that.  There the gradient may take either sign (or be 0, where an fp32 e is exactly 0); it must be finite.
"""
import contextlib
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from tests import pixel_cases as PC

ULP4 = 4.0 * 2.0 ** -23
DELTA = 1e-5
HALF_PI = np.pi / 2

# K: twice the worst ratio measured on the MI355X (DESIGN.md section 2 holds the table), rounded up to a power of two, never
# above 8.  T_O: four times the worst measured |v - v64| / (sum |term| / count), rounded up to one significant digit, never
# above 2e-6 -- the worst case of the 8 + 8 + 8-level fp32 summation of the block sums and the tail.
# Measured: worst ratio 0.75 (direction gradient, stand-alone pair at 725 x 725; 0.70 one-pass), 0.42 (mask term) -> K = 2;
# worst value deviation 2.7e-7 of its scale (one masked pixel) -> T_O = 2e-6.
K_ORI = 2.0
K_BCE = 2.0
T_O = 2e-6
T_B = 1e-7         # the kernel's stated bound of __logf(1 + en) against log1p(en)
MUTANTS = {"no_wrap": "wrap", "kink_sign": "kinks", "no_dn": "unit", "no_shift": "faint", "r0_inf": "zero_in_mask",
           "view_transposed": "unit"}


@contextlib.contextmanager
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def orientation_statement(omap, view, min_val, gt, conf, mask, bg, mutant=None, keep=None):
    """loss/losses.py::_orientation_term after the render, in the dtype of `omap`.  mask: bool [H, W] or None (then omap != bg).
    mutant: one of MUTANTS, a subtly wrong statement for the comparator to reject.  keep: dict that receives theta - gt."""
    o = omap.permute(1, 2, 0)
    h, w = o.shape[:2]
    V = view.t() if mutant == "view_transposed" else view
    pix = (o.flatten(0, 1) @ V[:3, :3])[:, :2]
    nrm = torch.norm(pix, dim=1, keepdim=True)
    if mutant == "no_dn":                  # the gradient through the norm dropped
        nrm = nrm.detach()
    elif mutant == "r0_inf":               # d|p| / dp = p / |p| also at p = 0
        nrm = torch.sqrt((pix * pix).sum(dim=1, keepdim=True))
    pix = pix / (nrm + min_val)
    x, y = pix[:, 0], pix[:, 1]
    if mutant != "no_shift":
        y = torch.where(y < min_val, y + min_val, y)
    theta = torch.atan2(x, y)
    if mutant != "no_wrap":
        theta = torch.where(theta < 0, theta + np.pi, theta)
    theta = theta.reshape(h, w)
    mask = torch.any(o != bg, dim=2) if mask is None else mask
    e = theta - gt
    diff = HALF_PI - torch.abs(torch.abs(e) - HALF_PI)
    if mutant == "kink_sign":              # the value is right, the gradient's sign is inverted beyond |e| = pi / 2
        diff = torch.where(torch.abs(e) > HALF_PI, 2 * diff.detach() - diff, diff)
    diff = diff * conf
    m = mask.to(diff.dtype)
    if keep is not None:
        keep["e"] = e.detach()
        keep["terms"] = (diff * m).detach()
        keep["mask"] = mask
    return (diff * m).sum() / m.sum()


def run_orientation(case, dtype, mutant=None):
    """(value, gradient [3, H, W] as float64 numpy, theta - gt, masked terms, mask) of the statement in `dtype`."""
    d = case if isinstance(case, types.SimpleNamespace) else PC.direction_case(*case)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    omap = t(d.omap).requires_grad_(True)
    keep = {}
    with _one_thread():
        v = orientation_statement(omap, t(PC.VIEW), PC.MIN_VAL, t(d.gt), t(d.conf),
                                  None if d.mask is None else torch.tensor(d.mask != 0), t(np.asarray(d.bg, dtype=np.float32)), mutant, keep)
        g, = torch.autograd.grad(v, omap)
    return float(v.detach()), g.double().numpy(), keep["e"].double().numpy(), keep["terms"].double().numpy(), keep["mask"].numpy()


def _kink_sign(e):
    return np.sign(np.abs(e) - HALF_PI) * np.sign(e)


def _norm3(g):
    return np.sqrt((np.asarray(g, dtype=np.float64) ** 2).sum(axis=0))


def pixel_rho(g, ref, scale=1.0):
    """rho_i of a [3, H, W] gradient for an upstream factor `scale` (0 outside the mask and where conf = 0).  On fragile pixels:
    against the nearer of +-g64_i, and 0 for a gradient that is exactly 0."""
    g = np.asarray(g, dtype=np.float64)
    g64 = ref.g64 * scale
    den = ref.kappa * _norm3(g64)
    live = ref.live
    rho = np.zeros(g.shape[1:])
    with np.errstate(invalid="ignore", divide="ignore"):
        plus = _norm3(g - g64) / den
        minus = _norm3(g + g64) / den
    rho[live] = plus[live]
    fr = live & ref.fragile
    rho[fr] = np.where(_norm3(g)[fr] == 0.0, 0.0, np.minimum(plus[fr], minus[fr]))
    return rho


def direction_report(g, ref, scale=1.0):
    """(worst rho in yardsticks, problems): comparator of the direction gradient.  Problems: non-finite elements, a non-zero
    element outside the mask or where the confidence is 0."""
    g = np.asarray(g)
    problems = []
    if not np.isfinite(g).all():
        return float("inf"), ["non-finite"]
    if g[:, ~ref.mask].any():
        problems.append("non-zero outside the mask")
    if g[:, ref.mask & (ref.conf == 0)].any():
        problems.append("non-zero at confidence 0")
    rho = pixel_rho(g, ref, scale)
    return float(rho.max()) / ref.yard if rho.size else 0.0, problems


def accepts_direction(g, ref, K, scale=1.0):
    worst, problems = direction_report(g, ref, scale)
    return worst <= K and not problems


def orientation_reference(case):
    """The float64 statement, the fp32 yardstick and the per-pixel quantities of the comparator for one direction case."""
    d = PC.direction_case(*case)
    v64, g64, e64, terms, mask = run_orientation(d, torch.float64)
    v32, g32, e32, _, mask32 = run_orientation(d, torch.float32)
    assert np.array_equal(mask, mask32)
    if not mask.any():      # 0 / 0: the value is NaN and torch's gradient with it; the kernels write zeros (no pixel has a term)
        g64, g32 = np.zeros_like(g64), np.zeros_like(g32)
    flat = d.omap.reshape(3, -1).T
    p = PC.view_plane(flat)
    r = np.hypot(p[:, 0], p[:, 1]).reshape(d.gt.shape)
    onorm = np.linalg.norm(flat.astype(np.float64), axis=1).reshape(d.gt.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(r > 0, np.maximum(1.0, onorm / r), 1.0)
    conf = d.conf.astype(np.float64)
    live = mask & (conf != 0)
    ae = np.abs(e64)
    fragile = live & (np.minimum(ae, np.abs(ae - HALF_PI)) <= DELTA * kappa)
    ref = types.SimpleNamespace(case=case, v64=v64, v32=v32, g64=g64, g32=g32, e64=e64, e32=e32, mask=mask, conf=conf, r=r,
                                kappa=kappa, live=live, fragile=fragile, count=int(mask.sum()),
                                term_scale=float(np.abs(terms).sum()) / max(int(mask.sum()), 1))
    ref.sign_flips = int((live & ~fragile & (_kink_sign(e32) != _kink_sign(e64))).sum())
    ref.fragile_share = float(fragile.sum()) / max(int(mask.sum()), 1)
    ref.yard = 1.0                          # (pixel_rho needs none)
    rho32 = pixel_rho(g32, ref)
    ref.e_ref = float(rho32.max()) if rho32.size else 0.0
    ref.yard = max(ref.e_ref, ULP4)
    return ref


@functools.lru_cache(maxsize=None)
def orientation_case_reference(case):
    return orientation_reference(case)


def value_ok(v, ref, K=K_ORI, T=T_O):
    """|v - v64| <= max(K |v32 - v64|, T * sum|term| / count); an empty mask gives NaN, as the reference."""
    if ref.count == 0:
        return bool(np.isnan(v) and np.isnan(ref.v64))
    return abs(v - ref.v64) <= max(K * abs(ref.v32 - ref.v64), T * ref.term_scale)


# ---- the mask term -----------------------------------------------------------------------------------------------------------------
def _run_bce(x, y, dtype):
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    with _one_thread():
        b = F.binary_cross_entropy_with_logits(xt, torch.tensor(np.asarray(y), dtype=dtype))
        g, = torch.autograd.grad(b, xt)
    return float(b.detach()), g.double().numpy() * x.size      # the gradient at its natural scale: sigmoid(x) - y


@functools.lru_cache(maxsize=None)
def bce_case_reference(case):
    x, y = PC.logit_case(*case)
    b64, g64 = _run_bce(x, y, torch.float64)
    b32, g32 = _run_bce(x, y, torch.float32)
    e_ref = float(np.abs(g32 - g64).max())
    return types.SimpleNamespace(case=case, b64=b64, b32=b32, g64=g64, g32=g32, e_ref=e_ref, yard=max(e_ref, ULP4))


def bce_report(g, ref, g_mask):
    """Worst |g / g_mask - (sigmoid64(x) - y)| over the pixels, in yardsticks; inf for a non-finite plane."""
    g = np.asarray(g, dtype=np.float64)
    if not np.isfinite(g).all():
        return float("inf")
    return float(np.abs(g / g_mask - ref.g64).max()) / ref.yard


def bce_value_ok(b, ref, K=K_BCE):
    return abs(b - ref.b64) <= max(K * abs(ref.b32 - ref.b64), T_B)


def head_total(total_fwd, l_mask, mask64, l_ori, ori64):
    """The fmaf chain of csrc/hgs_head_tail.h on the float64 terms, from the head forward's own SSIM / L1 part."""
    return l_ori * ori64 + (l_mask * mask64 + total_fwd)
