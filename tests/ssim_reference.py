"""The float64 statement of the SSIM / L1 pair and the bars built on it (tests/test_ssim_f64_cpu.py, tests/test_ssim_f64_gpu.py).

The reference is `loss.losses.ssim` / `l1_loss` called on float64 tensors: `_window` casts the fp32-rounded 11 x 11 window to the
input's dtype, so it is the reference's function with the reference's window at high precision -- no new arithmetic to trust.
The yardstick of every bar is the fp32 reference's own distance from it on the same pair, computed on the CPU once per case.
"""
import contextlib
import functools
import types

import numpy as np
import torch

from tests import ssim_cases as SC

ULP4 = 4.0 * 2.0 ** -23            # four fp32 ulps of the scale: the floor under the reference's own error


@contextlib.contextmanager
def _one_thread():
    """Images of a few thousand pixels: torch's CPU thread pool costs these convolutions ten times what it saves them."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _run(img, tgt, dtype):
    from loss import losses as Ls
    x = torch.tensor(np.asarray(img), dtype=dtype, requires_grad=True)
    y = torch.tensor(np.asarray(tgt), dtype=dtype)
    with _one_thread():
        s = Ls.ssim(x, y)
        g, = torch.autograd.grad(s, x)
        l1 = Ls.l1_loss(x.detach(), y)
    return float(s.detach()), float(l1), g.double().numpy()


def reference(img, tgt):
    """S64, L1_64, g64 = d mean SSIM / d image in float64; S32, g32 the same statements in fp32 (CPU)."""
    S64, L64, g64 = _run(img, tgt, torch.float64)
    S32, _, g32 = _run(img, tgt, torch.float32)
    return types.SimpleNamespace(S64=S64, L64=L64, g64=g64, S32=S32, g32=g32, scale=float(np.abs(g64).max()),
                                 e_ref=float(np.abs(g32 - g64).max()))


@functools.lru_cache(maxsize=None)
def case_reference(case):
    return reference(*SC.pair(*case))


def block_yardsticks(ref, shape):
    """Per block of the kernel's grid: (block, e_ref over the block, max |g64| over the block grown by REACH px)."""
    C, H, W = shape
    err, mag = np.abs(ref.g32 - ref.g64), np.abs(ref.g64)
    out = []
    for blk in SC.blocks(shape):
        c, y0, y1, x0, x1 = blk
        R = SC.REACH
        out.append((blk, float(err[c, y0:y1, x0:x1].max()),
                    float(mag[c, max(y0 - R, 0):min(y1 + R, H), max(x0 - R, 0):min(x1 + R, W)].max())))
    return out


def gradient_ratios(g, ref, shape):
    """How far `g` is from the float64 gradient in units of the yardstick max(e_ref, 4 ulp scale): (global ratio, worst block's
    ratio, blocks that must be exactly zero -- local scale 0 -- and are not).  A ratio <= K is comparator a."""
    g = np.asarray(g, dtype=np.float64)
    d = np.abs(g - ref.g64)
    bar = max(ref.e_ref, ULP4 * ref.scale)
    glob = float(d.max()) / bar if bar > 0 else (0.0 if not d.any() else float("inf"))
    worst, nonzero = 0.0, []
    for (c, y0, y1, x0, x1), e_blk, s_blk in block_yardsticks(ref, shape):
        if s_blk == 0.0:
            if g[c, y0:y1, x0:x1].any():
                nonzero.append((c, y0, x0))
            continue
        worst = max(worst, float(d[c, y0:y1, x0:x1].max()) / max(e_blk, ULP4 * s_blk))
    return glob, worst, nonzero


def accepts(g, ref, shape, K):
    """Comparator a: global and per-block bars, exact zeros where the local scale is zero; NaN / Inf never pass."""
    if not np.isfinite(np.asarray(g)).all():
        return False
    glob, worst, nonzero = gradient_ratios(g, ref, shape)
    return glob <= K and worst <= K and not nonzero
