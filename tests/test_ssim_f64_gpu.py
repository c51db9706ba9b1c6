"""hgs_ssim_l1_* (stand-alone) and hgs_loss_head_* (what training runs) against the float64 statement of SSIM / L1 on the
images of tests/ssim_cases.py.

The yardstick is the fp32 torch reference's own distance from float64 on the same pair (tests/ssim_reference.py;
tests/test_ssim_f64_cpu.py caps it): three filtered moments rounded differently stay within a small multiple K of it, a wrong
tap does not (test e).  K and T_S come from the table in DESIGN.md section 2 by the rules written there:
  K   = twice the worst measured ratio max|g_hip - g64| / max(e_ref, 4 ulp scale), global or per block, rounded up to a
        power of two; never above 8;
  T_S = four times the worst measured |S_hip - S64|, rounded up to one significant digit; never above 2e-5.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ssim_cases as SC
from tests import ssim_reference as R

pytestmark = pytest.mark.gpu

K = 8.0
T_S = 2e-5


def _dev(a):
    return torch.tensor(np.asarray(a), device="cuda")


def _front_end(case):
    """The product's entry point, hgs_runtime.fused.ssim_l1: (S, L1, d S / d image, d L1 / d image)."""
    from hgs_runtime.fused import ssim_l1
    img, tgt = SC.pair(*case)
    x = _dev(img).requires_grad_(True)
    s, l1 = ssim_l1(x, _dev(tgt))
    gs, = torch.autograd.grad(s, x, retain_graph=True)
    gl, = torch.autograd.grad(l1, x)
    return float(s.detach()), float(l1.detach()), gs.cpu().numpy(), gl.cpu().numpy()


def _c_abi(case, g_ssim, g_l1, window=None):
    """hgs_ssim_l1_forward / _backward through the C ABI with every output buffer (and the derivative maps between the two
    kernels) pre-filled with NaN; `window`: 11 floats, None = the product's.  Returns (partials [nb, 2], d_image), numpy."""
    import hgs_runtime as rt
    from hgs_runtime.fused import gaussian_window11
    img, tgt = (_dev(t) for t in SC.pair(*case))
    Cc, H, W = img.shape
    L = rt.lib()
    nb = L.hgs_ssim_l1_num_blocks(Cc, H, W)
    assert nb == SC.num_blocks(case[1])
    nan = float("nan")
    dmaps = torch.full((3, Cc, H, W), nan, device="cuda")
    partials = torch.full((nb, 2), nan, device="cuda")
    d_img = torch.full((Cc, H, W), nan, device="cuda")
    win = gaussian_window11() if window is None else (C.c_float * 11)(*[float(v) for v in window])
    gs, gl = torch.full((1,), float(g_ssim), device="cuda"), torch.full((1,), float(g_l1), device="cuda")
    rt.check(L.hgs_ssim_l1_forward(rt.current_stream(), Cc, H, W, win, img.data_ptr(), tgt.data_ptr(), dmaps.data_ptr(),
                                   partials.data_ptr()))
    rt.check(L.hgs_ssim_l1_backward(rt.current_stream(), Cc, H, W, win, img.data_ptr(), tgt.data_ptr(), dmaps.data_ptr(),
                                    gs.data_ptr(), gl.data_ptr(), d_img.data_ptr()))
    torch.cuda.synchronize()
    return partials.cpu().numpy(), d_img.cpu().numpy()


def _structural_zero_blocks(case):
    """Blocks around which both images are black as far as the gradient reaches: nothing but zeros enters their arithmetic."""
    a, b = SC.pair(*case)
    out = []
    for c, y0, y1, x0, x1 in SC.blocks(case[1]):
        sl = (c, slice(max(y0 - SC.REACH, 0), y1 + SC.REACH), slice(max(x0 - SC.REACH, 0), x1 + SC.REACH))
        if not a[sl].any() and not b[sl].any():
            out.append((c, y0, y1, x0, x1))
    return out


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_ssim_gradient_against_float64(case):
    """a. d mean SSIM / d image: globally and per block of the kernel's grid within K yardsticks of float64; exactly zero where
    the float64 gradient's local scale is (and in every block that only zeros reach)."""
    ref = R.case_reference(case)
    _, _, g, _ = _front_end(case)
    assert np.isfinite(g).all()
    glob, worst, nonzero = R.gradient_ratios(g, ref, case[1])
    print(f"ratio | {SC.case_id(case)} | {ref.e_ref / ref.scale:.1e} | {glob:.2f} | {worst:.2f} |")
    assert not nonzero, nonzero
    for c, y0, y1, x0, x1 in _structural_zero_blocks(case):
        assert not g[c, y0:y1, x0:x1].any(), (c, y0, x0)
    assert glob <= K and worst <= K, (glob, worst)
    assert R.accepts(g, ref, case[1], K)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_values_against_float64(case):
    """b. L1 to 1e-6 relative (exactly 0 on identical images); mean SSIM within max(K |S32 - S64|, T_S)."""
    ref = R.case_reference(case)
    s, l1, _, _ = _front_end(case)
    print(f"value | {SC.case_id(case)} | {abs(s - ref.S64):.1e} | {abs(ref.S32 - ref.S64):.1e} | {abs(l1 - ref.L64) / max(ref.L64, 1e-300):.1e} |")
    assert abs(l1 - ref.L64) <= 1e-6 * ref.L64
    if case[0] == "identical":
        assert l1 == 0.0
    assert abs(s - ref.S64) <= max(K * abs(ref.S32 - ref.S64), T_S), (s, ref.S64, ref.S32)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_l1_gradient_is_the_sign_over_n(case):
    """c. Upstream (g_ssim, g_l1) = (0, 1): sign(image - target) * fp32(1 / N) to 1 ulp, exactly 0 at ties -- and finite: an
    Inf or NaN in the filtered maps would come through 0 * map as NaN."""
    img, tgt = SC.pair(*case)
    _, g = _c_abi(case, 0.0, 1.0)
    assert np.isfinite(g).all()
    n = np.float32(1.0) / np.float32(img.size)
    sgn = np.sign(img.astype(np.float64) - tgt.astype(np.float64))
    assert not g[sgn == 0].any()
    assert np.abs(g.astype(np.float64) - sgn * np.float64(n)).max() <= np.spacing(n)
    if case[0] in ("identical", "render_black", "hair_black_bg", "impulse"):
        assert (sgn == 0).any()


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_every_block_is_written_once(case):
    """d. Outputs and derivative maps pre-filled with NaN: every partial sum and every gradient pixel is finite afterwards, the
    partial sums add up to the front end's values, and the gradient passes comparator a."""
    ref = R.case_reference(case)
    partials, g = _c_abi(case, 1.0, 0.0)
    assert np.isfinite(partials).all() and np.isfinite(g).all()
    n = float(np.prod(case[1]))
    s, l1 = partials.astype(np.float64).sum(axis=0) / n
    assert abs(l1 - ref.L64) <= 1e-6 * ref.L64
    assert abs(s - ref.S64) <= max(K * abs(ref.S32 - ref.S64), T_S)
    assert R.accepts(g, ref, case[1], K), R.gradient_ratios(g, ref, case[1])


@pytest.mark.parametrize("tap,factor", [(0, 1.02), (5, 1.0 + 1e-4)])
@pytest.mark.parametrize("case", SC.PERTURBED, ids=SC.case_id)
def test_the_bar_sees_a_wrong_window(case, tap, factor):
    """e. The window is an argument of the C ABI: with its outermost tap off by 2 %, or its centre tap by 1e-4, the same
    kernels must FAIL comparator a against the unperturbed float64 reference (and pass it with the window as it is)."""
    from hgs_runtime.fused import gaussian_window11
    ref = R.case_reference(case)
    win = [float(v) for v in gaussian_window11()]
    _, g = _c_abi(case, 1.0, 0.0, window=win)
    assert R.accepts(g, ref, case[1], K)
    win[tap] = float(np.float32(win[tap] * factor))
    _, g = _c_abi(case, 1.0, 0.0, window=win)
    glob, worst, _ = R.gradient_ratios(g, ref, case[1])
    print(f"wrong window | {SC.case_id(case)} | tap {tap} | {glob:.1f} | {worst:.1f} |")
    assert not R.accepts(g, ref, case[1], K), (glob, worst)


# ---- the loss head on the same images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint", [False, True], ids=["all-tiles", "tile-hint"])
@pytest.mark.parametrize("case", SC.HEAD_CASES, ids=SC.case_id)
def test_loss_head_equals_the_stand_alone_kernels(case, hint):
    """hgs_loss_head_* run the same two kernels with a device-resident target, zero-block flags and work lists: dL/dimage is
    bit for bit the stand-alone gradient at the head's weights, so the float64 bars above hold for the path training uses.
    With a tile hint: on the blocks somebody reads; the others are left alone."""
    from hgs_runtime.fused import ssim_l1
    from tests import gpu_util as G
    img, tgt = (_dev(t) for t in SC.pair(*case))
    _, H, W = case[1]
    gen = torch.Generator(device="cuda").manual_seed(H * 1000 + W)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    aux = G.loss_head_inputs(H, W, rnd)
    tx_n, ty_n = (W + 15) // 16, (H + 15) // 16
    used = torch.ones(ty_n, tx_n, dtype=torch.bool, device="cuda")
    if hint:
        used = rnd(ty_n, tx_n) > 0.5
        used[:, -1] = True
        used[-1, :] = ~used[-1, :]
    head = G.run_loss_head(img, tgt, aux, tile_used=(used.to(torch.int32) * 5).contiguous() if hint else None)
    opt = head["opt"]
    a = img.clone().requires_grad_(True)
    s, l1 = ssim_l1(a, tgt)
    ((1.0 - opt.lambda_dssim) * l1 + opt.lambda_dssim * (1.0 - s)).backward()
    o = head["terms"]
    assert abs(o["l1"] - float(l1)) <= 1e-6 * max(float(l1), 1e-6)
    assert abs(o["dssim"] - float(1.0 - s)) <= 2e-6
    bu = torch.nn.functional.max_pool2d(torch.nn.functional.pad(used.float(), (0, tx_n % 2, 0, ty_n % 2))[None, None], 2)[0, 0] > 0
    px_used = bu.repeat_interleave(32, dim=0).repeat_interleave(32, dim=1)[:H, :W]
    d = head["d_image"]
    assert torch.equal(d[:, px_used], a.grad[:, px_used])
    assert bool((d[:, ~px_used] == 7.0).all())
    if not hint:
        assert torch.equal(d, a.grad)
    # the work and skip lists partition the blocks that are read; skipped blocks carry no gradient
    work, skipped = head["work"].tolist(), head["skipped"].tolist()
    nby, nbx = (H + 31) // 32, (W + 31) // 32
    read = sorted(c * nby * nbx + int(b) for c in range(3) for b in torch.nonzero(bu.reshape(-1)).reshape(-1))
    assert sorted(work + skipped) == read and work == sorted(work)
    gb = torch.nn.functional.max_pool2d(torch.nn.functional.pad((a.grad != 0).float(), (0, (-W) % 32, 0, (-H) % 32))[None], 32)[0]
    assert not gb.reshape(-1)[head["skipped"].long()].any()
    if case[0] == "impulse" and not hint:          # two channels are black altogether
        assert skipped and work
