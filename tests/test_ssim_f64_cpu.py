"""The float64 reference of the SSIM / L1 kernels, and the conditions that keep the bar built on it honest (no GPU).

tests/test_ssim_f64_gpu.py holds the HIP kernels to `K * max(e_ref, 4 ulp * scale)` of the float64 gradient, where e_ref is
the fp32 torch reference's own distance from float64 on the same pair.  That bar is only as good as three things shown here:
the float64 run is the reference's function (it agrees with the reference's recorded fp32 run on the pinned inputs), e_ref
stays small (caps per family: the bar never opens wider than K * 1e-3 of scale, K * 1e-5 on the sharp families), and every
family of tests/ssim_cases.py has the property it is listed for.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ssim_cases as SC
from tests import ssim_reference as R
from tests import test_ref_loss_pins as P

C2 = 0.03 ** 2

# e_ref <= cap * scale.  Measured (CPU, fp32 torch against float64, worst case of the family over its listed shapes):
SHARP = {"noise": 2.8e-6, "binary": 3.0e-6, "hair_black_bg": 4.3e-7, "render_black": 4.2e-7, "impulse": 2.1e-7}     # cap 1e-5
SOFT = {"smooth": 1.9e-4, "flat_bright": 5.7e-4}                                                                       # cap 1e-3
# `identical` has no cap of this form: its float64 gradient is what is left of a cancelling sum (scale ~1e-19, asserted
# below), while an fp32 run leaves the rounding of the sum's TERMS (~5e8 times that).  Its e_ref is capped against the scale
# of those terms -- the gradient of the same image against a target 10 % darker -- at the sharp families' 1e-5 (measured 3e-6).


def _cap(family):
    return 1e-5 if family in SHARP else 1e-3


@pytest.mark.parametrize("ci", range(len(P.SSIM_CASES)))
def test_float64_run_agrees_with_the_recorded_reference_run(ci):
    """The five pinned pairs of ref_loss_pins.npz (drawn as test_ref_loss_pins.py draws them): mean SSIM to 1e-6, d_ssim to
    1e-5 of its scale (measured: 3e-8 and 2.7e-6)."""
    img, gt = P._ssim_inputs(ci)
    ref = R.reference(img, gt)
    k = f"ssim{ci}_"
    assert abs(ref.S64 - float(P.PINS[k + "ssim"])) <= 1e-6
    want = P.PINS[k + "d_ssim"].astype(np.float64)
    assert np.abs(ref.g64 - want).max() <= 1e-5 * np.abs(want).max()
    assert abs(ref.L64 - float(P.PINS[k + "l1"])) <= 1e-6 * float(P.PINS[k + "l1"])


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_fp32_reference_stays_within_its_cap(case):
    family, shape = case
    ref = R.case_reference(case)
    assert np.isfinite(ref.g64).all() and np.isfinite(ref.g32).all()
    if family == "identical":
        img = SC.pair(*case)[0]
        terms = R.reference(img, (0.9 * img).astype(np.float32)).scale
        assert ref.e_ref <= 1e-5 * terms, (ref.e_ref, terms)
        return
    assert family in SHARP or family in SOFT
    assert ref.e_ref <= _cap(family) * ref.scale, (ref.e_ref / ref.scale, _cap(family))


def test_every_family_is_listed_and_every_pair_is_an_image():
    assert set(SHARP) | set(SOFT) | {"identical"} == set(SC.FAMILIES)
    for case in SC.CASES + SC.HEAD_CASES:
        a, b = SC.pair(*case)
        for t in (a, b):
            assert t.dtype == np.float32 and t.shape == case[1] and t.min() >= 0.0 and t.max() <= 1.0


def _window_variance(img):
    """Variance of the image under the 11 x 11 window at every pixel, in float64, over the taps that lie inside the image
    (the zero padding is the frame's property, not the family's)."""
    from loss.losses import create_window
    x = torch.tensor(img, dtype=torch.float64)[None]
    C = x.shape[1]
    w = create_window(11, C).double()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=C)
    mass = conv(torch.ones_like(x))
    mu = conv(x) / mass
    return (conv(x * x) / mass - mu * mu).numpy()[0]


@pytest.mark.parametrize("case", [c for c in SC.CASES if c[0] in ("smooth", "flat_bright")], ids=SC.case_id)
def test_smooth_families_sit_where_the_variance_cancels(case):
    """Median window variance below C2 = 9e-4: E[x^2] - mu^2 loses its leading digits in fp32."""
    assert np.median(_window_variance(SC.pair(*case)[0])) < C2


@pytest.mark.parametrize("case", [c for c in SC.CASES + SC.HEAD_CASES if c[0] in ("hair_black_bg", "render_black")], ids=SC.case_id)
def test_black_background_families_have_zero_and_non_zero_blocks(case):
    family, shape = case
    a, b = SC.pair(*case)
    g = R.case_reference(case).g64
    zero = [blk for blk in SC.blocks(shape) if not g[blk[0], blk[1]:blk[2], blk[3]:blk[4]].any()]
    assert zero and len(zero) < SC.num_blocks(shape)
    C, H, W = shape
    for c, y0, y1, x0, x1 in zero:       # a zero block is zero for a reason: both images are black as far as the gradient reaches
        sl = (c, slice(max(y0 - SC.REACH, 0), y1 + SC.REACH), slice(max(x0 - SC.REACH, 0), x1 + SC.REACH))
        assert not a[sl].any() and not b[sl].any()
    if family == "render_black":
        assert not a.any() and b.any()
    else:
        assert a.any() and not b[:, :, 0].any() and np.abs(b[:, :, 1:] - 0.95 * a[:, :, :-1].astype(np.float64)).max() < 1e-7


@pytest.mark.parametrize("case", [c for c in SC.CASES + SC.HEAD_CASES if c[0] == "identical"], ids=SC.case_id)
def test_identical_images_leave_no_gradient_in_float64(case):
    ref = R.case_reference(case)
    assert ref.scale < 1e-15 and abs(ref.S64 - 1.0) < 1e-15 and ref.L64 == 0.0
    # every block's yardstick is a rounding remainder, not an exact cancellation (the reason (3, 1, 1) is not listed): the
    # float64 gradient is non-zero around every block and the fp32 reference is off in every block
    for _, e_blk, s_blk in R.block_yardsticks(ref, case[1]):
        assert e_blk > 0.0 and s_blk > 0.0


@pytest.mark.parametrize("case", [c for c in SC.CASES + SC.HEAD_CASES if c[0] == "impulse"], ids=SC.case_id)
def test_impulse_gradient_is_the_window_footprint(case):
    """Non-zero exactly within REACH px of the pixel, in its channel only."""
    family, (C, H, W) = case
    g = R.case_reference(case).g64
    want = np.zeros((C, H, W), bool)
    want[C - 1, max(H - 1 - SC.REACH, 0):, max(W - 1 - SC.REACH, 0):] = True
    assert np.array_equal(g != 0, want)


@pytest.mark.parametrize("case", [c for c in SC.CASES if c[0] == "binary"], ids=SC.case_id)
def test_binary_images_are_anticorrelated(case):
    a, b = SC.pair(*case)
    assert set(np.unique(a)) <= {0.0, 1.0} and np.array_equal(b, 1 - a)
    if min(case[1][1:]) >= 33:
        assert R.case_reference(case).S64 < -0.8


# ---- the comparator itself, without a GPU: fp32 torch with a wrong window stands in for a wrong kernel ----------------------------------
def _fp32_gradient_with_window(case, tap, factor, monkeypatch):
    from loss import losses as Ls
    w1 = Ls.gaussian(11, 1.5).float().clone()
    w1[tap] *= factor
    C = case[1][0]
    w2 = (w1[:, None] @ w1[None, :])[None, None].expand(C, 1, 11, 11).contiguous()
    monkeypatch.setattr(Ls, "_window", lambda size, channel, like: w2.to(like.dtype))
    a, b = SC.pair(*case)
    return R._run(a, b, torch.float32)[2]


@pytest.mark.parametrize("tap,factor", [(0, 1.02), (5, 1.0 + 1e-4)])
@pytest.mark.parametrize("case", SC.PERTURBED, ids=SC.case_id)
def test_the_bar_rejects_a_wrong_window_and_accepts_the_reference(case, tap, factor, monkeypatch):
    """Comparator a at the largest K the GPU test may use (8): the fp32 reference passes (ratio <= 1 by construction); the
    same statements with one window tap off -- the outermost by 2 %, the centre by 1e-4 -- do not."""
    ref = R.case_reference(case)
    assert R.accepts(ref.g32, ref, case[1], 1.0)
    wrong = _fp32_gradient_with_window(case, tap, factor, monkeypatch)
    glob, worst, _ = R.gradient_ratios(wrong, ref, case[1])
    print(SC.case_id(case), tap, "global %.1f worst block %.1f" % (glob, worst))
    assert not R.accepts(wrong, ref, case[1], 8.0), (glob, worst)
    assert max(glob, worst) > 32, (glob, worst)                   # not a near miss: four times the largest K
