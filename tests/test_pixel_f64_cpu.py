"""The float64 reference of the per-pixel loss terms, and the conditions that keep the bars built on it honest (no GPU).

tests/test_pixel_f64_gpu.py holds the three HIP forms of the orientation gradient to `K * max(e_ref, 4 * 2^-23)` per pixel
(tests/pixel_reference.py: rho_i, kappa_i, fragile pixels) and the mask term to the same form at its natural scale 1.  Shown
here: e_ref stays small in every class, fragile pixels are few and the fp32 statement never takes the other side of a kink
outside them, every class of tests/pixel_cases.py has the property it is listed for, the comparator rejects six subtly wrong
statements, and the statement is `loss/losses.py`'s own, bit for bit in fp32.
"""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixel_cases as PC
from tests import pixel_reference as R

E_REF_CAP = 2e-6
FRAGILE_CAP = {"head_on": 0.10}        # every other class: 1 % of the masked pixels


@pytest.mark.parametrize("case", PC.DIRECTION_CASES, ids=PC.case_id)
def test_fp32_statement_stays_within_its_cap_and_off_the_kinks(case):
    """e_ref <= 2e-6; fragile pixels <= 1 % of the masked ones (10 % in `head_on`); outside them the fp32 statement shows
    no sign disagreement with float64.  Measured at 67 x 131: e_ref 8e-8 (`head_on`) .. 3.3e-7, fragile share 0 except
    `head_on` 1.7 %, `kinks` 0.03 %; 4.3e-7 at 725 x 725."""
    ref = R.orientation_case_reference(case)
    print(f"yardstick | {PC.case_id(case)} | count {ref.count} | e_ref {ref.e_ref:.2e} | fragile {ref.fragile_share:.4f} | flips {ref.sign_flips} |")
    assert np.isfinite(ref.g64).all() and np.isfinite(ref.g32).all()
    assert ref.e_ref <= E_REF_CAP
    assert ref.fragile_share <= FRAGILE_CAP.get(case[0], 0.01)
    assert ref.sign_flips == 0
    # no masked pixel with a confidence has a float64 gradient of exactly 0 (the comparator divides by its norm), and the fp32
    # statement passes its own comparator with K = 1 by construction
    assert not (ref.live & (R._norm3(ref.g64) == 0)).any()
    assert R.accepts_direction(ref.g32, ref, 1.0)
    assert R.value_ok(ref.v32, ref, K=1.0, T=0.0)
    assert not ref.g64[:, ~ref.mask].any() and not ref.g64[:, ref.mask & (ref.conf == 0)].any()


@pytest.mark.parametrize("case", PC.LOGIT_CASES, ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}")
def test_fp32_mask_term_stays_within_its_cap(case):
    """sigmoid(x) - y at scale 1: e_ref <= 2e-6 (measured 1.3e-8 .. 1.2e-7)."""
    ref = R.bce_case_reference(case)
    assert np.isfinite(ref.g64).all() and ref.e_ref <= E_REF_CAP
    assert R.bce_report(ref.g32, ref, 1.0) <= 1.0 and R.bce_value_ok(ref.b32, ref, K=1.0)


# ---- every class has the property it is listed for ---------------------------------------------------------------------------------
def test_inputs_are_what_the_kernels_expect():
    for case in PC.DIRECTION_CASES:
        d = PC.direction_case(*case)
        H, W = case[1]
        assert d.omap.shape == (3, H, W) and d.omap.dtype == np.float32
        assert d.gt.dtype == np.float32 and d.gt.min() >= 0 and float(d.gt.max()) < np.pi
        assert d.conf.dtype == np.float32 and d.conf.min() == 0 and d.conf.max() < 1
        if d.mask is not None:
            assert d.mask.dtype == np.uint8 and set(np.unique(d.mask)) <= {0, 1}
            if case[2] == "m70":
                assert 0.6 < d.mask.mean() < 0.8 or H * W < 100
            assert (d.conf[d.mask != 0] == 0).any() or case[2] != "m70" or H * W < 100
    assert int(PC.direction_case("unit", PC.MAIN, "one").mask.sum()) == 1
    assert int(PC.direction_case("unit", PC.MAIN, "empty").mask.sum()) == 0


def _view_xy(d):
    p = PC.view_plane(d.omap.reshape(3, -1).T)
    return p[:, 0], p[:, 1], np.hypot(p[:, 0], p[:, 1])


def test_direction_classes_have_their_properties():
    m = lambda d: d.mask.reshape(-1) != 0
    d = PC.direction_case("faint", PC.MAIN)
    _, _, r = _view_xy(d)
    assert (r[m(d)] < 1e-8).any() and ((r[m(d)] > 3e-7) & (r[m(d)] < 3e-6)).any() and (r[m(d)] > 1e-4).any()
    d = PC.direction_case("zero_in_mask", PC.MAIN)
    _, _, r = _view_xy(d)
    assert 0.15 < (r == 0).mean() < 0.25 and (r[m(d)] == 0).sum() > 100
    d = PC.direction_case("head_on", PC.MAIN)
    ref = R.orientation_case_reference(("head_on", PC.MAIN, "m70"))
    assert np.median(ref.kappa) > 30 and ref.kappa.max() > 1e3
    d = PC.direction_case("wrap", PC.MAIN)
    x, y, _ = _view_xy(d)
    assert np.abs(x).max() < 2e-3 and np.abs(y).min() > 0.1
    for sx in (-1, 1):
        for sy in (-1, 1):
            assert ((np.sign(x) == sx) & (np.sign(y) == sy) & m(d)).sum() > 500
    th = PC.theta64(d.omap.reshape(3, -1).T)
    assert (th < 1e-2).sum() > 1000 and (th > np.pi - 1e-2).sum() > 1000 and ((th > 1e-2) & (th < np.pi - 1e-2)).sum() == 0
    ref = R.orientation_case_reference(("kinks", PC.MAIN, "m70"))
    ae = np.abs(ref.e64)
    near = np.minimum(np.minimum(ae, np.abs(ae - np.pi)), np.abs(ae - R.HALF_PI))     # |e| = pi is e = 0 seen across the wrap
    assert near[ref.mask].max() < 0.11 and near[ref.mask].min() > 5e-5
    for lo, hi in ((0.0, 0.2), (R.HALF_PI - 0.2, R.HALF_PI), (R.HALF_PI, R.HALF_PI + 0.2)):
        assert ((ae > lo) & (ae < hi) & ref.live).sum() > 500


@pytest.mark.parametrize("variant", ["none_black", "none_colour"])
def test_maskless_variants_hold_background_pixels_of_every_kind(variant):
    d = PC.direction_case("unit", PC.MAIN, variant)
    o = d.omap.reshape(3, -1).T
    bg = np.asarray(d.bg, dtype=np.float32)
    differs = (o != bg).sum(axis=1)
    assert (differs == 0).sum() > 500 and (differs == 1).sum() > 100 and (differs == 3).sum() > 5000
    assert (np.signbit(o) & (o == 0)).any()                      # -0.0
    ref = R.orientation_case_reference(("unit", PC.MAIN, variant))
    assert np.array_equal(ref.mask.reshape(-1), differs > 0)
    if variant == "none_colour":
        assert (ref.r[ref.mask] == 0).any()                      # (0, -0, 0) differs from bg: masked, r = 0


def test_logit_classes_have_their_properties():
    x, y = PC.logit_case("confident", PC.MAIN)
    assert np.abs(x).min() >= 5 and np.array_equal(x > 0, y == 1)
    x, y = PC.logit_case("confident_wrong", PC.MAIN)
    assert np.abs(x).min() >= 5 and np.array_equal(x > 0, y == 0)
    x, y = PC.logit_case("extreme", PC.MAIN)
    assert ((x == 0) & ~np.signbit(x)).any() and ((x == 0) & np.signbit(x)).any() and np.abs(x[x != 0]).min() >= 60 and np.abs(x).max() <= 120
    x, y = PC.logit_case("soft_target", PC.MAIN)
    assert ((y > 0) & (y < 1)).mean() > 0.5 and (y == 0).any() and (y == 1).any()
    x, y = PC.logit_case("cancel", PC.MAIN)
    assert np.abs(R.bce_case_reference(("cancel", PC.MAIN)).g64).max() <= 2.0 ** -24


# ---- the comparator itself: subtly wrong fp32 statements stand in for a wrong kernel ---------------------------------------------------
@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_the_comparator_rejects_a_wrong_statement(mutant):
    """At the K the GPU file uses.  Measured, in yardsticks: no +pi wrap, the kink's sign and the transposed view matrix
    ~4e6 (a flipped pixel has rho = 2); the shift dropped 2.1e3; 1 / r at r = 0 gives NaN; the gradient through the norm
    dropped 2.2 -- theta does not depend on the common divisor of x and y, so that term is what the 1e-6 shift of y leaves,
    at most 1e-6 |x| of the pixel's gradient: the bar sees it only while K stays at or below 2."""
    case = (R.MUTANTS[mutant], PC.MAIN, "m70")
    ref = R.orientation_case_reference(case)
    assert R.accepts_direction(ref.g32, ref, 1.0)
    g = R.run_orientation(case, torch.float32, mutant)[1]
    worst, problems = R.direction_report(g, ref)
    print(f"mutant | {mutant} | {case[0]} | {worst:.3g} | {problems} |")
    assert not R.accepts_direction(g, ref, R.K_ORI), (worst, problems)


def test_the_bce_bar_sees_a_shifted_logit():
    """sigmoid(x + 1e-5) on `cancel`: 2.5e-6 at x = 0, five yardsticks."""
    ref = R.bce_case_reference(("cancel", PC.MAIN))
    x, y = PC.logit_case("cancel", PC.MAIN)
    g = R._run_bce(x + np.float32(1e-5), y, torch.float32)[1]
    assert R.bce_report(g, ref, 1.0) > R.K_BCE


# ---- the statement is the product's --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.DIRECTION_CASES, ids=PC.case_id)
def test_the_statement_is_the_products_restatement_bit_for_bit(case, monkeypatch):
    """loss/losses.py::_orientation_term with fused_losses = False on the same fp32 tensors: value and gradient bits."""
    from loss import losses as Ls
    monkeypatch.setattr(Ls, "fused_losses", False)
    d = PC.direction_case(*case)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    omap = t(d.omap).requires_grad_(True)
    cam = types.SimpleNamespace(world_view_transform=t(PC.VIEW), orientation_field=t(d.gt), orientation_confidence=t(d.conf),
                                mask=None if d.mask is None else torch.tensor(d.mask != 0))
    with R._one_thread():
        v = Ls._orientation_term(omap, types.SimpleNamespace(min_val=PC.MIN_VAL), cam, t(np.asarray(d.bg, dtype=np.float32)))
        g, = torch.autograd.grad(v, omap)
    v32, g32 = R.run_orientation(case, torch.float32)[:2]
    assert np.array_equal(np.float32(v.item()).view(np.uint32), np.float32(v32).view(np.uint32)) or (np.isnan(v.item()) and np.isnan(v32))
    assert np.array_equal(g.numpy().view(np.uint32), g32.astype(np.float32).view(np.uint32))


def test_the_mask_statement_is_the_products():
    """loss/losses.py calls F.binary_cross_entropy_with_logits on (mask_img, float_mask): so does the reference module."""
    x, y = PC.logit_case("logit_mixed", PC.MAIN)
    b = F.binary_cross_entropy_with_logits(torch.tensor(x), torch.tensor(y))
    assert float(b) == R.bce_case_reference(("logit_mixed", PC.MAIN)).b32
