"""The three HIP forms of the per-pixel loss terms against their float64 statement on the inputs of tests/pixel_cases.py:
  a. hgs_orientation_loss_* (stand-alone pair, `hgs_runtime.fused.orientation_loss`): ori_fwd_kernel / ori_bwd_kernel;
  b. hgs_loss_head_forward + _backward (two passes): pix_fwd_kernel, the tail of hgs_head_tail.h, pix_bwd_kernel;
  c. hgs_loss_head_forward with d_extra_unit (one pass, what training runs), d. the same with a tile hint.
The direction gradient is graded per pixel (tests/pixel_reference.py: rho_i <= K * max(e_ref, 4 * 2^-23), kappa_i, fragile
pixels), the mask term's gradient at its natural scale 1, the values against `max(K |v32 - v64|, T)`; tests/test_pixel_f64_cpu.py
caps the yardsticks.  e: the same kernels fail the comparator when an ABI argument is subtly wrong.  f: the mask count of a
view whose mask holds {0, 255}.  Every output plane and partial sum starts as NaN (or as FILL where "left alone" is graded).
Each test prints its row before it asserts (`pytest -s`): form, case, e_ref, worst ratio in yardsticks, fragile share.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import pixel_cases as PC
from tests import pixel_reference as R

pytestmark = pytest.mark.gpu

K_ORI, K_BCE, T_O = R.K_ORI, R.K_BCE, R.T_O
UP = float(np.float32(0.37))
FILL = 7.0
NAN = float("nan")


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _full(shape, value=NAN):
    return torch.full(shape, value, dtype=torch.float32, device="cuda")


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _refs(case):
    cls, logit, frame, mask = case
    return R.orientation_case_reference((cls, frame, mask)), R.bce_case_reference((logit, frame))


# ---- a. the stand-alone pair --------------------------------------------------------------------------------------------------------
def _stand_alone(case, min_val=PC.MIN_VAL, view=PC.VIEW, conf_factor=None):
    """(value, count, gradient [3, H, W]) of `orientation_loss` through autograd, and the same through the C ABI with the
    partial sums and the gradient planes pre-filled with NaN: count from the partials, the two gradients bit-equal."""
    import hgs_runtime as rt
    from hgs_runtime.fused import orientation_loss
    d = PC.direction_case(*case)
    H, W = case[1]
    omap = _dev(d.omap).requires_grad_(True)
    gt, conf, vm = _dev(d.gt), _dev(d.conf), _dev(view)
    if conf_factor is not None:
        conf = conf * conf_factor
    mask = None if d.mask is None else _dev(d.mask)
    v = orientation_loss(omap, vm, list(d.bg), min_val, gt, conf, mask)
    g, = torch.autograd.grad(v, omap)
    L = rt.lib()
    nb = L.hgs_orientation_loss_num_blocks(H, W)
    partials, d_omap = _full((nb, 2)), _full((3, H, W))
    bg3 = (C.c_float * 3)(*d.bg)
    one = torch.ones(1, device="cuda")
    rt.check(L.hgs_orientation_loss_forward(rt.current_stream(), H, W, omap.data_ptr(), vm.data_ptr(), bg3, float(min_val),
                                            gt.data_ptr(), conf.data_ptr(), None if mask is None else mask.data_ptr(),
                                            partials.data_ptr()))
    sums = partials.sum(dim=0)
    count = sums[1:2].contiguous()
    rt.check(L.hgs_orientation_loss_backward(rt.current_stream(), H, W, omap.data_ptr(), vm.data_ptr(), bg3, float(min_val),
                                             gt.data_ptr(), conf.data_ptr(), None if mask is None else mask.data_ptr(),
                                             one.data_ptr(), count.data_ptr(), d_omap.data_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(partials).all())
    assert _bits_equal(d_omap, g)
    value = float(v.detach())
    assert value == float(sums[0] / sums[1]) or (np.isnan(value) and float(sums[1]) == 0.0)
    return value, float(count), g.cpu().numpy()


@pytest.mark.parametrize("case", PC.DIRECTION_CASES, ids=PC.case_id)
def test_stand_alone_pair_against_float64(case):
    """a. With a mask, without one (black and coloured background), one masked pixel, none: value, count, gradient; exactly 0
    outside the mask; an empty mask gives NaN and a gradient of zeros."""
    ref = R.orientation_case_reference(case)
    v, count, g = _stand_alone(case)
    worst, problems = R.direction_report(g, ref)
    print(f"row | a | {PC.case_id(case)} | {ref.e_ref:.2e} | {worst:.2f} | {ref.fragile_share:.4f} | value {abs(v - ref.v64) / max(ref.term_scale, 1e-300):.1e} |")
    assert count == ref.count
    assert R.value_ok(v, ref, K_ORI, T_O), (v, ref.v64, ref.v32)
    if ref.count == 0:
        assert np.isnan(v) and not g.any()
    assert not problems and worst <= K_ORI, (worst, problems)


# ---- b, c, d. the loss head ------------------------------------------------------------------------------------------------------------
def _head(case, defer_tail=0, one_pass=False, tile_used=None, upstreams=(), min_val=PC.MIN_VAL, view=PC.VIEW, conf_factor=None,
          logit_shift=None, inputs=None, targets=None):
    """hgs_loss_head_forward (+ one _backward per upstream gradient) on a device-resident target row built from the case.
    one_pass: with d_extra_unit [4, H, W], pre-filled with FILL when a tile hint is given and with NaN otherwise.  `inputs`:
    device tensors in place of the case's arrays (the huge frames); `targets`: a device-resident row in place of the one built
    here (a ViewTable's)."""
    import hgs_runtime as rt
    from arguments import OptimizationParams
    from hgs_runtime.strand_step import head_params
    if inputs is None:
        cls, logit, (H, W), mv = case
        d = PC.direction_case(cls, (H, W), mv)
        x, y = PC.logit_case(logit, (H, W))
        rng = np.random.default_rng([H, W, 11])
        a = rng.uniform(0, 1, (3, H, W))
        inputs = dict(image=_dev(a.astype(np.float32)), gt_image=_dev(np.clip(a + rng.normal(0, 0.1, a.shape), 0, 1).astype(np.float32)),
                      mask_img=_dev(x), float_mask=_dev(y), omap=_dev(d.omap), orientation=_dev(d.gt), confidence=_dev(d.conf),
                      mask=_dev(d.mask))
    t = types.SimpleNamespace(**inputs)
    H, W = t.mask.shape
    if conf_factor is not None:
        t.confidence = t.confidence * conf_factor
    if logit_shift is not None:
        t.mask_img = t.mask_img + logit_shift
    row = rt.ViewTargets()
    row.image, row.float_mask, row.orientation, row.confidence, row.mask = (
        u.data_ptr() for u in (t.gt_image, t.float_mask, t.orientation, t.confidence, t.mask))
    for k, v in enumerate(np.asarray(view, dtype=np.float32).reshape(-1)):
        row.viewmatrix[k] = float(v)
    for k, v in enumerate(np.eye(4, dtype=np.float32).reshape(-1)):
        row.projmatrix[k] = float(v)
    row.mask_count = float(torch.count_nonzero(t.mask).item())
    if targets is None:
        targets = torch.from_numpy(np.frombuffer(bytes(row), dtype=np.uint8).copy()).cuda()
    hp = head_params(H, W, OptimizationParams(), 0, 0, min_val, True)
    hp.defer_tail = int(defer_tail)
    if tile_used is not None:
        assert tile_used.data_ptr() % 16 == 0
        hp.tile_used, hp.tiles_x, hp.tiles_y = tile_used.data_ptr(), tile_used.shape[1], tile_used.shape[0]
    L = rt.lib()
    scratch = _full((L.hgs_loss_head_scratch_floats(C.byref(hp)),))
    out = _full((rt.HEAD_NOUT,))
    d_unit = _full((4, H, W), FILL if tile_used is not None else NAN) if one_pass else None
    rt.check(L.hgs_loss_head_forward(rt.current_stream(), C.byref(hp), t.image.data_ptr(), t.mask_img.data_ptr(), t.omap.data_ptr(),
                                     targets.data_ptr(), None, None, scratch.data_ptr(), out.data_ptr(),
                                     None if d_unit is None else d_unit.data_ptr(), None))
    grads = {}
    for up in upstreams:
        go = torch.full((1,), up, dtype=torch.float32, device="cuda")
        d_img, d_mask, d_omap = _full((3, H, W)), _full((H, W)), _full((3, H, W))
        rt.check(L.hgs_loss_head_backward(rt.current_stream(), C.byref(hp), t.image.data_ptr(), t.mask_img.data_ptr(),
                                          t.omap.data_ptr(), targets.data_ptr(), None, None, scratch.data_ptr(), out.data_ptr(),
                                          go.data_ptr(), 0, d_img.data_ptr(), d_mask.data_ptr(), d_omap.data_ptr(), None))
        grads[up] = (d_img, d_mask, d_omap)
    torch.cuda.synchronize()
    return types.SimpleNamespace(out=out, terms=dict(zip(rt.HEAD_OUT, out.tolist())), grads=grads, d_unit=d_unit, N=H * W,
                                 l_mask=float(hp.lambda_mask), l_ori=float(hp.lambda_orientation), inputs=inputs)


def _grade_terms(form, case, head):
    """The orientation term, its count and the total (the mean of the mask term has a test of its own below)."""
    oref, bref = _refs(case)
    o = head.terms
    print(f"row | {form} | {PC.case_id(case)} | orientation {abs(o['orientation'] - oref.v64) / max(oref.term_scale, 1e-300):.1e} of its scale | "
          f"mask {abs(o['mask'] - bref.b64):.1e} (fp32 {abs(bref.b32 - bref.b64):.1e}) |")
    assert o["ori_count"] == oref.count
    assert R.value_ok(o["orientation"], oref, K_ORI, T_O), (o["orientation"], oref.v64, oref.v32)
    want = R.head_total(o["total_fwd"], head.l_mask, bref.b64, head.l_ori, oref.v64)
    if oref.count == 0:
        assert np.isnan(o["total"]) and np.isnan(o["orientation"])
    else:
        assert np.isfinite(o["total_fwd"]) and abs(o["total"] - want) <= 2e-6 * abs(want), (o["total"], want)


def _grade_gradients(form, case, d_mask, d_omap, up, K_ori=K_ORI, K_bce=K_BCE):
    """(worst direction ratio, problems, worst mask-term ratio); asserts unless a K is None."""
    oref, bref = _refs(case)
    N = case[2][0] * case[2][1]
    l_mask, l_ori = float(np.float32(0.01)), 100.0
    wb = R.bce_report(d_mask.cpu().numpy(), bref, l_mask * up / N)
    wo, problems = R.direction_report(d_omap.cpu().numpy(), oref, l_ori * up)
    print(f"row | {form} | {PC.case_id(case)} | {oref.e_ref:.2e} | {wo:.2f} | {oref.fragile_share:.4f} | mask term {bref.e_ref:.2e} | {wb:.2f} |")
    if K_ori is not None:
        assert not problems and wo <= K_ori, (wo, problems)
    if K_bce is not None:
        assert wb <= K_bce, wb
    return wo, problems, wb


@pytest.mark.parametrize("case", PC.HEAD_CASES, ids=PC.case_id)
def test_two_pass_head_against_float64(case):
    """b. d_extra_unit = NULL, then the backward with an upstream gradient of 0.37: the terms, the count, the total, d_mask and
    d_omap; with the tail deferred to the backward the same bits."""
    runs = [_head(case, defer_tail=dt, upstreams=(UP,)) for dt in (0, 1)]
    assert runs[0].l_mask == float(np.float32(0.01)) and runs[0].l_ori == 100.0
    _grade_terms("b", case, runs[0])
    _, d_mask, d_omap = runs[0].grads[UP]
    _grade_gradients("b", case, d_mask, d_omap, UP)
    assert _bits_equal(runs[0].out, runs[1].out)
    for p, q in zip(runs[0].grads[UP], runs[1].grads[UP]):
        assert _bits_equal(p, q)


@pytest.mark.parametrize("case", PC.HEAD_CASES, ids=PC.case_id)
def test_mask_term_mean_against_float64(case):
    """b, c. out["mask"], the same bits from both forms of the forward: |b - b64| <= max(K |b32 - b64|, 1e-7).

    The bar is absolute, and two classes have means (17.4, 42.7) of which one fp32 ulp is 1.9e-6 and 3.8e-6: only the
    correctly rounded fp32 mean passes there.  With an fp32 sum of the block sums and the product with fp32(1 / HW) the head
    returned its fp32 neighbour (|b - b64| = 1.4e-6 and 4.0e-6); the tail now sums the mask term's partials in float64 and
    divides by H * W, one rounding.  What the fp32 block sums leave is 3e-9 and 7e-9 of the mean there (emulated on the CPU),
    a sixth of the distance to the nearest rounding boundary."""
    _, bref = _refs(case)
    two, one = _head(case), _head(case, one_pass=True)
    b = two.terms["mask"]
    print(f"row | mask mean | {PC.case_id(case)} | {bref.b64:.6g} | {abs(b - bref.b64):.1e} | fp32 {abs(bref.b32 - bref.b64):.1e} |")
    assert _bits_equal(two.out, one.out)
    assert R.bce_value_ok(b, bref, K_BCE), (b, bref.b64, bref.b32)


def _one_pass_against_two_pass(case, one, two):
    """Per pixel, the one-pass planes within K yardsticks of the two-pass gradient at upstream 1 (same angle, same side of
    every kink: no pixel is fragile between the two)."""
    oref, bref = _refs(case)
    _, d_mask, d_omap = two.grads[1.0]
    gm = (one.d_unit[0].double() - d_mask.double()).abs().max().item() / (one.l_mask / one.N) / bref.yard
    diff = R._norm3((one.d_unit[1:4].double() - d_omap.double()).cpu().numpy())
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.where(oref.live, diff / (oref.kappa * R._norm3(oref.g64 * one.l_ori)), 0.0)
    go = float(rho.max()) / oref.yard
    print(f"row | c vs b | {PC.case_id(case)} | direction {go:.2f} | mask term {gm:.2f} |")
    assert go <= K_ORI and gm <= K_BCE, (go, gm)


@pytest.mark.parametrize("case", PC.HEAD_CASES, ids=PC.case_id)
def test_one_pass_head_against_float64(case):
    """c. The forward writes the four gradient planes for an upstream gradient of 1, normalised by the row's mask count."""
    one = _head(case, one_pass=True)
    _grade_terms("c", case, one)
    assert bool(torch.isfinite(one.d_unit).all())
    _grade_gradients("c", case, one.d_unit[0], one.d_unit[1:4], 1.0)
    _one_pass_against_two_pass(case, one, _head(case, upstreams=(1.0,)))


def _tile_hint(H, W, seed):
    """Random uint32 hint [tiles_y, tiles_x] (16-byte aligned) with the last tile column set and the last tile row inverted,
    and the same expanded to pixels."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    gen = torch.Generator(device="cuda").manual_seed(seed)
    used = torch.rand(ty, tx, device="cuda", generator=gen) > 0.5
    used[:, -1] = True
    used[-1, :] = ~used[-1, :]
    hint = (used.to(torch.int32) * 5).contiguous()          # (the kernels read `!= 0` of 32-bit words)
    px = used.repeat_interleave(16, dim=0).repeat_interleave(16, dim=1)[:H, :W]
    return hint, px


def test_one_pass_head_with_a_tile_hint_writes_the_same_bits_on_used_tiles():
    """d. Pixels of used tiles: bitwise those of c; the others keep the fill."""
    case = ("unit", "logit_mixed", PC.MAIN, "m70")
    H, W = PC.MAIN
    hint, px = _tile_hint(H, W, 5)
    assert bool(px.any()) and bool((~px).any())
    full = _head(case, one_pass=True)
    part = _head(case, one_pass=True, tile_used=hint)
    assert _bits_equal(part.d_unit[:, px], full.d_unit[:, px])
    assert bool((part.d_unit[:, ~px] == FILL).all())
    assert _bits_equal(part.out, full.out)
    _grade_terms("d", case, part)


@pytest.mark.parametrize("frame", PC.HUGE_FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_tile_hint_of_a_frame_around_two_to_the_24_pixels(frame):
    """d. 2^24 - 9 pixels: pixel -> row through the float reciprocal of W, where i + 0.5 is no longer exact above 2^23 and the
    correction step decides; 2^24 + 4090: the integer division.  GPU-drawn inputs, no float64: WHICH pixels were written,
    against the hint expanded with torch ops.  (More SSIM blocks than the list builder takes: the head runs without lists.)"""
    from tests import gpu_util as G
    H, W = frame
    gen = torch.Generator(device="cuda").manual_seed(H * 10000 + W)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    aux = G.loss_head_inputs(H, W, rnd)
    inputs = dict(aux, image=rnd(3, H, W), gt_image=rnd(3, H, W))
    hint, px = _tile_hint(H, W, 6)
    head = _head(None, one_pass=True, tile_used=hint, inputs=inputs)
    written = head.d_unit != FILL
    assert torch.equal(written.all(dim=0), px) and torch.equal(written.any(dim=0), px)
    assert bool(torch.isfinite(head.d_unit).all())
    assert head.terms["ori_count"] == float(torch.count_nonzero(aux["mask"]).item())
    del head, written, inputs, aux
    torch.cuda.empty_cache()


# ---- e. the bar sees a wrong kernel ------------------------------------------------------------------------------------------------------
def _all_forms(case, **wrong):
    """(form, worst direction ratio, problems, worst mask-term ratio) of the three implementations on one head case."""
    cls, logit, frame, mv = case
    res = []
    if "logit_shift" not in wrong:
        _, _, g = _stand_alone((cls, frame, mv), **wrong)
        res.append(("a",) + R.direction_report(g, _refs(case)[0]) + (0.0,))
    two = _head(case, upstreams=(UP,), **wrong)
    res.append(("b",) + _grade_gradients("e/b", case, two.grads[UP][1], two.grads[UP][2], UP, None, None))
    one = _head(case, one_pass=True, **wrong)
    res.append(("c",) + _grade_gradients("e/c", case, one.d_unit[0], one.d_unit[1:4], 1.0, None, None))
    return res


_WRONG = {"min_val": (("faint", "confident", PC.MAIN, "m70"), dict(min_val=2 * PC.MIN_VAL)),
          "view": (("unit", "logit_mixed", PC.MAIN, "m70"), dict(view=np.ascontiguousarray(PC.VIEW.T))),
          "confidence": (("unit", "logit_mixed", PC.MAIN, "m70"), dict(conf_factor=1.0 + 1e-4)),
          "logits": (("kinks", "cancel", PC.MAIN, "m70"), dict(logit_shift=1e-5))}


@pytest.mark.parametrize("what", list(_WRONG))
def test_the_bar_sees_a_wrong_argument(what):
    """e. The constants of the kernels are not ABI arguments, their inputs are: with min_val doubled (`faint`), the view matrix
    transposed or the confidence times 1 + 1e-4 (`unit`), or the logits + 1e-5 (the mask plane of `cancel`), every form must
    FAIL the comparator against the unperturbed float64 reference -- and pass it as it is."""
    case, wrong = _WRONG[what]
    for form, wo, problems, wb in _all_forms(case):
        assert wo <= K_ORI and not problems and wb <= K_BCE, (form, wo, problems, wb)
    for form, wo, problems, wb in _all_forms(case, **wrong):
        print(f"wrong {what} | {form} | direction {wo:.3g} {problems} | mask term {wb:.3g} |")
        if what == "logits":
            assert wb > K_BCE, (form, wb)
        else:
            assert wo > K_ORI or problems, (form, wo)


# ---- f. the mask count of a mask that is not 0 / 1 ---------------------------------------------------------------------------------------
def test_view_table_counts_the_pixels_of_a_0_255_mask():
    """Every kernel tests `mask != 0` and counts 1: the row's mask_count, which normalises the one-pass gradient, is the number
    of non-zero pixels whatever their value -- and the one-pass planes on such a row pass the comparator."""
    import hgs_runtime as rt
    from hgs_runtime.strand_step import ViewTable
    case = ("unit", "logit_mixed", PC.MAIN, "m70")
    H, W = PC.MAIN
    d = PC.direction_case("unit", PC.MAIN)
    x, y = PC.logit_case("logit_mixed", PC.MAIN)
    m255 = _dev(d.mask) * 255
    assert set(torch.unique(m255).tolist()) == {0, 255}
    cam = types.SimpleNamespace(image_height=H, image_width=W, FoVx=0.8, FoVy=0.6, original_image=torch.rand(3, H, W, device="cuda"),
                                orientation_field=_dev(d.gt), orientation_confidence=_dev(d.conf), float_mask=_dev(y), mask=m255,
                                world_view_transform=_dev(PC.VIEW), full_proj_transform=torch.eye(4, device="cuda"),
                                camera_center=torch.zeros(3, device="cuda"))
    vt = ViewTable([cam])
    row = rt.ViewTargets.from_buffer_copy(vt.table[:C.sizeof(rt.ViewTargets)].cpu().numpy().tobytes())
    assert row.mask_count == float(int((d.mask != 0).sum()))
    assert [row.viewmatrix[k] for k in range(16)] == [float(v) for v in PC.VIEW.reshape(-1)]
    inputs = dict(image=cam.original_image * 0.9, gt_image=cam.original_image, mask_img=_dev(x), float_mask=cam.float_mask,
                  omap=_dev(d.omap), orientation=cam.orientation_field, confidence=cam.orientation_confidence, mask=m255)
    one = _head(case, one_pass=True, inputs=inputs, targets=vt.table)      # the table's own row 0
    _grade_gradients("f", case, one.d_unit[0], one.d_unit[1:4], 1.0)
