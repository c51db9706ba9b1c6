"""The float64 reference of the per-view image statistics and the conditions that keep its bars honest (no GPU).

tests/test_view_stats_f64_gpu.py holds csrc/hgs_view_stats.hip to tests/view_stats_reference.py: counts exact, the within-10 /
within-20 counts decided by float64 outside the ambiguous pixels, sse_hair of a one-pixel mask bit for bit, the orientation
sums within `K * yard * kappa_i` per pixel.  Shown here: the yardstick of every class (printed; measured values below), few
ambiguous pixels and no float32 decision against float64 outside them, every new class has the property it is listed for, the
exact planes of the size edges are exact, the comparator rejects nine subtly wrong statements, and the reference is pinned
to loss/losses.py::_orientation_term and to loss/image_metrics.py::_cpu_stats.

Yardsticks `e_ref` = worst |diff32 - diff64| / kappa of the float32 CPU statement, 16 x 16 / 67 x 131 at min_val 1e-6 (1e-7:
2.0e-7 .. 4.2e-7): unit 3.1e-7 / 3.8e-7, faint 3.2e-7 / 3.8e-7, zero_in_mask 3.0e-7 / 4.0e-7, head_on 6.6e-8 / 8.0e-8, wrap
2.9e-7 / 3.2e-7, kinks 2.6e-7 / 3.4e-7, edge10 2.9e-7 / 3.2e-7, edge20 2.7e-7 / 3.0e-7, denormal 2.9e-7 / 3.1e-7, fg_edge
3.5e-7 / 3.7e-7, gt_ends 2.6e-7 / 3.0e-7: all below the floor 4 * 2^-23 = 4.8e-7, which is therefore the yardstick everywhere.
Ambiguous share of the masked pixels: 0 except head_on 1.8 % (3.8 % at 16 x 16) and the edge classes (their m <= 0.5 pixels).
Mutants, in yardsticks on the one-hot views: no wrap 6e6 (whole planes 8e5), view matrix transposed 1e6 (whole planes 2e4), the shift
dropped 1e3 (`faint`; whole planes 14) and 2.05 .. 2.13 (`zero_in_mask`: seen only while K <= 2); the others change a count or sse_hair.

`<` in place of `<=` at the thresholds cannot be shown by any input: near both thresholds the statement's float32 diff is
pi/2 - |a - pi/2| with |a - pi/2| in [1, 2), a multiple of 2^-23, and float32(10 pi / 180) = 1464088.25 * 2^-23 (the 20 degree
one twice that) is none.  The mutant `edge_in_out` is the nearest thing that can be observed: the largest attainable value
below the threshold counted as outside (test_no_float32_diff_equals_a_threshold asserts the lattice).
"""
import math
import types

import numpy as np
import pytest
import torch

from tests import pixel_cases as PC
from tests import view_stats_cases as VC
from tests import view_stats_reference as VR

AMBIGUOUS_CAP = {"head_on": 0.10}            # every other class 1 %; the edge classes hold exactly their m <= 0.5 pixels
CLASS_RUNS = [(c, f, mv) for c in VC.CLASSES for f in (VC.FRAME_A, PC.MAIN) for mv in VC.MIN_VALS]
_run_id = lambda r: f"{r[0]}-{r[1][0]}x{r[1][1]}-{r[2]:.0e}"   # noqa: E731


def test_constants_are_the_products():
    from loss import image_metrics as IM
    assert VC.DELTA == VR.DELTA and VC.T10 == float(IM.TH10) and VC.T20 == float(IM.TH20) and VR.STATS == IM.STATS
    assert VC.MIN_VALS[1] == float(np.float32(IM.MIN_VAL)) and VC.HALF_PI32 == IM._HALF_PI
    for hw in VC.SMALL_SIZES + VC.LARGE_SIZES:
        assert VC.num_blocks(hw) == min(-(-hw // 4096), 1024)


@pytest.mark.parametrize("run", CLASS_RUNS, ids=_run_id)
def test_fp32_statement_decides_as_float64_off_the_ambiguous_pixels(run):
    cls, frame, mv = run
    c = VC.hard_case(cls, frame, mv)
    ref = VR.pixel_reference(c, mv)
    om = c.mask.reshape(-1) != 0
    n = int(om.sum())
    share = max(int((ref.amb10 & om).sum()), int((ref.amb20 & om).sum())) / n
    print(f"yardstick | {_run_id(run)} | count {n} | e_ref {ref.e_ref:.2e} | ambiguous {share:.4f} | flips {ref.flips} |")
    assert np.isfinite(ref.diff64).all() and np.isfinite(ref.diff32).all() and ref.e_ref <= 2e-6
    assert ref.flips == 0
    if cls in ("edge10", "edge20"):
        amb, sure = (ref.amb10, ref.in10) if cls == "edge10" else (ref.amb20, ref.in20)
        assert np.array_equal(amb, (c.edge_m <= 0.5) & ~ref.exact)
        assert int(ref.exact.sum()) == 2 and ref.exact[0] and ref.exact[4] and sure[0] and not sure[4]
        decidable, n = ~amb, amb.size               # (every pixel of the frame: each is the one masked pixel of some view)
        assert decidable.sum() >= 0.5 * n and (decidable & sure).sum() > 0.2 * n and (decidable & ~sure).sum() > 0.2 * n
        assert np.array_equal(sure[~amb & ~ref.exact], c.edge_side[~amb & ~ref.exact] < 0)
    else:
        assert share <= AMBIGUOUS_CAP.get(cls, 0.01)
    # the float32 statement passes its own comparator, on one-hot views of every pixel and without a mask plane
    hot = VR.one_hot(om.size, np.arange(om.size)) if frame == VC.FRAME_A else VR.one_hot(om.size, VC.hot_positions(frame))
    worst, problems = VR.report(VR.fp32_rows(c, mv, hot), ref, hot)
    assert not problems and worst <= 1.0 + 1e-6, (worst, problems)
    worst, problems = VR.report(VR.fp32_rows(c, mv, None, om_rows=hot), ref, None, om_rows=hot)
    assert not problems, problems


def test_new_classes_have_their_properties():
    tiny = np.finfo(np.float32).tiny
    c = VC.hard_case("denormal", PC.MAIN)
    o = c.omap.reshape(3, -1).T
    sub = (o != 0) & (np.abs(o) < tiny)
    assert (sub.sum(axis=1) == 1).sum() > 1000 and (sub.sum(axis=1) == 3).sum() > 1000
    assert ((o == 0).all(axis=1)).sum() > 2000 and (np.signbit(o) & (o == 0)).any()
    assert (sub.any(axis=1) == ((o != 0).any(axis=1) & (np.abs(o).max(axis=1) < tiny))).all()      # subnormal pixels hold nothing larger
    c = VC.hard_case("fg_edge", PC.MAIN)
    for v in VC.FG_EDGE_VALUES:
        assert ((c.fg == v) | (np.isnan(c.fg) & np.isnan(v))).sum() > 1000
    assert float(VC.FG_EDGE_VALUES[1]) < 0.5 < float(VC.FG_EDGE_VALUES[2])
    c = VC.hard_case("gt_ends", PC.MAIN)
    th = VC.theta64(c.omap.reshape(3, -1).T, c.view, PC.MIN_VAL)
    g = c.gt.reshape(-1)
    for lo in (True, False):
        for at0 in (True, False):
            assert (((th < 1e-2) == lo) & ((g == 0) == at0)).sum() > 1000
    assert set(np.unique(g)) == {np.float32(0), PC.PI32_BELOW}
    c = VC.hard_case("unit", VC.FRAME_A, clamp=True)
    assert (c.pred < 0).sum() > 20 and (c.pred > 1).sum() > 20
    for cls in VC.CLASSES:
        c = VC.hard_case(cls, PC.MAIN)
        assert c.pred.min() >= 0 and c.pred.max() <= 1 and (c.pred == c.gt_rgb).all(axis=0).sum() > 300
        assert 0.6 < c.mask.mean() < 0.8 and c.gt.min() >= 0 and float(c.gt.max()) < np.pi
    pos = VC.hot_positions(PC.MAIN)
    assert {0, 63, 64, 255, 256, 511, 512, 767, 768, 8776, 8448, 8703} <= set(pos) and max(pos) == 67 * 131 - 1


def test_no_float32_diff_equals_a_threshold():
    """The exact pair straddles each threshold on neighbouring points of the 2^-23 lattice, and the thresholds are off it."""
    for T in (VC.T10, VC.T20):
        g_in, g_out = VC.edge_pair(np.float32(T))
        d_in, d_out = (float(VC.diff32_at_theta_zero(g)) for g in (g_in, g_out))
        assert d_in < T < d_out and d_out - d_in == 2.0 ** -23
        assert math.ldexp(d_in, 23) == int(math.ldexp(d_in, 23)) and math.ldexp(T, 23) != int(math.ldexp(T, 23))
    rng = np.random.default_rng(3)
    t = rng.uniform(0, np.pi, 1 << 20).astype(np.float32)
    for T in (VC.T10, VC.T20):
        g = (t + np.float32(T) + rng.integers(-64, 64, t.size) * np.float32(2.0 ** -26)).astype(np.float32)
        d = VC.HALF_PI32 - np.abs(np.abs(t - g) - VC.HALF_PI32)
        assert not (d == np.float32(T)).any() and (np.abs(d - np.float32(T)) < 1e-6).sum() > 1000


# ---- the size edges ----------------------------------------------------------------------------------------------------------------
SOME_COMBOS = [(True, True, "conf"), (False, True, "noconf"), (False, False, "none")]     # at the multi-megapixel sizes


@pytest.mark.parametrize("hw", VC.SMALL_SIZES)
def test_exact_planes_give_the_integer_sums_on_the_cpu_path(hw):
    """_cpu_stats on the exact planes equals the integer sums bit for bit for every combination of absent planes, V = 3."""
    from loss.image_metrics import _cpu_stats
    x = VC.exact_planes(3, hw)
    t = torch.from_numpy
    for combo in VC.COMBOS:
        with_mask, with_fg, ori = combo
        got = _cpu_stats(t(x.pred), t(x.gt), t(x.fg) if with_fg else None, t(x.mask) if with_mask else None,
                         t(x.omap) if ori != "none" else None, t(x.viewmats), t(x.gt_theta) if ori != "none" else None,
                         t(x.conf) if ori == "conf" else None, 1e-7, 0.5).numpy()
        assert np.array_equal(got, VC.exact_expected(x, combo)), combo


def test_exact_planes_are_exact_at_the_largest_size_and_every_view_differs():
    x = VC.exact_planes(1, VC.LARGE_SIZES[-1])
    for combo in SOME_COMBOS:                 # (_isum asserts the lattice and N * max * 2^q < 2^53)
        want = VC.exact_expected(x, combo)
        assert np.isfinite(want).all() and want[0, 0] > 1e5
    x = VC.exact_planes(65535, 1)
    want = VC.exact_expected(x, (True, True, "conf"))
    assert len(np.unique(want, axis=0)) > 2000 and len(np.unique(x.pred.reshape(65535, 3), axis=0)) > 65000
    for k in range(10):
        assert len(np.unique(want[:, k])) >= 2, k
    x = VC.exact_planes(3, 4097)
    assert len({tuple(np.flatnonzero(m.reshape(-1))) for m in x.viewmats[:, :3, :2]}) == 3


@pytest.mark.parametrize("mutant", VR.SIZE_MUTANTS)
def test_the_exact_sums_see_a_wrong_loop(mutant):
    """The last stride trip dropped: at every size that has more than one trip; a 3-plane tensor read at v * HW: at every V = 3
    frame, in every combination."""
    if mutant == "drop_last_trip":
        for hw in VC.LARGE_SIZES[3:]:
            x = VC.exact_planes(1, hw)
            for combo in SOME_COMBOS:
                a, b = VC.exact_expected(x, combo), VC.exact_expected(x, combo, nb=VC.num_blocks(hw), mutant=mutant)
                assert a[0, 0] != b[0, 0] and not np.array_equal(a, b), (hw, combo)
    else:
        for hw in VC.SMALL_SIZES:
            x = VC.exact_planes(3, hw)
            for combo in VC.COMBOS:
                a, b = VC.exact_expected(x, combo), VC.exact_expected(x, combo, mutant=mutant)
                assert np.array_equal(a[0], b[0]) and a[1, 0] != b[1, 0] and a[2, 0] != b[2, 0], (hw, combo)


# ---- the comparator has teeth -----------------------------------------------------------------------------------------------------------
ONE_HOT_ONLY = ("edge_in_out", "no_shift")


def _layouts(c):
    n = c.mask.size
    whole = np.stack([c.mask.reshape(-1) != 0, VC.second_mask(c.frame).reshape(-1) != 0])
    return {"one-hot": VR.one_hot(n, np.arange(n) if n <= 256 else VC.hot_positions(c.frame)), "whole": whole}


@pytest.mark.parametrize("mutant,cls", [(m, c) for m, cs in VR.MUTANTS.items() for c in cs])
def test_the_comparator_rejects_a_wrong_statement(mutant, cls):
    """Each mutant on the class listed for it, at the K the GPU file uses, by the one-hot views of both layouts.  The sums of
    whole planes (two views at 67 x 131) see the mutants that touch many pixels; ONE_HOT_ONLY they cannot see, which is what the
    one-hot views are for: a changed decision on one pixel hides in the ambiguous allowance of a plane, and the shift of
    `zero_in_mask` moves a pixel's angle by 2 yardsticks at most, with either sign."""
    seen_whole = False
    for frame in (VC.FRAME_A, PC.MAIN):
        c = VC.hard_case(cls, frame)
        ref = VR.pixel_reference(c, PC.MIN_VAL)
        for name, masks in _layouts(c).items():
            if frame == VC.FRAME_A and name == "whole":
                continue
            good = VR.report(VR.fp32_rows(c, PC.MIN_VAL, masks), ref, masks)
            worst, problems = VR.report(VR.fp32_rows(c, PC.MIN_VAL, masks, mutant=mutant), ref, masks)
            print(f"mutant | {mutant} | {cls} | {frame[0]}x{frame[1]} {name} | {worst:.3g} | {problems[:3]} |")
            assert not good[1], good
            assert problems or name == "whole", (mutant, cls, frame, name)
            seen_whole = seen_whole or (name == "whole" and bool(problems))
    assert seen_whole == (mutant not in ONE_HOT_ONLY or cls == "faint"), (mutant, cls)


# ---- the reference is pinned -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", VC.MIN_VALS)
def test_reference_against_the_training_term_in_float64(mv, monkeypatch):
    """sum(diff64 * conf) / count over the mask is loss/losses.py::_orientation_term on float64 tensors."""
    from loss import losses as Ls
    monkeypatch.setattr(Ls, "fused_losses", False)
    c = VC.hard_case("unit", PC.MAIN, mv)
    ref = VR.pixel_reference(c, mv)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)   # noqa: E731
    cam = types.SimpleNamespace(world_view_transform=t(c.view), orientation_field=t(c.gt), orientation_confidence=t(c.conf),
                                mask=torch.tensor(c.mask != 0))
    want = float(Ls._orientation_term(t(c.omap), types.SimpleNamespace(min_val=float(np.float32(mv))), cam, torch.zeros(3, dtype=torch.float64)))
    om = c.mask.reshape(-1) != 0
    got = math.fsum((ref.diff64 * ref.conf)[om]) / om.sum()
    assert abs(got - want) <= 1e-13 * abs(want), (got, want)


@pytest.mark.parametrize("cls", ["unit", "fg_edge", "denormal"])
def test_reference_against_the_cpu_path(cls):
    """_cpu_stats on a hard plane, two views with different masks, with and without a mask plane: accepted by the comparator at
    K = 1 + the float32 product's rounding, counts equal to the float32 statement's."""
    from loss.image_metrics import _cpu_stats
    c = VC.hard_case(cls, PC.MAIN)
    ref = VR.pixel_reference(c, PC.MIN_VAL)
    masks = _layouts(c)["whole"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    two = lambda a: t(np.stack([a, a]))   # noqa: E731
    args = (two(c.pred), two(c.gt_rgb), two(c.fg))
    rest = (two(c.omap), two(c.view), two(c.gt), two(c.conf), PC.MIN_VAL, 0.5)
    got = _cpu_stats(*args, t(masks.reshape(2, *c.frame)), *rest).numpy()
    worst, problems = VR.report(got, ref, masks)
    print(f"_cpu_stats | {cls} | {worst:.3f} yardsticks | {problems} |")
    assert not problems and worst <= 1.0 + 1e-3
    mine = VR.fp32_rows(c, PC.MIN_VAL, masks)
    assert np.array_equal(got[:, [2, 3, 4, 7]], mine[:, [2, 3, 4, 7]])
    assert np.abs(got[:, 8:] - mine[:, 8:]).max() <= max(int(ref.amb10.sum()), int(ref.amb20.sum()))
    all_rows = np.ones((2, c.mask.size), bool)
    got = _cpu_stats(*args, None, *rest).numpy()
    worst, problems = VR.report(got, ref, None, om_rows=all_rows)
    assert not problems and worst <= 1.0 + 1e-3, (worst, problems)
