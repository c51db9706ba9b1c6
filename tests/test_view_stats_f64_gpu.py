"""csrc/hgs_view_stats.hip (`loss.image_metrics._gpu_stats`) against the float64 statement of tests/view_stats_reference.py on
the inputs of tests/view_stats_cases.py; tests/test_view_stats_f64_cpu.py keeps the bars honest.
  a. one-hot views: a batch of V views over one hard plane, view v with a GT mask (or, without a mask plane, a direction
     image) set at one pixel only, so the per-view sums ARE that pixel's terms -- layout A (16 x 16, every pixel) and layout B
     (67 x 131, three blocks: lanes 0, 63, 64, 255, the ends of every stride trip, the last pixel), every class, both min_val;
  b. the render clamped by the wrapper (`clamp`, through view_metrics);
  c. every size edge on planes whose sums are exact: equality with integer sums for every combination of absent planes, the
     grid's y limit V = 65535, and the two refusals;
  d. whole hard planes, two views with different masks, against the summed per-pixel bars;
  e. the wrapper hands the kernel what it expects (strides, dtypes).
Counts are exact; the within-10 / within-20 counts are decided by float64 outside the ambiguous pixels; sse_hair of a one-pixel
mask is the float64 sum of the three numpy float32 squares, bit for bit; orientation sums within K * yard * kappa_i per pixel.
Each test prints its row before it asserts (`pytest -s`): case, worst ratio in yardsticks.

Measured on the MI355X, worst |diff - diff64| / (kappa * yard) per class over both layouts, both min_val, with and without a
mask plane (yard = 4 * 2^-23 everywhere: every class's e_ref is below the floor):
  unit 0.66 | faint 0.57 | zero_in_mask 0.54 | head_on 0.13 | wrap 0.47 | kinks 0.64 | edge10 0.50 | edge20 0.49 | denormal 0.48 |
  fg_edge 0.58 | gt_ends 0.42 | clamp (through the wrapper) 0.60; with and without a mask plane the same figures (the same pixels);
  whole planes, the summed bar: <= 0.07 (67 x 131), 0.03 (725 x 725).
K = twice the worst ratio (0.66), rounded up to a power of two = 2.  No within count left [sure, sure + ambiguous], every count,
every one-pixel sse_hair and every statistic of the exact planes was equal: the kernel needed no change.
"""
import numpy as np
import pytest
import torch

from tests import pixel_cases as PC
from tests import view_stats_cases as VC
from tests import view_stats_reference as VR

pytestmark = pytest.mark.gpu

K = VR.K_VS
NAN = float("nan")


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _rep(a, n):
    t = _dev(a)
    return t[None].expand(n, *t.shape).contiguous()


def _stats(c, min_val, masks=None, om_rows=None, with_fg=True, with_conf=True):
    """[N, 10] from the kernel: N views that share the planes of `c`; masks bool [N, HW] are their GT masks, or (no mask
    plane) om_rows the pixels of each view's direction image that are kept."""
    from loss.image_metrics import _gpu_stats
    n = len(masks) if masks is not None else len(om_rows)
    H, W = c.frame
    omap = _rep(c.omap, n)
    mask = None
    if masks is not None:
        mask = _dev(masks.reshape(n, H, W))
    else:
        omap = torch.where(_dev(om_rows.reshape(n, 1, H, W)), omap, torch.zeros((), device="cuda"))
    out = _gpu_stats(_rep(c.pred, n), _rep(c.gt_rgb, n), _rep(c.fg, n) if with_fg else None, mask, omap, _rep(c.view, n), _rep(c.gt, n),
                     _rep(c.conf, n) if with_conf else None, min_val, 0.5)
    return out.numpy()


def _hot(frame):
    n = frame[0] * frame[1]
    return VR.one_hot(n, np.arange(n) if frame == VC.FRAME_A else VC.hot_positions(frame))


# ---- a. one-hot views ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", VC.MIN_VALS, ids=lambda m: f"{m:.0e}")
@pytest.mark.parametrize("frame", [VC.FRAME_A, PC.MAIN], ids=["A", "B"])
@pytest.mark.parametrize("cls", VC.CLASSES)
def test_one_hot_views_against_float64(cls, frame, mv):
    c = VC.hard_case(cls, frame, mv)
    ref = VR.pixel_reference(c, mv)
    hot = _hot(frame)
    masked = _stats(c, mv, masks=hot)
    maskless = _stats(c, mv, om_rows=hot)
    w1, p1 = VR.report(masked, ref, hot, K=K)
    w2, p2 = VR.report(maskless, ref, None, om_rows=hot, K=K)
    print(f"row | a | {cls} | {frame[0]}x{frame[1]} | {mv:.0e} | views {len(hot)} | masked {w1:.3f} | maskless {w2:.3f} | {p1 + p2} |")
    assert not p1 and not p2, (p1, p2)
    # without a confidence plane the weighted sum is the plain one, bit for bit; without a foreground plane its counts are 0
    bare = _stats(c, mv, masks=hot, with_fg=False, with_conf=False)
    assert np.array_equal(bare[:, 6], bare[:, 5]) and np.array_equal(bare[:, 5], masked[:, 5]) and not bare[:, 3:5].any()
    assert np.array_equal(bare[:, [0, 1, 2, 7, 8, 9]], masked[:, [0, 1, 2, 7, 8, 9]])


# ---- b. the wrapper's clamp ------------------------------------------------------------------------------------------------------------
def test_clamped_render_through_the_wrapper():
    from loss.image_metrics import STATS, view_metrics
    raw = VC.hard_case("unit", VC.FRAME_A, clamp=True)
    c = VC.hard_case("unit", VC.FRAME_A)
    c = type(c)(**{**vars(c), "pred": np.clip(raw.pred, 0, 1)})
    ref = VR.pixel_reference(c, VC.MIN_VALS[1])
    hot = _hot(VC.FRAME_A)
    n = len(hot)
    out = view_metrics(_rep(raw.pred, n), _rep(c.gt_rgb, n), fg=_rep(c.fg, n), gt_mask=_dev(hot.reshape(n, 16, 16)), omap=_rep(c.omap, n),
                       viewmats=_rep(c.view, n), gt_theta=_rep(c.gt, n), confidence=_rep(c.conf, n))
    rows = np.array([[m[k] for k in STATS] for m in out])
    worst, problems = VR.report(rows, ref, hot, K=K)
    print(f"row | b | clamp | {worst:.3f} | {problems} |")
    assert not problems, problems
    assert (raw.pred < 0).any() and (raw.pred > 1).any()


# ---- c. the size edges -----------------------------------------------------------------------------------------------------------------
def _exact_run(x, combo):
    from loss.image_metrics import _gpu_stats
    with_mask, with_fg, ori = combo
    d = x.dev
    return _gpu_stats(d["pred"], d["gt"], d["fg"] if with_fg else None, d["mask"] if with_mask else None,
                      d["omap"] if ori != "none" else None, d["viewmats"], d["gt_theta"] if ori != "none" else None,
                      d["conf"] if ori == "conf" else None, VC.MIN_VALS[1], 0.5).numpy()


def _upload(x):
    x.dev = {k: _dev(getattr(x, k)) for k in ("pred", "gt", "fg", "mask", "omap", "viewmats", "gt_theta", "conf")}
    return x


@pytest.mark.parametrize("hw", VC.SMALL_SIZES + VC.LARGE_SIZES)
def test_every_size_edge_gives_the_integer_sums(hw):
    """1 .. 257 and 4095 .. 4097 pixels with V = 3 (per-view hashes and view matrices); 64 / 65 rows for the second-stage
    reduce, the block cap reached and binding, and a 17th and 18th stride trip with V = 1: all ten statistics equal the integer
    sums, for every combination of absent planes."""
    import hgs_runtime as rt
    V = 3 if hw <= 4097 else 1
    assert rt.lib().hgs_view_stats_num_blocks(1, hw) == VC.num_blocks(hw)
    x = _upload(VC.exact_planes(V, hw))
    for combo in VC.COMBOS:
        got = _exact_run(x, combo)
        want = VC.exact_expected(x, combo)
        assert np.array_equal(got, want), (hw, combo, got, want)
    del x
    torch.cuda.empty_cache()


def test_the_grid_y_limit_and_the_refusals():
    """V = 65535 at 1 x 1, every view distinct, all rows checked; V = 65536 and H W = 2^30 + 1 are refused with the library's
    error and nothing is launched (the NaN-filled outputs stay untouched)."""
    import hgs_runtime as rt
    x = _upload(VC.exact_planes(65535, 1))
    for combo in ((True, True, "conf"), (False, True, "noconf")):
        assert np.array_equal(_exact_run(x, combo), VC.exact_expected(x, combo)), combo
    L = rt.lib()
    assert L.hgs_view_stats_num_blocks(1, (1 << 30) + 1) == 0 and L.hgs_view_stats_num_blocks(32769, 32768) == 0
    assert L.hgs_view_stats_num_blocks(32768, 32768) == 1024 and L.hgs_view_stats_num_blocks(0, 5) == 0
    big = _upload(VC.exact_planes(65536, 1))
    partials = torch.full((65536, 1, 10), NAN, dtype=torch.float64, device="cuda")
    out = torch.full((65536, 10), NAN, dtype=torch.float64, device="cuda")
    d = big.dev
    args = [d["pred"].data_ptr(), d["gt"].data_ptr(), d["mask"].data_ptr(), d["fg"].data_ptr(), 0.5, d["omap"].data_ptr(),
            d["viewmats"].data_ptr(), d["gt_theta"].data_ptr(), d["conf"].data_ptr(), VC.MIN_VALS[1], partials.data_ptr(), out.data_ptr()]
    for V, H, W in ((65536, 1, 1), (1, 1, (1 << 30) + 1), (0, 1, 1)):
        assert L.hgs_view_stats(rt.current_stream(), V, H, W, *args) == 1
        assert "hgs_view_stats: bad sizes" in L.hgs_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(partials).all())
    from loss.image_metrics import _gpu_stats
    with pytest.raises(rt.HgsError, match="bad sizes"):
        _gpu_stats(d["pred"], d["gt"], None, None, None, None, None, None, 1e-7, 0.5)
    # the same buffers are accepted one view short
    assert L.hgs_view_stats(rt.current_stream(), 65535, 1, 1, *args) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:65535].cpu().numpy(), VC.exact_expected(x, (True, True, "conf")))
    assert bool(torch.isnan(out[65535]).all())


# ---- d. whole planes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,frame", [(c, PC.MAIN) for c in VC.CLASSES] + [("unit", PC.LARGE)],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_whole_planes_against_the_summed_bars(cls, frame):
    """Two views with different masks (70 % and an independent 30 %), and the same planes without a mask plane."""
    for mv in VC.MIN_VALS:
        c = VC.hard_case(cls, frame, mv)
        ref = VR.pixel_reference(c, mv)
        masks = np.stack([c.mask.reshape(-1) != 0, VC.second_mask(frame).reshape(-1) != 0])
        w1, p1 = VR.report(_stats(c, mv, masks=masks), ref, masks, K=K)
        every = np.ones((1, c.mask.size), bool)
        w2, p2 = VR.report(_stats(c, mv, om_rows=every), ref, None, om_rows=every, K=K)
        print(f"row | d | {cls} | {frame[0]}x{frame[1]} | {mv:.0e} | masked {w1:.3f} | maskless {w2:.3f} | {p1 + p2} |")
        assert not p1 and not p2, (p1, p2)


# ---- e. the wrapper ----------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_hands_the_kernel_what_it_expects():
    """Non-contiguous planes, masks of other dtypes, float64 angles and a non-contiguous view-matrix batch give the same dicts,
    bit for bit, as contiguous float32 / bool inputs."""
    from loss.image_metrics import view_metrics
    c = VC.hard_case("unit", PC.MAIN)
    V = 3
    H, W = c.frame
    masks = np.stack([c.mask != 0, VC.second_mask(c.frame) != 0, np.zeros(c.frame, bool)])
    vm = _rep(c.view, V) * torch.tensor([1.0, -1.0, 1.0], device="cuda")[:, None, None]
    base = dict(pred_rgb=_rep(VC.hard_case("unit", PC.MAIN, clamp=True).pred, V), gt_rgb=_rep(c.gt_rgb, V), fg=_rep(c.fg, V), gt_mask=_dev(masks),
                omap=_rep(c.omap, V) * torch.tensor([1.0, 0.5, -1.0], device="cuda")[:, None, None, None], viewmats=vm,
                gt_theta=_rep(c.gt, V), confidence=_rep(c.conf, V))
    want = view_metrics(**base)
    assert want[0]["orient_count"] > 0 and want[2]["orient_err_deg"] is None and want[0] != want[1]

    def channel_last(t):          # the same values, channel-last storage permuted back
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

    def every_second(t):          # a [::2] slice of a buffer twice as long in the last dimension
        wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
        wide[..., ::2] = t
        return wide[..., ::2]

    m = base["gt_mask"]
    variants = {
        "channel-last": dict(pred_rgb=channel_last(base["pred_rgb"]), omap=channel_last(base["omap"]), fg=base["fg"].transpose(1, 2).contiguous().transpose(1, 2)),
        "sliced": dict(pred_rgb=every_second(base["pred_rgb"]), omap=every_second(base["omap"]), fg=every_second(base["fg"]), gt_rgb=every_second(base["gt_rgb"])),
        "bool mask, strided": dict(gt_mask=every_second(m)),
        "uint8 mask 2 / 255": dict(gt_mask=torch.where(m, torch.where(_dev(c.gt) > 1.5, 2, 255), 0).to(torch.uint8)),
        "int64 mask": dict(gt_mask=m.to(torch.int64) * -7),
        "float mask": dict(gt_mask=m.to(torch.float32) * 0.5),
        "float64 angles": dict(gt_theta=base["gt_theta"].double(), confidence=base["confidence"].double()),
        "viewmats transposed twice": dict(viewmats=vm.transpose(1, 2).contiguous().transpose(1, 2)),
    }
    for name, change in variants.items():
        for k, t in change.items():
            assert torch.equal(t, base[k].to(t.dtype)) or k == "gt_mask", (name, k)
        if name not in ("uint8 mask 2 / 255", "int64 mask", "float mask", "float64 angles"):
            assert any(not t.is_contiguous() for t in change.values()), name
        got = view_metrics(**{**base, **change})
        assert got == want, name
