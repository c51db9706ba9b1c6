"""The float64 statement of the per-view image statistics (loss/image_metrics.py's docstring; csrc/hgs_view_stats.hip) and the
comparator built on it (tests/test_view_stats_f64_cpu.py, tests/test_view_stats_f64_gpu.py).  No product code.

Per pixel, from the reference alone:
  e_c          the three float32 squares (pred_c - gt_c)^2 in numpy -- IEEE basic operations, the same bits on any device;
  mask, fg     GT-mask membership (!= 0), foreground membership (fg >= float32(0.5); NaN is not foreground);
  om           orientation-mask membership: the GT mask, else any(omap != 0);
  diff64       pi/2 - | |theta - gt| - pi/2 | in float64 with true pi; theta - gt from pixel_reference.orientation_statement,
               which tests/test_pixel_f64_cpu.py holds to loss/losses.py::_orientation_term;
  kappa        max(1, |o| / r) as tests/pixel_reference.py defines it: the rounding of px, py that an fp32 angle carries.
A pixel is AMBIGUOUS for a threshold T when |diff64 - T| <= DELTA * kappa: there the count may take either value.  A pixel
whose view-plane x is exactly 0 with y > 0 has theta = 0 on every implementation, so its float32 diff is IEEE-exact: it is
never ambiguous, and is decided by that float32 value (`sure`).

The bar of a sum over a set S of orientation pixels is sum_S K * yard * kappa_i (* conf_i for the weighted sum): the per-pixel
bar added up.  yard = max(4 * 2^-23, worst |diff32 - diff64| / kappa of the float32 CPU statement on that case).
"""
import math
import types

import numpy as np
import torch

from tests import pixel_reference as R
from tests import view_stats_cases as VC

DELTA = R.DELTA
ULP4 = R.ULP4
# K: twice the worst ratio measured on the MI355X (DESIGN.md section 2 holds the table), rounded up to a power of two, never
# above 8.  Measured: worst ratio 0.66 (`unit`, 16 x 16 one-hot views; tests/test_view_stats_f64_gpu.py lists every class) -> K = 2.
K_VS = 2.0
STATS = ["sse", "sse_hair", "mask_count", "fg_count", "inter_count", "orient_abs_sum", "orient_weighted_sum", "orient_count",
         "orient_within_10_count", "orient_within_20_count"]
# mutant -> the classes whose cases must reject it (tests/test_view_stats_f64_cpu.py); the last two belong to the size edges
MUTANTS = {"no_wrap": ["wrap"], "view_transposed": ["unit"], "no_shift": ["faint", "zero_in_mask"], "edge_in_out": ["edge10", "edge20"],
           "fg_gt": ["fg_edge"], "om_from_omap": ["zero_in_mask"], "hair_by_fg": ["unit"]}
SIZE_MUTANTS = ["drop_last_trip", "view_offset"]
_STATEMENT_MUTANTS = ("no_wrap", "view_transposed", "no_shift")


def _diff(omap, view, min_val, gt, dtype, mutant=None):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)   # noqa: E731
    keep = {}
    with R._one_thread():
        R.orientation_statement(t(omap), t(view), float(np.float32(min_val)), t(gt), torch.ones((), dtype=dtype), None, torch.zeros(3, dtype=dtype),
                                mutant if mutant in _STATEMENT_MUTANTS else None, keep)
        e = keep["e"]
        diff = R.HALF_PI - torch.abs(torch.abs(e) - R.HALF_PI)
    return diff.numpy()


def orientation_pixels(omap, view, min_val, gt):
    """diff64, kappa, the float32 statement's diff32, and the exact-theta pixels of one view (arrays [H, W])."""
    omap, gt = np.asarray(omap, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    flat = omap.reshape(3, -1).T
    p = VC.view_xy(flat, view)
    kappa = VC.kappa64(flat, view).reshape(gt.shape)
    exact = ((p[:, 0] == 0) & (p[:, 1] > 0)).reshape(gt.shape)
    return types.SimpleNamespace(diff64=_diff(omap, view, min_val, gt, torch.float64), diff32=_diff(omap, view, min_val, gt, torch.float32),
                                 kappa=kappa, exact=exact, diff_exact=VC.diff32_at_theta_zero(gt).astype(np.float64))


def _decide(o, T):
    """(sure_in, ambiguous) of one threshold: float64 decides, except on exact-theta pixels, where the float32 value does."""
    amb = (np.abs(o.diff64 - T) <= DELTA * o.kappa) & ~o.exact
    return np.where(o.exact, o.diff_exact <= T, o.diff64 <= T) & ~amb, amb


def ambiguous_counts(omap, view, min_val, gt, om):
    """(ambiguous for 10 degrees, for 20 degrees) among the pixels `om` of one view."""
    o = orientation_pixels(omap, view, min_val, gt)
    return tuple(int((_decide(o, T)[1] & om).sum()) for T in (VC.T10, VC.T20))


def pixel_reference(c, min_val, with_conf=True):
    """Everything the comparator needs about one hard case (tests/view_stats_cases.py hard_case), per pixel, flat [HW]."""
    d = c.pred - c.gt_rgb
    e = d * d                                                        # float32
    assert e.dtype == np.float32
    e64 = e.astype(np.float64)
    o = orientation_pixels(c.omap, c.view, min_val, c.gt)
    conf = c.conf.astype(np.float64) if with_conf else np.ones(c.gt.shape)
    in10, amb10 = _decide(o, VC.T10)
    in20, amb20 = _decide(o, VC.T20)
    f = lambda a: np.asarray(a).reshape(-1)   # noqa: E731
    nz = (c.omap != 0).any(axis=0)
    ref = types.SimpleNamespace(case=c, min_val=min_val, e_terms=e64.reshape(3, -1), sse_pix=f((e64[0] + e64[1]) + e64[2]),
                                fg=f(c.fg >= np.float32(0.5)), nonzero=f(nz), diff64=f(o.diff64), diff32=f(o.diff32.astype(np.float64)),
                                kappa=f(o.kappa), conf=f(conf), in10=f(in10), amb10=f(amb10), in20=f(in20), amb20=f(amb20), exact=f(o.exact))
    ref.e_ref = float((np.abs(ref.diff32 - ref.diff64) / ref.kappa).max())
    ref.yard = max(ref.e_ref, ULP4)
    ref.flips = int(((f(o.diff32) <= np.float32(VC.T10)) != ref.in10)[~ref.amb10].sum() + ((f(o.diff32) <= np.float32(VC.T20)) != ref.in20)[~ref.amb20].sum())
    return ref


def fp32_rows(c, min_val, masks, with_conf=True, mutant=None, om_rows=None):
    """[N, 10]: the float32 statement's statistics of N views that share the planes of `c` and differ in their GT mask (masks:
    bool [N, HW]), summed in float64.  masks None: no mask plane, and om_rows [N, HW] says which pixels of each view's direction
    image are not zeroed (layouts with a one-hot omap).  mutant: one of MUTANTS, a subtly wrong statement."""
    d = c.pred - c.gt_rgb
    e = (d * d).astype(np.float64).reshape(3, -1)
    pix = (e[0] + e[1]) + e[2]
    diff = _diff(c.omap, c.view, min_val, c.gt, torch.float32, mutant).reshape(-1)
    w = (diff * c.conf.reshape(-1)) if with_conf else diff
    th10, th20 = np.float32(VC.T10), np.float32(VC.T20)
    if mutant == "edge_in_out":       # the largest value the statement can produce below the threshold counts as outside
        th10, th20 = (np.nextafter(VC.diff32_at_theta_zero(VC.edge_pair(t)[0]), np.float32(0)) for t in (th10, th20))
    fg = (c.fg > np.float32(0.5)) if mutant == "fg_gt" else (c.fg >= np.float32(0.5))
    fg = fg.reshape(-1)
    nz = (c.omap != 0).any(axis=0).reshape(-1)
    N = len(masks) if masks is not None else len(om_rows)
    M = np.zeros((N, pix.size), bool) if masks is None else masks
    om = (om_rows & nz[None]) if masks is None else (np.broadcast_to(nz, M.shape) if mutant == "om_from_omap" else M)
    hair = (M & fg[None]) if mutant == "hair_by_fg" else M
    s = lambda sel, val: (sel * np.asarray(val, dtype=np.float64)[None]).sum(axis=1)   # noqa: E731
    one = np.ones(pix.size)
    out = np.zeros((N, 10))
    out[:, 0] = math.fsum(e.reshape(-1))
    out[:, 1], out[:, 2] = s(hair, pix), s(M, one)
    out[:, 3], out[:, 4] = fg.sum(), s(M & fg[None], one)
    out[:, 5], out[:, 6], out[:, 7] = s(om, diff), s(om, w), s(om, one)
    out[:, 8], out[:, 9] = s(om, diff <= th10), s(om, diff <= th20)
    return out


def report(rows, ref, masks=None, om_rows=None, K=K_VS):
    """(worst ratio in yardsticks, problems) of [N, 10] statistics against the float64 reference: the comparator of the one-hot
    views and of whole planes alike.  masks / om_rows as in fp32_rows."""
    rows = np.asarray(rows, dtype=np.float64)
    problems = []
    if not np.isfinite(rows).all():
        return float("inf"), ["non-finite"]
    maskless = masks is None
    M = np.zeros((len(rows), ref.sse_pix.size), bool) if maskless else masks
    om = (om_rows & ref.nonzero[None]) if maskless else M
    cnt = lambda sel: sel.sum(axis=1).astype(np.float64)   # noqa: E731
    for k, want in ((2, cnt(M)), (3, np.full(len(rows), float(ref.fg.sum()))), (4, cnt(M & ref.fg[None])), (7, cnt(om))):
        if not np.array_equal(rows[:, k], want):
            problems.append(f"{STATS[k]}: {int((rows[:, k] != want).sum())} views differ")
    total = math.fsum(ref.e_terms.reshape(-1))
    if np.abs(rows[:, 0] - total).max() > ref.e_terms.size * 2.0 ** -53 * total:
        problems.append("sse")
    for v in range(len(rows)):
        idx = np.flatnonzero(M[v])
        if len(idx) == 1:                       # one pixel: the float64 sum of its three squares in order, no tolerance
            ok = rows[v, 1] == ref.sse_pix[idx[0]]
        else:
            want = math.fsum(ref.e_terms[:, idx].reshape(-1))
            ok = abs(rows[v, 1] - want) <= 3 * len(idx) * 2.0 ** -53 * want
        if not ok:
            problems.append(f"sse_hair of view {v}")
    for k, sure, amb in ((8, ref.in10, ref.amb10), (9, ref.in20, ref.amb20)):
        lo = cnt(om & sure[None])
        hi = lo + cnt(om & amb[None])
        bad = (rows[:, k] < lo) | (rows[:, k] > hi) | (rows[:, k] != np.rint(rows[:, k]))
        if bad.any():
            problems.append(f"{STATS[k]}: {int(bad.sum())} views outside [sure, sure + ambiguous]")
    worst = 0.0
    for k, weight in ((5, np.ones_like(ref.conf)), (6, ref.conf)):
        want = (om * (ref.diff64 * weight)[None]).sum(axis=1)
        bar = (om * (ref.yard * ref.kappa * weight)[None]).sum(axis=1)
        err = np.abs(rows[:, k] - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bar)
        worst = max(worst, float(ratio.max(initial=0.0)))
    if worst > K:
        problems.append(f"orientation sums: {worst:.3g} yardsticks")
    return worst, problems


def one_hot(n_pix, positions):
    m = np.zeros((len(positions), n_pix), bool)
    m[np.arange(len(positions)), positions] = True
    return m
