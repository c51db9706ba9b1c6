"""Seeded inputs for the float64 checks of the per-view image statistics (csrc/hgs_view_stats.hip behind loss/image_metrics.py)
-- numpy only, no product code: what tests/pixel_cases.py is for the training term, whose six direction classes are reused.
tests/test_view_stats_f64_cpu.py shows that every class has the property it is listed for; tests/test_view_stats_f64_gpu.py
runs the kernel on the same arrays.

  hard_case(cls, frame, min_val)   one view's planes: render (already clamped), capture, foreground channel, GT mask,
                                   direction image, view matrix, GT angle, confidence.
  hot_positions(frame)             the pixels of layout B (one one-hot view each).
  exact_planes(V, HW)              planes whose per-pixel terms are the same bits on every IEEE device and whose sums are exact
                                   in any order, with the integer sums they must give (exact_expected).
"""
import functools
import types
import zlib

import numpy as np

from tests import pixel_cases as PC

DELTA = 1e-5                                        # tests/pixel_reference.py DELTA (the CPU file asserts they agree)
MIN_VALS = [PC.MIN_VAL, float(np.float32(1e-7))]     # the training runs' value and loss/image_metrics.py MIN_VAL
T10, T20 = float(np.float32(10 * np.pi / 180)), float(np.float32(20 * np.pi / 180))   # the contract's float32 thresholds
HALF_PI32 = np.float32(np.pi / 2)
FRAME_A = (16, 16)
NEW_CLASSES = ["edge10", "edge20", "denormal", "fg_edge", "gt_ends"]
CLASSES = PC.CLASSES + NEW_CLASSES                   # `clamp` is `unit` with an unclamped render: it needs the wrapper
EDGE_MS = (0.0, 0.5, 3.0, 30.0)

# the view of the edge classes: px = o2, py = o0 exactly (not the identity, not symmetric), so a pixel (c, 0, 0) has x = 0 and
# atan2(0, y > 0) = 0 on every implementation
PERM = np.zeros((4, 4), np.float32)
PERM[2, 0] = PERM[0, 1] = PERM[1, 2] = PERM[3, 3] = 1.0
PERM[3, :3] = (0.5, -1.5, 2.0)
PERM.setflags(write=False)
assert np.abs(PERM[:3, :3] - PERM[:3, :3].T).max() == 1.0


def view_xy(flat32, view):
    return np.asarray(flat32, dtype=np.float64) @ np.asarray(view, dtype=np.float64)[:3, :2]


def theta64(flat32, view, min_val):
    """The angle of image_metrics.py's docstring in float64 (used to PLACE targets; the reference is view_stats_reference)."""
    p = view_xy(flat32, view)
    n = np.hypot(p[:, 0], p[:, 1]) + min_val
    x, y = p[:, 0] / n, p[:, 1] / n
    y = np.where(y < min_val, y + min_val, y)
    th = np.arctan2(x, y)
    return np.where(th < 0, th + np.pi, th)


def kappa64(flat32, view):
    p = view_xy(flat32, view)
    r = np.hypot(p[:, 0], p[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r > 0, np.maximum(1.0, np.linalg.norm(np.asarray(flat32, dtype=np.float64), axis=1) / r), 1.0)


def diff32_at_theta_zero(g):
    """The contract's float32 difference at theta = 0: IEEE subtractions and absolute values only."""
    g = np.asarray(g, dtype=np.float32)
    return HALF_PI32 - np.abs(np.abs(np.float32(0) - g) - HALF_PI32)


def edge_pair(th):
    """(g_in, g_out): float32 GT angles whose float32 difference from theta = 0 is the largest value <= th and the smallest
    > th that the statement can produce (tests/test_image_metrics_cpu.py::_edge_pair's method)."""
    g = np.float32(th)
    for _ in range(8):
        g = np.nextafter(g, np.float32(0))
    cands = []
    for _ in range(32):
        cands.append((g, diff32_at_theta_zero(g)))
        g = np.nextafter(g, np.float32(1))
    g_in = max((c for c in cands if c[1] <= th), key=lambda c: c[1])[0]
    g_out = min((c for c in cands if c[1] > th), key=lambda c: c[1])[0]
    return g_in, g_out


# ---- the new classes -------------------------------------------------------------------------------------------------------------
def _edge(rng, n, T, min_val):
    """Pixel i: diff64 = T + side * m * DELTA * kappa with m = EDGE_MS[i % 4], side = -1, +1 for i // 4 even, odd.  Pixels 0
    and 4 are the exact pair: (c, 0, 0) with the GT angles of edge_pair."""
    flat = np.zeros((n, 3), np.float32)
    todo = np.arange(n)
    while len(todo):                                 # directions with kappa <= 8: 30 DELTA kappa stays far inside (0, T)
        cand = PC._unit(rng, len(todo)).astype(np.float32)
        flat[todo] = cand
        todo = todo[kappa64(cand, PERM) > 8.0]
    i = np.arange(n)
    m = np.asarray(EDGE_MS)[i % 4]
    side = np.where((i // 4) % 2 == 0, -1.0, 1.0)
    th = theta64(flat, PERM, min_val)
    d = T + side * m * DELTA * kappa64(flat, PERM)
    gt = np.where(th + d < np.pi - 1e-3, th + d, th - d).astype(np.float32)
    g_in, g_out = edge_pair(np.float32(T))
    flat[0] = (0.75, 0.0, 0.0)
    flat[4] = (0.5, 0.0, 0.0)
    gt[0], gt[4] = g_in, g_out
    return flat, gt, m, side


def _denormal(rng, n):
    """Subnormal components (one, two or all three of a pixel), all-zero pixels beside them, -0.0, and ordinary pixels."""
    flat = PC._unit(rng, n).astype(np.float32)
    sub = (rng.integers(1, 1 << 22, (n, 3)).astype(np.float32) * np.float32(2.0 ** -149)) * rng.choice([-1.0, 1.0], (n, 3)).astype(np.float32)
    kind = np.arange(n) % 6                          # 0: ordinary, 1: all zero, 2..4: 1..3 subnormal components (rest 0), 5: -0.0
    flat[kind == 1] = 0.0
    for k in (2, 3, 4):
        for row in np.flatnonzero(kind == k):
            ch = (row + np.arange(k - 1)) % 3
            flat[row] = 0.0
            flat[row, ch] = sub[row, ch]
    flat[kind == 5] = np.float32(-0.0)
    return flat


FG_EDGE_VALUES = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)),
                           np.nan, 0.0, 1.0], np.float32)


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def hard_case(cls, frame, min_val=PC.MIN_VAL, clamp=False):
    """One view's planes (read-only, the same on every call): pred, gt_rgb [3, H, W] in [0, 1] (`clamp`: pred in [-0.3, 1.3],
    for the wrapper), fg [H, W], mask uint8 [H, W] (70 % set), omap [3, H, W], view [4, 4], gt, conf [H, W]."""
    H, W = frame
    n = H * W
    rng = np.random.default_rng([zlib.crc32(cls.encode()), H, W, 20250101])
    extra = {}
    view = PC.VIEW
    if cls in PC.CLASSES:
        d = PC.direction_case(cls, frame, "m70")
        omap, gt, conf, mask = d.omap, d.gt, d.conf, d.mask
    else:
        conf = np.minimum(rng.uniform(0.0, 1.0, n).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
        conf[rng.uniform(size=n) < 0.05] = 0.0
        mask = (rng.uniform(size=n) < 0.7).astype(np.uint8)
        gt = np.minimum(rng.uniform(0.0, np.pi, n).astype(np.float32), PC.PI32_BELOW)
        if cls in ("edge10", "edge20"):
            view = PERM
            flat, gt, m, side = _edge(rng, n, T10 if cls == "edge10" else T20, min_val)
            mask[:8] = 1                              # the exact pair and one pixel of every m are orientation pixels
            extra = dict(edge_m=m, edge_side=side)
        elif cls == "denormal":
            flat = _denormal(rng, n)
        elif cls == "gt_ends":
            flat = PC._wrap(rng, n).astype(np.float32)
            gt = np.where(rng.uniform(size=n) < 0.5, np.float32(0), PC.PI32_BELOW).astype(np.float32)
        else:
            assert cls == "fg_edge", cls
            flat = PC._unit(rng, n).astype(np.float32)
        omap = flat.reshape(H, W, 3).transpose(2, 0, 1)
        gt, conf, mask = gt.reshape(H, W), conf.reshape(H, W), mask.reshape(H, W)
    rng = np.random.default_rng([zlib.crc32(cls.encode()), H, W, 77])
    gt_rgb = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    pred = gt_rgb + rng.normal(0, 0.2, (3, H, W)).astype(np.float32) * (10.0 ** rng.uniform(-6, 0, (1, H, W))).astype(np.float32)
    same = rng.uniform(size=(H, W)) < 0.1            # errors of every size from 1e-7 up, and pixels with none
    pred[:, same] = gt_rgb[:, same]
    pred = pred * np.float32(1.6) - np.float32(0.3) if clamp else np.clip(pred, 0, 1)
    fg = rng.uniform(0, 1, (H, W)).astype(np.float32)
    fg[rng.uniform(size=(H, W)) < 0.1] = 0.5
    if cls == "fg_edge":
        fg = FG_EDGE_VALUES[rng.integers(0, len(FG_EDGE_VALUES), (H, W))]
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    mask.setflags(write=False)
    return types.SimpleNamespace(cls=cls, frame=frame, min_val=min_val, pred=_f32(pred), gt_rgb=_f32(gt_rgb), fg=_f32(fg), mask=mask,
                                 omap=_f32(omap), view=view, gt=_f32(gt), conf=_f32(conf), **extra)


@functools.lru_cache(maxsize=None)
def second_mask(frame):
    """The GT mask of the second view of a whole-plane run: 30 % set, independent of the class's."""
    m = (np.random.default_rng([frame[0], frame[1], 5]).uniform(size=frame) < 0.3).astype(np.uint8)
    m.setflags(write=False)
    return m


# ---- layout B ----------------------------------------------------------------------------------------------------------------------
BLOCK, PIX_PER_BLOCK, MAX_BLOCKS = 256, 4096, 1024


def num_blocks(hw):
    return min((hw + PIX_PER_BLOCK - 1) // PIX_PER_BLOCK, MAX_BLOCKS)


def hot_positions(frame):
    """Lanes 0, 63, 64, 255 of each block, the first and last pixel of each block's every stride trip, the frame's last pixel."""
    hw = frame[0] * frame[1]
    nb = num_blocks(hw)
    stride = nb * BLOCK
    pos = set()
    for b in range(nb):
        for lane in (0, 63, 64, 255):
            pos.add(b * BLOCK + lane)
        for first in range(b * BLOCK, hw, stride):
            pos.update((first, min(first + BLOCK - 1, hw - 1)))
    pos.add(hw - 1)
    return sorted(p for p in pos if p < hw)


assert num_blocks(PC.MAIN[0] * PC.MAIN[1]) == 3 and len(hot_positions(PC.MAIN)) > 70


# ---- size edges: exact planes ---------------------------------------------------------------------------------------------------------
SMALL_SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
LARGE_SIZES = [64 * 4096, 64 * 4096 + 1, 1024 * 4096, 1024 * 4096 + 1, 1024 * 4096 + 262144 + 77]
assert num_blocks(LARGE_SIZES[0]) == 64 and num_blocks(LARGE_SIZES[1]) == 65 and num_blocks(LARGE_SIZES[2]) == 1024
assert num_blocks(LARGE_SIZES[3]) == 1024 and LARGE_SIZES[4] > 17 * 262144
GT_LIST = np.array([0.0, 0.125, T10, np.nextafter(np.float32(T10), np.float32(1)), 0.3, T20, 1.0, 1.5, 1.625, 2.0, 3.0, PC.PI32_BELOW],
                   np.float32)
CONF_LIST = np.array([0.0, 0.25, 0.5, 1.0], np.float32)
C_LIST = np.array([0.0, 0.5, 1.0, 2.0, 0.75], np.float32)       # the one nonzero omap component; 0: nothing blended
FG_LIST = np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)
MASK_LIST = np.array([0, 1, 0, 255, 2, 0], np.uint8)
COMBOS = [(m, f, o) for m in (True, False) for f in (True, False) for o in ("none", "conf", "noconf")]


def _hash(p, v, k):
    """A 32-bit mix of pixel, view and plane number (uint64 arithmetic, murmur3's finalizer)."""
    h = (p.astype(np.uint64) * np.uint64(0x9E3779B1) + v.astype(np.uint64) * np.uint64(0x85EBCA77) + np.uint64(k * 0xC2B2AE3D + 1)) & np.uint64(0xFFFFFFFF)
    for mul in (0x85EBCA6B, 0xC2B2AE35):
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(16))


def exact_planes(V, hw):
    """pred, gt [V, 3, 1, hw] multiples of 2^-12 in [0, 1]; mask, fg; omap with one nonzero component c in channel (1, 2, 0)[v % 3]
    and a view matrix that sends that channel to y and an EMPTY channel to x (so x = 0 and theta = 0 exactly, while another
    view's matrix would give theta = pi / 2 or r = 0); gt_theta from GT_LIST, confidence from CONF_LIST.  Everything depends on
    (pixel, view) through hashes."""
    p = np.arange(hw, dtype=np.uint64)[None, :]
    v = np.arange(V, dtype=np.uint64)[:, None]
    q = lambda k, mod: (_hash(p, v, k) % np.uint64(mod)).astype(np.int64)
    pred = np.stack([q(k, 4097) for k in range(3)], 1).astype(np.float32) / np.float32(4096)
    gt = np.stack([q(3 + k, 4097) for k in range(3)], 1).astype(np.float32) / np.float32(4096)
    mask = MASK_LIST[q(6, len(MASK_LIST))]
    fg = FG_LIST[q(7, len(FG_LIST))]
    c = C_LIST[q(8, len(C_LIST))]
    gt_theta = GT_LIST[q(9, len(GT_LIST))]
    conf = CONF_LIST[q(10, len(CONF_LIST))]
    ych = (np.arange(V) + 1) % 3                     # the channel that carries c
    xch = (ych + 1) % 3                              # an empty channel
    omap = np.zeros((V, 3, hw), np.float32)
    omap[np.arange(V), ych] = c
    vm = np.zeros((V, 4, 4), np.float32)
    vm[:, :, 2:] = (_hash(np.arange(16, dtype=np.uint64)[None, :8], v, 11) % np.uint64(7)).astype(np.float32).reshape(V, 4, 2) - 3.0
    vm[:, 3, :2] = 2.5                               # (the translation row: never read)
    vm[np.arange(V), xch, 0] = 1.0
    vm[np.arange(V), ych, 1] = 1.0
    sh = lambda a: np.ascontiguousarray(a.reshape(a.shape[:-1] + (1, hw)))
    return types.SimpleNamespace(V=V, hw=hw, pred=sh(pred), gt=sh(gt), mask=sh(mask), fg=sh(fg), omap=sh(omap), viewmats=vm,
                                 gt_theta=sh(gt_theta), conf=sh(conf), c=c)


def _isum(a, q, keep):
    """Exact sum over the pixels of the float64 values `a` [V, hw] (multiples of 2^-q) where `keep`, through int64."""
    k = np.ldexp(a, q)
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max(initial=0) * a.shape[1] < 2.0 ** 53
    return np.ldexp(np.where(keep, k, 0).astype(np.int64).sum(axis=1).astype(np.float64), -q)


def exact_expected(x, combo, nb=None, mutant=None):
    """[V, 10] float64: the ten statistics of exact_planes as integer sums.  mutant: `drop_last_trip` (the pixels of the last
    grid-stride trip of a launch of nb blocks are not visited), `view_offset` (a 3-plane tensor read at v * HW)."""
    with_mask, with_fg, ori = combo
    V, hw = x.V, x.hw
    pred = x.pred.reshape(V, 3, hw)
    if mutant == "view_offset":
        flat = x.pred.reshape(V * 3, hw)
        pred = np.stack([flat[v:v + 3] for v in range(V)])
    visit = np.ones((1, hw), bool)
    if mutant == "drop_last_trip":
        stride = nb * BLOCK
        visit = (np.arange(hw) < (hw - 1) // stride * stride)[None, :]
    d = pred - x.gt.reshape(V, 3, hw)
    e = (d * d).astype(np.float64).sum(axis=1)       # three multiples of 2^-24 below 1: exact
    out = np.zeros((V, 10))
    out[:, 0] = _isum(e, 24, visit)
    m = (x.mask.reshape(V, hw) != 0) & with_mask
    out[:, 1] = _isum(e, 24, m & visit)
    out[:, 2] = (m & visit).sum(axis=1)
    f = (x.fg.reshape(V, hw) >= np.float32(0.5)) & with_fg
    out[:, 3] = (f & visit).sum(axis=1)
    out[:, 4] = (f & m & visit).sum(axis=1)
    if ori != "none":
        g = x.gt_theta.reshape(V, hw)
        diff = diff32_at_theta_zero(g)
        w = diff * x.conf.reshape(V, hw) if ori == "conf" else diff
        om = (m if with_mask else x.c != 0) & visit
        out[:, 5] = _isum(diff.astype(np.float64), 26, om)
        out[:, 6] = _isum(w.astype(np.float64), 28, om)
        out[:, 7] = om.sum(axis=1)
        out[:, 8] = (om & (diff <= np.float32(T10))).sum(axis=1)
        out[:, 9] = (om & (diff <= np.float32(T20))).sum(axis=1)
    return out
