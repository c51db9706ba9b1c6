"""Seeded inputs for the float64 checks of the per-pixel loss terms -- the orientation term and the mask term (binary
cross-entropy with logits) of csrc/hgs_losses.hip -- numpy only, no product code: what tests/ssim_cases.py is for SSIM / L1.
tests/test_pixel_f64_cpu.py shows on the CPU that every class has the property it is listed for and that the fp32 statement
stays within its caps; tests/test_pixel_f64_gpu.py runs the HIP kernels on the same arrays.

A direction case is (class, (H, W), mask variant); a head case adds a logit class.  Every list is explicit.
"""
import functools
import types
import zlib

import numpy as np

MIN_VAL = float(np.float32(1e-6))      # gaussians.min_val as the C ABI receives it (a `float`)
PI32_BELOW = np.float32(3.1415925)     # the largest fp32 below pi: targets lie in [0, pi)

# ---- frames ---------------------------------------------------------------------------------------------------------------------
SMALL, MAIN, LARGE = (5, 7), (67, 131), (725, 725)
FRAMES = [SMALL, MAIN, LARGE]
assert (MAIN[0] * MAIN[1]) % 256 and MAIN[0] % 16 and MAIN[1] % 16 and MAIN[0] % 32 and MAIN[1] % 32
# 2054 pixel workgroups: the tail's `i += 256` loop, unrolled 8 times, takes one full unrolled trip and a remainder
assert (LARGE[0] * LARGE[1] + 255) // 256 == 2054 and 2048 < 2054 < 2 * 2048


# ---- view matrix ----------------------------------------------------------------------------------------------------------------
def _view_matrix():
    """world_view_transform (row vectors: p_view = p_world @ V[:3, :3], translation in the last ROW): a seeded rotation far
    from the identity and far from symmetric, so a transposed or mis-indexed V shows."""
    rng = np.random.default_rng(20240517)
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    V = np.eye(4)
    V[:3, :3] = q
    V[3, :3] = rng.uniform(-2, 2, 3)
    return np.ascontiguousarray(V, dtype=np.float32)


VIEW = _view_matrix()
VIEW.setflags(write=False)
assert np.abs(VIEW[:3, :3] - np.eye(3)).max() > 0.5 and np.abs(VIEW[:3, :3] - VIEW[:3, :3].T).max() > 0.3
_R64 = VIEW[:3, :3].astype(np.float64)
_RINV = np.linalg.inv(_R64)            # view-space vector -> world: o = v_view @ _RINV
Z_VIEW = _RINV[2]                      # the world direction along the view axis


def view_plane(flat32):
    """(px, py) = (o @ V[:3, :3])[:, :2] of fp32 world vectors [N, 3], in float64."""
    return (np.asarray(flat32, dtype=np.float64) @ _R64)[:, :2]


def theta64(flat32):
    """The angle of loss/losses.py::_orientation_term in float64 (numpy; used to PLACE targets, the reference of the tests is
    tests/pixel_reference.py)."""
    p = view_plane(flat32)
    n = np.hypot(p[:, 0], p[:, 1]) + MIN_VAL
    x, y = p[:, 0] / n, p[:, 1] / n
    y = np.where(y < MIN_VAL, y + MIN_VAL, y)
    th = np.arctan2(x, y)
    return np.where(th < 0, th + np.pi, th)


# ---- direction-image classes: flat [N, 3] world vectors (float64, rounded to fp32 by the caller) ----------------------------------
def _dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _log_uniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def _unit(rng, n):
    return _dirs(rng, n) * rng.uniform(0.2, 1.0, (n, 1))


def _faint(rng, n):
    """r far below, around and above min_val = 1e-6: the `y < min_val` shift matters."""
    return _dirs(rng, n) * _log_uniform(rng, 1e-9, 1e-3, n)[:, None]


def _zero_in_mask(rng, n):
    o = _unit(rng, n)
    o[rng.uniform(size=n) < 0.2] = 0.0
    return o


HEAD_ON_EPS = (1e-4, 1e-1)


def _head_on(rng, n):
    """a * z_view + eps * d: nearly along the view axis, px and py come from cancellation."""
    return rng.uniform(0.2, 1.0, (n, 1)) * Z_VIEW[None] + _log_uniform(rng, *HEAD_ON_EPS, n)[:, None] * _dirs(rng, n)


def _wrap(rng, n):
    """View-space x within 1e-7 .. 1e-3 of 0 on either side, both signs of y: theta on either side of 0 / pi."""
    x = _log_uniform(rng, 1e-7, 1e-3, n) * rng.choice([-1.0, 1.0], n)
    y = rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)
    z = rng.uniform(-1.0, 1.0, n)
    return np.stack([x, y, z], 1) @ _RINV


_DIRECTION = {"unit": _unit, "faint": _faint, "zero_in_mask": _zero_in_mask, "head_on": _head_on, "wrap": _wrap, "kinks": _unit}
CLASSES = list(_DIRECTION)

# ---- mask variants ----------------------------------------------------------------------------------------------------------------
BG_BLACK, BG_COLOUR = (0.0, 0.0, 0.0), (0.1, 0.2, 0.3)
MASKS = ["m70", "one", "empty", "none_black", "none_colour"]


def _background_pixels(rng, o, bg):
    """No mask: it is derived as omap != bg.  15 % of the pixels equal bg, 5 % differ from it in one component only, and
    zeros come with either sign."""
    n = o.shape[0]
    b = np.asarray(bg, dtype=np.float32)
    u = rng.uniform(size=n)
    o[u < 0.15] = b
    one = np.flatnonzero((u >= 0.15) & (u < 0.20))
    o[one] = b
    o[one, rng.integers(0, 3, len(one))] += np.float32(0.25)
    neg = np.flatnonzero(u < 0.05)
    if bg == BG_BLACK:
        o[neg] = np.float32(-0.0)                       # equals bg: unmasked
        sel = one[::2]
        o[sel[o[sel, 0] == 0], 0] = np.float32(-0.0)    # -0.0 beside the one component that differs
    else:
        o[neg] = np.array([0.0, -0.0, 0.0], np.float32)  # differs from bg, r = 0
    return o


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def direction_case(cls, frame, mask="m70"):
    """omap [3, H, W], gt [H, W] in [0, pi), conf [H, W] in [0, 1) with exact zeros, mask uint8 [H, W] or None, bg: the same
    read-only arrays on every call."""
    H, W = frame
    n = H * W
    rng = np.random.default_rng([zlib.crc32(cls.encode()), zlib.crc32(mask.encode()), H, W])
    flat = _DIRECTION[cls](rng, n).astype(np.float32)
    bg = BG_COLOUR if mask == "none_colour" else BG_BLACK
    if mask.startswith("none"):
        flat = _background_pixels(rng, flat, bg)
    gt = rng.uniform(0.0, np.pi, n)
    if cls == "kinks":     # near, not on, the kinks of the bidirectional difference: e = 0 and |e| = pi / 2
        gt = theta64(flat) + rng.choice([0.0, np.pi / 2, -np.pi / 2], n) + rng.choice([-1.0, 1.0], n) * _log_uniform(rng, 1e-4, 1e-1, n)
        gt = np.mod(gt, np.pi)
    gt = np.minimum(gt.astype(np.float32), PI32_BELOW)
    conf = rng.uniform(0.0, 1.0, n).astype(np.float32)
    conf = np.minimum(conf, np.float32(1.0 - 2.0 ** -24))
    conf[rng.uniform(size=n) < 0.05] = 0.0
    m = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    if mask == "one":
        m[:] = 0
        m[(n * 2) // 3] = 1
        conf[(n * 2) // 3] = np.float32(0.75)
    elif mask == "empty":
        m[:] = 0
    omap = flat.reshape(H, W, 3).transpose(2, 0, 1)
    return types.SimpleNamespace(cls=cls, frame=frame, mask_variant=mask, omap=_f32(omap), gt=_f32(gt.reshape(H, W)),
                                 conf=_f32(conf.reshape(H, W)), bg=bg,
                                 mask=None if mask.startswith("none") else _ro(m.reshape(H, W)))


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


# ---- logit classes of the mask term: (logits x, target y), fp32 [H, W] -----------------------------------------------------------------
def _sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def _logit_mixed(rng, n):
    return rng.uniform(-2, 2, n), (rng.uniform(size=n) < 0.5)


def _confident(rng, n):
    y = rng.uniform(size=n) < 0.5
    return rng.uniform(5, 30, n) * np.where(y, 1.0, -1.0), y


def _confident_wrong(rng, n):
    y = rng.uniform(size=n) < 0.5
    return rng.uniform(5, 30, n) * np.where(y, -1.0, 1.0), y


def _extreme(rng, n):
    x = rng.uniform(60, 120, n) * rng.choice([-1.0, 1.0], n)
    u = rng.uniform(size=n)
    x[u < 0.02] = 0.0
    x[(u >= 0.02) & (u < 0.04)] = -0.0
    return x, (rng.uniform(size=n) < 0.5)


def _soft_target(rng, n):
    """Fractional targets, as a resized mask has (with exact 0 and 1 among them)."""
    y = np.clip(rng.uniform(-0.2, 1.2, n), 0.0, 1.0)
    return rng.uniform(-4, 4, n), y


def _cancel(rng, n):
    """y = fp32(sigmoid(x)): the gradient sigmoid(x) - y is what rounding leaves."""
    x = rng.uniform(-4, 4, n).astype(np.float32)
    return x, _sigmoid64(x)


_LOGITS = {"logit_mixed": _logit_mixed, "confident": _confident, "confident_wrong": _confident_wrong, "extreme": _extreme,
           "soft_target": _soft_target, "cancel": _cancel}
LOGIT_CLASSES = list(_LOGITS)


@functools.lru_cache(maxsize=None)
def logit_case(cls, frame):
    H, W = frame
    rng = np.random.default_rng([zlib.crc32(cls.encode()), H, W, 7])
    x, y = _LOGITS[cls](rng, H * W)
    return _f32(np.asarray(x, dtype=np.float32).reshape(H, W)), _f32(np.asarray(y, dtype=np.float32).reshape(H, W))


# ---- the lists ------------------------------------------------------------------------------------------------------------------
# every class at MAIN with the 70 % mask; `unit` also on the other two frames and with the other mask variants
MASKED_CASES = [(c, MAIN, "m70") for c in CLASSES] + [("unit", SMALL, "m70"), ("unit", LARGE, "m70"),
                                                      ("unit", MAIN, "one"), ("unit", MAIN, "empty")]
MASKLESS_CASES = [(c, MAIN, m) for c in ("unit", "zero_in_mask") for m in ("none_black", "none_colour")]   # stand-alone path only
DIRECTION_CASES = MASKED_CASES + MASKLESS_CASES
# the loss head (masked views only): each direction class rides with one logit class; `unit` + `logit_mixed` on all frames
_PARTNER = dict(zip(CLASSES, LOGIT_CLASSES))
assert _PARTNER["unit"] == "logit_mixed" and len(CLASSES) == len(LOGIT_CLASSES)
HEAD_CASES = [(c, _PARTNER[c], f, m) for c, f, m in MASKED_CASES]
LOGIT_CASES = sorted({(l, f) for _, l, f, _ in HEAD_CASES})
# the one-pass form with a tile hint, without float64: 2^24 - 9 pixels (pixel -> row through a float reciprocal and its
# correction step) and 2^24 + 4090 (the integer division)
HUGE_FRAMES = [(4099, 4093), (4099, 4094)]
assert HUGE_FRAMES[0][0] * HUGE_FRAMES[0][1] == (1 << 24) - 9 and HUGE_FRAMES[1][0] * HUGE_FRAMES[1][1] >= (1 << 24)


def case_id(case):
    *names, frame, mask = case
    return "-".join(names) + f"-{frame[0]}x{frame[1]}-{mask}"
