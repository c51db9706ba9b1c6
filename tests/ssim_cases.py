"""Seeded inputs for the float64 SSIM / L1 checks (numpy only, fp32 images in [0, 1]; no product code): what tests/scenes.py
is for the rasterizer.  tests/test_ssim_f64_cpu.py shows on the CPU that every family has the property it is listed for and
that the fp32 reference stays within its caps; tests/test_ssim_f64_gpu.py runs the HIP kernels on the same pairs.

A case is (family, (C, H, W)).  CASES is an explicit list: a family that degenerates at a shape (no all-zero block fits
beside the hair below ~33 px of width) is absent from it, never skipped at run time.
"""
import functools
import zlib

import numpy as np

BLOCK = 32        # csrc/hgs_losses.hip LT: output pixels per side of an SSIM block (blocks per channel, edge blocks partial)
REACH = 10        # pixels an image value reaches in the gradient: window radius 5 forward, 5 again backward

# ---- shapes ---------------------------------------------------------------------------------------------------------------------
SMALLER_THAN_WINDOW = [(3, 1, 1), (3, 1, 4), (3, 2, 3), (3, 5, 4), (3, 11, 11)]      # W % 4 == 0: float4 loads, else scalar
BLOCK_EDGES = [(3, 32, 32), (3, 33, 33), (3, 31, 36), (3, 32, 64)]
SEVERAL_BLOCKS = [(3, 40, 44), (3, 61, 97), (3, 96, 128), (3, 70, 132)]              # 70 x 132: 3 x 5 blocks, a full 3 x 3 neighbourhood
# block totals around SSIM_SUBBANDS = 32 (the persistent workgroups' permutation has to visit every block exactly once)
BLOCK_TOTALS = [(3, 8, 320), (1, 8, 1024), (3, 8, 352), (1, 8, 1056), (2, 40, 44)]   # 30, 32, 33, 33, 8 blocks
SHAPES = SMALLER_THAN_WINDOW + BLOCK_EDGES + SEVERAL_BLOCKS + BLOCK_TOTALS
HEAD_SHAPES = [(3, 40, 44), (3, 33, 100), (3, 70, 132), (3, 96, 128)]                # the loss head: three channels always


def num_blocks(shape):
    C, H, W = shape
    return C * ((H + BLOCK - 1) // BLOCK) * ((W + BLOCK - 1) // BLOCK)


assert [num_blocks(s) for s in BLOCK_TOTALS] == [30, 32, 33, 33, 8]


# ---- families -------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _noise(rng, shape):
    a = rng.uniform(0, 1, shape)
    return a, np.clip(a + rng.normal(0, 0.1, shape), 0, 1)


def _smooth(rng, shape):
    """Low-frequency sinusoid (periods 64 and 80 px, per-channel gain; amplitude / period is what keeps the window variance
    under C2), target = image + a ripple of amplitude 0.02."""
    C, H, W = shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gain = np.array([1.0, 0.8, 0.6])[:C, None, None]
    ph = rng.uniform(0, 2 * np.pi, (C, 1, 1))
    a = 0.5 + 0.25 * gain * np.sin(2 * np.pi * x / 64 + ph) * np.cos(2 * np.pi * y / 80 + 0.5 * ph)
    b = a + 0.02 * np.sin(2 * np.pi * (x + 2 * y) / 23 + ph)
    return a, b


def _flat_bright(rng, shape):
    return 0.97 + rng.normal(0, 1e-3, shape), 0.97 + rng.normal(0, 1e-3, shape)


def hair_box(shape):
    """(y0, y1, x0, x1) of the box the hair families draw in, or None where no block could stay black.  Everything right of
    x1 + 1 -- the last block column grown by REACH, over all rows -- stays exactly zero in image and target (the target is
    the image moved right by 1 px); from 54 rows on the box keeps to the upper half (70 and 96 rows: the last block row stays
    black as well)."""
    C, H, W = shape
    x1 = (W - 1) // BLOCK * BLOCK - REACH - 1
    y1 = H - 1 if H < 54 else H // 2
    return (1, y1, 1, x1) if x1 >= 13 and y1 >= 2 else None


def _hair(rng, shape):
    C, H, W = shape
    y0, y1, x0, x1 = hair_box(shape)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gain = np.array([1.0, 0.85, 0.7])[:C, None, None]
    stripes = gain * (0.5 + 0.45 * np.sin(2 * np.pi * (x + 0.3 * y) / 5 + rng.uniform(0, 2 * np.pi, (C, 1, 1))))
    a = np.zeros(shape)
    a[:, y0:y1, x0:x1] = stripes[:, y0:y1, x0:x1]
    b = np.zeros(shape)
    b[:, :, 1:] = 0.95 * a[:, :, :-1]
    return a, b


def _hair_black_bg(rng, shape):
    return _hair(rng, shape)


def _render_black(rng, shape):
    return np.zeros(shape), _hair(rng, shape)[1]


def _binary(rng, shape):
    a = (rng.uniform(0, 1, shape) < 0.5).astype(np.float64)
    return a, 1 - a


def _identical(rng, shape):
    a = rng.uniform(0, 1, shape)
    return a, a.copy()


def _impulse(rng, shape):
    a = np.zeros(shape)
    a[-1, -1, -1] = 1.0                      # last channel, last row, last column: the far corner of the (partial) last block
    return a, np.zeros(shape)


_FAMILIES = {"noise": _noise, "smooth": _smooth, "flat_bright": _flat_bright, "hair_black_bg": _hair_black_bg,
             "render_black": _render_black, "binary": _binary, "identical": _identical, "impulse": _impulse}
FAMILIES = list(_FAMILIES)


@functools.lru_cache(maxsize=None)
def pair(family, shape):
    """(image, target), float32 [C, H, W] in [0, 1]: the same arrays on every call (read-only)."""
    rng = np.random.default_rng([zlib.crc32(family.encode()), *shape])
    a, b = _FAMILIES[family](rng, tuple(shape))
    a, b = _f32(np.clip(a, 0, 1)), _f32(np.clip(b, 0, 1))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


# ---- the list -------------------------------------------------------------------------------------------------------------------
_HAIR_SHAPES = [(3, 33, 33), (3, 40, 44), (3, 61, 97), (3, 96, 128), (3, 70, 132), (3, 8, 352), (2, 40, 44)]
assert all(hair_box(s) is not None for s in _HAIR_SHAPES + HEAD_SHAPES)
assert all(hair_box(s) is None for s in SMALLER_THAN_WINDOW + [(3, 32, 32)])
_LISTED = {
    "noise": SHAPES,
    "smooth": SHAPES,
    "flat_bright": [(3, 1, 4), (3, 5, 4), (3, 11, 11), (3, 33, 33), (3, 40, 44), (3, 61, 97), (3, 70, 132), (3, 8, 352)],
    "hair_black_bg": _HAIR_SHAPES,
    "render_black": _HAIR_SHAPES,
    "binary": [(3, 1, 4), (3, 2, 3), (3, 11, 11), (3, 33, 33), (3, 40, 44), (3, 61, 97), (1, 8, 1056)],
    # not below 20 pixels a block: with target = image every gradient is the rounding remainder of a cancelling sum, so a
    # block's yardstick is the largest of as many remainders as it has pixels.  At (3, 1, 1) it is ONE remainder a block, and
    # that one is exactly 0 in float64 in one channel and in the fp32 reference in two: the block bars would ask a kernel for
    # an exact cancellation the reference's own fp32 reaches by chance (tests/test_ssim_f64_cpu.py asserts that no listed
    # block's yardstick is such a zero).  (3, 5, 4) and (3, 11, 11) are the images smaller than the window, on both load paths.
    "identical": [(3, 5, 4), (3, 11, 11), (3, 32, 32), (3, 40, 44), (3, 70, 132), (3, 8, 320)],
    "impulse": [(3, 5, 4), (3, 11, 11), (3, 33, 33), (3, 31, 36), (3, 40, 44), (3, 61, 97), (3, 70, 132), (1, 8, 1056)],
}
CASES = [(f, s) for f in FAMILIES for s in _LISTED[f]]
assert all(sum(1 for f, _ in CASES if f == fam) >= 4 for fam in FAMILIES)
assert all((f, s) in CASES for f in ("noise", "smooth") for s in SHAPES)

# what test 3e perturbs the window on, and the loss head's cases
PERTURBED = [(f, (3, 40, 44)) for f in ("noise", "smooth", "hair_black_bg", "binary")]
assert all(c in CASES for c in PERTURBED)
HEAD_FAMILIES = ["hair_black_bg", "render_black", "impulse", "noise", "identical"]
HEAD_CASES = [(f, s) for f in HEAD_FAMILIES for s in HEAD_SHAPES]


def case_id(case):
    f, (C, H, W) = case
    return f"{f}-{C}x{H}x{W}"


def blocks(shape):
    """The kernel's own grid: (channel, y0, y1, x0, x1) per block, edge blocks partial."""
    C, H, W = shape
    return [(c, y0, min(y0 + BLOCK, H), x0, min(x0 + BLOCK, W))
            for c in range(C) for y0 in range(0, H, BLOCK) for x0 in range(0, W, BLOCK)]
