"""Seeded scenes for the float64 check of blend_fwd_kernel / blend_bwd_kernel (csrc/hgs_blend.hip): tile lists whose length, stop
position, clamp, threshold and segment structure are what the case says.  numpy only; tests/blend_reference.py grades them,
tests/test_blend_f64_cpu.py asserts what each class below is listed for.

Construction.  A narrow camera (10 degrees: the projection's off-axis terms stay under 1 %) looks down +z; a Gaussian is an
isotropic `cov3D_precomp` of `sigma` pixels placed at a chosen pixel position, and its depth grows with the order it was added
in: a tile's list is the order of the add() calls.  A Gaussian whose radius r = ceil(3 sqrt(sigma^2 + 0.3)) and centre c (pixels,
inside its tile) satisfy r <= c < 17 - r touches that one tile only.  Colours are `colors_precomp`.

Every scene carries `classes` {name: tile indices or flat pixel indices y * W + x}, `bg7` (a non-zero 7-channel background),
`extra4` [P, 4] (the single pass's extra channels) and `dpix7` [7, H, W] (the upstream gradient).

Left out, with the reason:
  * `stop` at list positions 1 and 2 with clear margin: alpha <= 0.99 bounds T (1 - alpha) >= 1e-2 after one entry and >= 1e-4
    (1 - O(ulp)) after two -- the second decision sits ON the stop threshold, never clear of it.  Position 3 is the earliest
    clear stop; the case holds 3 and 4.
"""
import math

import numpy as np

from tests import scenes

FORMS = ("bg", "black", "seven")
FOV_DEG = 10.0
DEPTH0 = 2.0
DEPTH_STEP = 1e-3
OFF = 0.1                           # a Gaussian "on" a pixel sits this far off its centre: |power| >= 1e-5 there, the pixel stays clear
SPLIT_S = (128, 256, 1024)          # segment lengths the `split` case is pinned to (hgs_set_segment_policy(S, S, 1))


class _Builder:
    def __init__(self, W, H, seed):
        self.W, self.H = W, H
        self.cam = scenes.make_camera(eye=(0.0, 0.0, -DEPTH0), target=(0, 0, 0), W=W, H=H, fovx_deg=FOV_DEG)
        self.rng = np.random.default_rng(seed)
        self.rows = []

    def add(self, px, py, sigma, opacity, color=None, indefinite=False):
        """One Gaussian centred on pixel position (px, py), `sigma` pixels wide, behind everything added before."""
        z = DEPTH0 + DEPTH_STEP * len(self.rows)
        fx = self.W / (2.0 * self.cam["tanfovx"])
        x = ((2.0 * px + 1.0) / self.W - 1.0) * z * self.cam["tanfovx"]
        y = ((2.0 * py + 1.0) / self.H - 1.0) * z * self.cam["tanfovy"]
        s2 = (sigma * z / fx) ** 2
        cov = (s2, 0.0, 0.0, -0.5 * s2 if indefinite else s2, 0.0, s2)
        if color is None:
            color = self.rng.uniform(-1.0, 1.0, 3)
        self.rows.append((x, y, z - DEPTH0, opacity, cov, tuple(color)))
        return len(self.rows) - 1

    def tile_centre(self, t):
        gx = (self.W + 15) // 16
        return 16.0 * (t % gx), 16.0 * (t // gx)

    def scene(self, name, classes):
        P = len(self.rows)
        rng = np.random.default_rng(1000 + P)
        s = dict(self.cam)
        s.update(name=name,
                 means3D=np.array([[r[0], r[1], r[2]] for r in self.rows], np.float32).reshape(P, 3),
                 opacities=np.array([r[3] for r in self.rows], np.float32),
                 cov3D_precomp=np.array([r[4] for r in self.rows], np.float32).reshape(P, 6),
                 colors_precomp=np.array([r[5] for r in self.rows], np.float32).reshape(P, 3),
                 shs=None, scales=None, rotations=None, sh_degree=0, scale_modifier=1.0)
        return _finish(s, classes, rng)


def _finish(s, classes, rng):
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    s["bg7"] = np.array([0.3, -0.2, 0.7, 0.5, -0.4, 0.25, 0.6], np.float32)
    s["bg"] = s["bg7"][:3].copy()
    s["extra4"] = rng.uniform(-1.0, 1.0, (P, 4)).astype(np.float32)
    s["dpix7"] = rng.normal(size=(7, H, W)).astype(np.float32)
    s["classes"] = {k: np.asarray(v, np.int64) for k, v in classes.items()}
    return s


def _pix(W, pts):
    return [int(y) * W + int(x) for x, y in pts]


def _compact(b, t, n, op_lo, op_hi, sig_lo=1.4, sig_hi=1.9):
    """n single-tile Gaussians in tile t: radius <= 7, centres in [7.5, 9.5)^2 of the tile."""
    x0, y0 = b.tile_centre(t)
    for _ in range(n):
        b.add(x0 + b.rng.uniform(7.5, 9.5), y0 + b.rng.uniform(7.5, 9.5), b.rng.uniform(sig_lo, sig_hi),
              b.rng.uniform(op_lo, op_hi))


BATCH_COUNTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)    # around REC_BATCH 64 and BWD_BATCH 32


def batch_edges():
    b = _Builder(64, 48, 11)
    classes = {}
    for t, n in enumerate(BATCH_COUNTS):
        _compact(b, t, n, 0.01, 0.03)
        classes[f"n{n}"] = [t]
    return b.scene("batch_edges", classes)


def stop():
    b = _Builder(64, 48, 12)
    W = 64
    cl = {}
    # tiles 0, 1: stacks of twelve near-opaque Gaussians centred ON a pixel: that pixel stops at position 3 (alpha 0.983: 0.017^2 is
    # 3 thresholds, 0.017^3 stops) and at position 4 (alpha 0.948: 0.052^3 is 1.4 thresholds)
    for t, op, key in ((0, 0.985, "stop_at_3"), (1, 0.95, "stop_at_4")):
        x0, y0 = b.tile_centre(t)
        for _ in range(12):
            b.add(x0 + 8.0 + OFF, y0 + 8.0 + OFF, 2.0, op)
        cl[key] = _pix(W, [(x0 + 8, y0 + 8)])
    # tiles 2..5: p - 2 faint entries, then two opaque ones, all centred between the four middle pixels (G = 0.9435 there): the
    # second opaque entry stops those pixels at position p, from a final_T of 7e-4 .. 9e-4; five more entries behind (tile 5: none,
    # the stop is the list's last entry)
    tiny = []
    for t, p, op_low, trail, key in ((2, 63, 0.07, 5, "stop_at_63"), (3, 64, 0.07, 5, "stop_at_64"), (4, 65, 0.07, 5, "stop_at_65"),
                                     (5, 40, 0.10, 0, "stop_at_last")):
        x0, y0 = b.tile_centre(t)
        for k in range(p - 2):
            b.add(x0 + 7.5, y0 + 7.5, 2.0, op_low)
        b.add(x0 + 7.5, y0 + 7.5, 2.0, 1.0)
        b.add(x0 + 7.5, y0 + 7.5, 2.0, 1.0)
        for k in range(trail):
            b.add(x0 + 7.5, y0 + 7.5, 2.0, op_low)
        cl[key] = _pix(W, [(x0 + 7, y0 + 7), (x0 + 8, y0 + 7), (x0 + 7, y0 + 8), (x0 + 8, y0 + 8)])
        if t != 5:
            tiny += cl[key]
    cl["tiny_final_T"] = tiny
    # tile 6: six faint entries for every quadrant, then stacks of eight opaque needles-of-a-pixel in quadrants 0 and 3 only
    x0, y0 = b.tile_centre(6)
    _compact(b, 6, 6, 0.05, 0.1)
    st, nv = [], []
    for cx, cy in ((4.5, 4.5), (11.5, 11.5)):
        for _ in range(8):
            b.add(x0 + cx, y0 + cy, 1.0, 1.0)
        st += _pix(W, [(x0 + cx - 0.5, y0 + cy - 0.5), (x0 + cx + 0.5, y0 + cy - 0.5), (x0 + cx - 0.5, y0 + cy + 0.5),
                       (x0 + cx + 0.5, y0 + cy + 0.5)])
    for qx, qy in ((8, 0), (0, 8)):
        nv += _pix(W, [(x0 + qx + i, y0 + qy + j) for i in range(8) for j in range(8)])
    cl["quadrants_stop"], cl["quadrants_never"] = st, nv
    return b.scene("stop", cl)


def clamp():
    b = _Builder(64, 48, 13)
    W = 64
    centres = ((12, 12, 1.0), (44, 14, 0.999), (26, 36, 0.995))
    for x, y, op in centres:                       # opacity x G above 0.99 on the centre pixel, 0.98 on its four neighbours
        b.add(x + OFF, y + OFF, 6.0, op)
    for _ in range(8):                             # what lies behind them
        b.add(b.rng.uniform(8, 56), b.rng.uniform(8, 40), b.rng.uniform(5.0, 9.0), b.rng.uniform(0.03, 0.2))
    cl = {"clamped": _pix(W, [(x, y) for x, y, _ in centres]),
          "just_under": _pix(W, [(x + i, y + j) for x, y, _ in centres for i, j in ((1, 0), (-1, 0), (0, 1), (0, -1))])}
    return b.scene("clamp", cl)


def faint():
    b = _Builder(64, 48, 14)
    W = 64
    col = lambda: b.rng.uniform(-10.0, 10.0, 3)    # noqa: E731
    for k in range(36):
        kind = k % 3
        if kind == 0:                              # alpha in [1.2, 3] / 255 on the class pixels (G >= 0.72 there)
            b.add(32, 24, 14.0, b.rng.uniform(1.7, 3.0) / 255.0, col())
        elif kind == 1:                            # below the 1 / 255 threshold everywhere
            b.add(32, 24, 14.0, b.rng.uniform(0.3, 0.8) / 255.0, col())
        else:                                      # an indefinite conic (cov3D_precomp = sigma^2 diag(1, -1/2, 1)) centred above the
            b.add(b.rng.uniform(28, 36), 4, 14.0, 0.5, col(), indefinite=True)   # class pixels: power > 0 there
    cl = {"faint": _pix(W, [(x, y) for x in range(24, 40) for y in range(16, 32)])}
    return b.scene("faint", cl)


SPLIT_TILES = {"list_200": (0, 200), "list_300": (2, 300), "list_2200": (8, 2200)}
SPLIT_PLANTS = {"stop_first_seg": ((10, 11, 12), (4, 4)), "stop_middle_seg": ((600, 601, 602), (8, 3)),
                "stop_seg_last_entry": ((1019, 1021, 1023), (12, 4)), "stop_seg_first_entry": ((1018, 1020, 1024), (4, 12)),
                "stop_last_seg": ((2190, 2191, 2192), (12, 12))}


def split():
    """Tiles 0, 2 and 8 with lists of 200, 300 and 2200 single-tile entries.  S = 128: two, three and eighteen segments;
    S = 256: unsplit, unsplit, nine; S = 1024: unsplit, unsplit, three.  In tile 8 five triples of alpha 0.985 on a pixel the faint
    entries do not reach stop that pixel at the triple's third entry: list index 12 (first segment), 602 (a middle one at S = 128
    and 256), 1023 and 1024 (last / first entry of a segment for every S that divides 1024), 2192 (last segment).  The tile's
    middle pixels stop on the faint entries alone, wherever that falls."""
    b = _Builder(64, 48, 15)
    W = 64
    cl = {}
    _compact(b, 0, 200, 0.01, 0.1)
    _compact(b, 2, 300, 0.01, 0.1)
    x0, y0 = b.tile_centre(8)
    plant_at = {}
    for key, (ks, (lx, ly)) in SPLIT_PLANTS.items():
        for k in ks:
            assert k not in plant_at
            plant_at[k] = (lx, ly)
        cl[key] = _pix(W, [(x0 + lx, y0 + ly)])
    for k in range(2200):
        if k in plant_at:
            lx, ly = plant_at[k]
            b.add(x0 + lx + OFF, y0 + ly + OFF, 0.8, 0.985)
        else:
            b.add(x0 + b.rng.uniform(7.5, 9.5), y0 + b.rng.uniform(7.5, 9.5), b.rng.uniform(1.6, 1.8), b.rng.uniform(0.004, 0.03))
    cl["never"] = _pix(W, [(x0, y0), (x0 + 15, y0), (x0, y0 + 15), (x0 + 15, y0 + 15)])
    for key, (t, _) in SPLIT_TILES.items():
        cl[key] = [t]
    return b.scene("split", cl)


def _border(W, H, n, seed):
    b = _Builder(W, H, seed)
    for k in range(n):
        op = 0.95 if k % 3 == 2 else b.rng.uniform(0.05, 0.4)
        if k % 2:
            b.add(W - 1 + OFF, b.rng.integers(0, H) + OFF, 3.0, op)        # centred on the last column
        else:
            b.add(b.rng.integers(0, W) + OFF, H - 1 + OFF, 3.0, op)        # centred on the last row
    edge = [(W - 1, y) for y in range(H)] + [(x, H - 1) for x in range(W - 1)]
    return b.scene(f"border_{W}x{H}", {"edge": _pix(W, edge)})


def border_37x21():
    return _border(37, 21, 60, 16)


def border_7x5():
    return _border(7, 5, 20, 17)


def needles(n=160):
    """Thin strand Gaussians as scenes.strand_scene makes them (one long axis, 1e-4 across, SH colour of degree 0), laid out for a
    64 x 48 image: 3 to 8 pixels long at any angle in the image plane, 0.55 pixels across once the 0.3 dilation is added -- the
    conic's eigenvalues differ by a factor 30 to 200, `power` is a difference of terms many times its size, and footprints cross
    quadrant and tile boundaries."""
    b = _Builder(64, 48, 18)
    rng = b.rng
    fx = 64 / (2.0 * b.cam["tanfovx"])
    xyz, scales, quats = [], [], []
    for k in range(n):
        z = DEPTH0 + DEPTH_STEP * k
        px, py, th = rng.uniform(2, 62), rng.uniform(2, 46), rng.uniform(0, math.pi)
        xyz.append((((2 * px + 1) / 64 - 1) * z * b.cam["tanfovx"], ((2 * py + 1) / 48 - 1) * z * b.cam["tanfovy"], z - DEPTH0))
        scales.append((rng.uniform(3.0, 8.0) * z / fx, 1e-4, 1e-4))
        quats.append((math.cos(th / 2), 0.0, 0.0, math.sin(th / 2)))
    s = dict(b.cam)
    s.update(name="needles", means3D=np.array(xyz, np.float32), opacities=rng.uniform(0.3, 0.95, n).astype(np.float32),
             scales=np.array(scales, np.float32), rotations=np.array(quats, np.float32), cov3D_precomp=None, colors_precomp=None,
             shs=((rng.uniform(0, 1, (n, 1, 3)) - 0.5) / 0.28209479177387814).astype(np.float32), sh_degree=0, scale_modifier=1.0)
    return _finish(s, {"all": np.arange(64 * 48)}, np.random.default_rng(19))


CASES = {"batch_edges": batch_edges, "stop": stop, "clamp": clamp, "faint": faint, "split": split, "border_37x21": border_37x21,
         "border_7x5": border_7x5, "needles": needles}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def split_of(n, S):
    """(number of segments, segment length) of a list of n entries at segment length S: csrc/hgs_common.h hgs_split_of."""
    if n <= S * 6 // 4:
        return 1, n
    seglen, nseg = S, -(-n // S)
    if nseg > 63:
        seglen = ((-(-n // 63)) + 63) & ~63
        nseg = -(-n // seglen)
    return nseg, seglen
