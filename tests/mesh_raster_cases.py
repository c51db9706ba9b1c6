"""Hand-built hard inputs for the line / triangle rasterizer of the dataset synthesis (scene/mesh_renderer.py, csrc/hgs_raster.hip).

Every case is a function returning (models, views, projections, W, H, lighting, background, mesh_indices).  Window coordinates are
placed through identity view / projection as _ndc of tests/test_mesh_raster_cpu.py does: a vertex at (x, y) px gets
ndc = (x / W * 2 - 1, y / H * 2 - 1).  x and y are multiples of 1/256 px, so the snapped coordinates a case intends are
X = 256 x, Y = 256 y; each model built here carries them as `intent` ([N, 2] int64), checked while building against the float32
cast in exact rationals and asserted against the vertex stage by tests/test_mesh_raster_hard_cpu.py.  Frames with coordinates far
outside use power-of-two W and H, where the float32 ndc is exact.  The screen tile is 32x32: 96x70 has 3x3 tiles, the last row of
tiles 6 px high.

The decisions covered, by case:
  lines_directions    x- and y-major in both directions across 3 tile columns / rows; exact diagonals |dX| == |dY| in all four
                      directions, through centres and off them; end points on pixel centres (half-open interval); a slope of
                      -1/256 px (floor against truncating division)
  lines_tile_edges    lines along x or y = 31.5, 32, 32.5 (and 63.5, 64, 64.5) and on x = 31.99 .. 32.01, widths 1, 2 and 3; a minor band
                      that straddles a tile boundary inside one tile column
  lines_wide          widths 33 and 70; bands leaving the viewport below 0, above Wv - 1, and lying entirely outside; y = -0.5
  lines_far           end points at +-2000 px and +-16383.9 px on a 128x64 frame; zero-length, one-column and no-centre lines; lines
                      whose columns all lie left of 0 or right of W - 1
  tris_hard           a triangle covering every tile from far outside; a sub-pixel sliver across a tile corner; vertices on pixel
                      centres and tile corners; A == 0, A < 0; boxes empty after clipping
  tris_shared_edges   pairs sharing an edge on a tile boundary, through pixel centres next to it, and on a diagonal through a tile
                      corner: each centre covered once (COVERED_ONCE)
  depth_ties          equal depths across a tile boundary in both draw orders; z_w = 1, just below 1, and 0; a line losing only its
                      first fragment to the far-plane discard
  models_64           64 models, empty ones at the front, in the middle and at the end, lines and triangles interleaved
  mesh_subset         the same list with mesh_indices out of order and repeated
  all_empty           every model empty
  prims_255/256/257   the primitive count around the 256-lane workgroup
  hot_tile_300/1100   one tile listing more than 256 / 1024 primitives
  dropped_rules       c.w <= 0 (negative and zero), |c.z| > c.w at both planes, |x_w| and |y_w| > 2^14 and exactly 2^14; kept and
                      dropped vertices shared between kept and dropped primitives; two views dropping different primitives
  shading_persp       lit and unlit lines and triangles under a perspective camera with c.w from 0.1 to 1.0 along each primitive; a
                      model matrix with rotation and non-uniform scale
  shading_edges       a zero normal, the light at a fragment, cos < 0, colours below 0 and above 1, products on 127.5 / 255
  size_WxH            frames (1, 1), (31, 33), (32, 32), (33, 31), (97, 65) and (16384, 2): X up to 2^22, 512 tile columns
  views_3             three views with their own view and projection matrices"""
from fractions import Fraction

import numpy as np

from scene.mesh_renderer import Lighting, MeshModel

I4 = np.eye(4)
CASES = {}
COVERED_ONCE = {}          # case -> window pixels (i, j) on shared edges that exactly one triangle must cover


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _pal(k):
    return [((37 * k) % 200 + 40) / 255.0, ((91 * k + 50) % 200 + 40) / 255.0, ((53 * k + 120) % 200 + 40) / 255.0, 1.0]


def _vertex(p, W, H):
    """ndc vertex and intended (X, Y) of a window position (x, y[, z_ndc]) in pixels."""
    x, y = p[0], p[1]
    z = p[2] if len(p) > 2 else 0.0
    X, Y = Fraction(x) * 256, Fraction(y) * 256
    assert X.denominator == 1 and Y.denominator == 1, p
    nd = [x / W * 2 - 1, y / H * 2 - 1, z]
    for n, S, want in ((nd[0], W, X), (nd[1], H, Y)):          # the float32 cast keeps the intended snap, far from a tie
        got = (Fraction(float(np.float32(n))) / 2 + Fraction(1, 2)) * S * 256
        assert abs(got - want) < Fraction(1, 8), (p, float(got), int(want))
    return nd, (int(X), int(Y))


def _model(prims, k, W, H, colors=None, **kw):
    """A model of separate primitives (k = 2 lines, 3 triangles), each with its own vertices and its own colour."""
    verts, intent, cols = [], [], []
    for n, prim in enumerate(prims):
        for p in prim:
            nd, xy = _vertex(p, W, H)
            verts.append(nd)
            intent.append(xy)
            cols.append(_pal(n) if colors is None else colors[n])
    idx = np.arange(len(verts)).reshape(-1, k)
    kw.setdefault("use_lighting", False)
    m = MeshModel(np.array(verts, np.float64).reshape(-1, 3), colors=np.array(cols).reshape(-1, 4),
                  edges=idx if k == 2 else None, faces=idx if k == 3 else None, **kw)
    m.intent = np.array(intent, np.int64).reshape(-1, 2)
    return m


def lines(segs, W, H, width=1.0, **kw):
    return _model(segs, 2, W, H, line_width=width, **kw)


def tris(ts, W, H, **kw):
    return _model(ts, 3, W, H, **kw)


def _area(t):
    (x0, y0), (x1, y1), (x2, y2) = [p[:2] for p in t]
    return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)


def ccw(*t):
    return tuple(t) if _area(t) > 0 else (t[0], t[2], t[1])


def cw(*t):
    return tuple(t) if _area(t) < 0 else (t[0], t[2], t[1])


def quad(x0, y0, x1, y1, z=0.0):
    a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
    return [(a, b, c), (a, c, d)]


def _ret(models, W, H, views=I4, projs=I4, lighting=None, background=(0.1, 0.2, 0.3), mesh_indices=None):
    return models, views, projs, W, H, lighting, background, mesh_indices


W0, H0 = 96, 70


@case
def lines_directions():
    segs = [((2.5, 3.25), (93.5, 20.75)), ((93.25, 25.5), (1.75, 40.25)), ((5.5, 1.5), (20.25, 68.5)), ((40.75, 69.0), (30.5, 0.5)),
            ((1.5, 1.5), (66.5, 66.5)), ((90.5, 2.5), (26.5, 66.5)), ((70.5, 68.5), (10.5, 8.5)), ((3.5, 60.5), (55.5, 8.5)),
            ((10.25, 5.75), (60.25, 55.75)), ((80.75, 60.25), (30.75, 10.25)), ((2.25, 10.0), (60.5, 10.0 - 1 / 256)),
            ((85.0, 2.5), (85.0 - 1 / 256, 60.25)), ((0.5, 45.5), (95.5, 45.5)), ((95.5, 50.5), (0.5, 50.5))]
    return _ret([lines(segs, W0, H0)], W0, H0)


@case
def lines_tile_edges():
    segs = []
    for c in (31.5, 32.0, 32.5, 63.5, 64.0, 64.5):
        segs.append(((1.5, c), (94.5, c)))
        segs.append(((c, 68.5), (c, 1.5)))
    for X in range(8189, 8196):                                     # x = 31.99 .. 32.01
        segs.append(((X / 256, 3.25), (X / 256, 66.75)))
    segs += [((2.5, 29.5), (30.5, 34.25)), ((30.25, 35.5), (1.5, 28.75)), ((29.5, 2.5), (34.25, 30.5)), ((34.5, 62.5), (29.75, 36.25)),
             ((33.5, 31.25), (62.5, 32.75)), ((66.5, 63.5), (94.5, 64.5))]
    return _ret([lines(segs, W0, H0, width=w) for w in (1.0, 2.0, 3.0)], W0, H0)


@case
def lines_wide():
    s33 = [((3.5, 5.5), (90.5, 5.5)), ((90.5, 2.5), (90.5, 66.5)), ((10.5, 10.5), (60.5, 60.5)), ((5.5, -40.5), (80.5, -40.5)),
           ((80.5, 120.5), (5.5, 120.5)), ((-30.5, 5.5), (-30.5, 60.5)), ((140.25, 60.5), (140.25, 5.5)), ((2.5, 66.25), (93.5, 60.75)),
           ((3.5, -16.5), (70.5, -16.25)), ((5.5, 86.5), (70.5, 86.25))]
    s70 = [((2.5, 35.5), (94.5, 35.5)), ((48.25, 1.5), (48.25, 69.0)), ((90.5, 64.5), (8.5, 4.5)), ((1.5, 104.5), (95.5, 104.75))]
    s1 = [((10.5, -0.5), (50.5, -0.5)), ((-0.5, 10.5), (-0.5, 50.5)), ((60.5, 70.5), (20.5, 70.5)), ((96.5, 60.5), (96.5, 5.5)),
          ((10.5, -0.25), (50.5, -0.75))]
    return _ret([lines(s33, W0, H0, width=33.0), lines(s70, W0, H0, width=70.0), lines(s1, W0, H0, width=1.0),
                 lines(s1, W0, H0, width=2.0)], W0, H0)


@case
def lines_far():
    W, H = 128, 64
    e = 4194278 / 256                                              # 16383.8984...: just inside the 2^14 guard band
    segs = [((-2000.5, -900.25), (2000.75, 950.5)), ((2000.5, 10.5), (-2000.5, 50.25)), ((16383.875, 16383.875), (-16383.875, -16383.875)),
            ((-e, 31.5), (e, 33.0)), ((e, 40.25), (-e, 20.75)), ((64.5, -16000.0), (70.25, 16000.0)), ((100.5, e), (90.25, -e)),
            ((-e, e), (e, -e + 64)), ((20.5, 20.5), (20.5, 20.5)), ((40.25, 10.5), (41.0, 10.75)), ((50.625, 10.5), (50.875, 10.5)),
            ((-50.5, 20.5), (-3.5, 30.5)), ((130.5, 20.5), (180.5, 40.5)), ((20.5, -40.5), (25.5, -2.5)), ((30.5, 66.5), (35.5, 90.5)),
            ((-10.5, 40.5), (10.5, 45.5)), ((120.5, 5.5), (2000.5, 300.5)), ((16384.0, 16384.0), (0.0, 0.0)),
            ((-16384.0, 10.5), (16384.0, 50.5))]
    return _ret([lines(segs, W, H, width=1.0), lines(segs, W, H, width=5.0)], W, H)


@case
def tris_hard():
    ts = [ccw((-1500.0, -1200.0, 0.5), (2000.0, -1100.0, 0.5), (100.0, 1900.0, 0.5)),
          ccw((20.25, 20.5), (44.5, 44.25), (44.25, 44.5)),                      # sliver across the tile corner (32, 32)
          ccw((58.0, 70.0, -0.1), (70.25, 58.0, -0.1), (70.0, 58.0, -0.1)),     # sliver across (64, 64)
          ccw((32.0, 32.0, -0.2), (64.0, 32.0, -0.2), (32.0, 64.0, -0.2)),      # vertices on tile corners
          ccw((31.5, 31.5, -0.3), (40.5, 31.5, -0.3), (31.5, 40.5, -0.3)),      # vertices on pixel centres
          ccw((63.5, 31.5, -0.3), (72.5, 40.5, -0.3), (63.5, 40.5, -0.3)),
          ((10.0, 10.0), (20.0, 20.0), (30.0, 30.0)), ((5.0, 5.0), (5.0, 5.0), (9.0, 9.0)),      # A == 0
          cw((50.5, 5.5, -0.5), (50.5, 25.5, -0.5), (80.5, 5.5, -0.5)),                          # A < 0
          ccw((-30.0, 10.0), (-10.0, 10.0), (-20.0, 30.0)), ccw((10.0, 80.0), (30.0, 80.0), (20.0, 100.0)),   # outside
          ccw((10.625, 10.625), (10.875, 10.625), (10.75, 10.875)),             # between pixel centres
          ccw((40.625, 3.0), (40.875, 3.0), (40.75, 60.0)),                     # between two pixel columns, 57 px high
          ccw((80.0, 50.0, -0.4), (140.0, 60.0, -0.4), (90.0, 120.0, -0.4)),    # partly outside
          ccw((-0.5, -0.5, -0.6), (0.5, -0.5, -0.6), (-0.5, 0.5, -0.6)),
          ccw((95.5, 69.5, -0.6), (96.5, 69.5, -0.6), (95.5, 70.5, -0.6)), ccw((94.5, 68.5, -0.6), (97.0, 68.5, -0.6), (94.5, 71.0, -0.6))]
    return _ret([tris(ts, W0, H0)], W0, H0)


@case
def tris_shared_edges():
    ts = [((16.0, 8.0), (32.0, 8.0), (32.0, 40.0)), ((16.0, 8.0), (32.0, 40.0), (16.0, 40.0)),       # shared edges on x = 32
          ((32.0, 8.0), (48.0, 8.0), (48.0, 40.0)), ((32.0, 8.0), (48.0, 40.0), (32.0, 40.0)),
          ccw((10.5, 50.5), (32.5, 44.5), (32.5, 66.5)), ccw((32.5, 44.5), (60.5, 50.5), (32.5, 66.5)),   # through centres, x = 32.5
          ccw((50.5, 31.5), (90.5, 31.5), (70.5, 20.5)), ccw((50.5, 31.5), (90.5, 31.5), (70.5, 43.5)),   # y = 31.5
          ccw((56.5, 56.5), (68.5, 68.5), (56.5, 68.5)), ccw((56.5, 56.5), (68.5, 56.5), (68.5, 68.5)),   # diagonal through (64, 64)
          ccw((64.0, 2.0), (80.0, 2.0), (64.0, 18.0)), ccw((64.0, 2.0), (64.0, 18.0), (52.0, 2.0))]       # on x = 64, from y = 2
    return _ret([tris(ts, W0, H0)], W0, H0)


COVERED_ONCE["tris_shared_edges"] = ([(31, j) for j in range(8, 40)] + [(32, j) for j in range(8, 40)] + [(32, j) for j in range(45, 66)] +
                                     [(i, 31) for i in range(51, 90)] + [(k, k) for k in range(57, 68)] + [(63, 5), (64, 5), (40, 20)])


@case
def depth_ties():
    near = float(np.float32(1.0 - 2.0 ** -23))                    # z_w = 1 - 2^-24: d = 2^24 - 2, the last depth kept
    red, blue = [[1.0, 0.1, 0.1, 1.0]] * 2, [[0.1, 0.1, 1.0, 1.0]] * 2
    a = tris(quad(10.0, 5.0, 60.0, 25.0, -0.5) + quad(12.0, 42.0, 58.0, 58.0, -0.5), W0, H0, colors=red + blue)
    b = tris(quad(20.0, 10.0, 70.0, 30.0, -0.5) + quad(22.0, 40.0, 68.0, 62.0, -0.5), W0, H0, colors=blue + red)
    c = lines([((2.5, 15.5, -0.5), (90.5, 15.5, -0.5)), ((2.5, 50.5, -0.5), (90.5, 50.5, -0.5)), ((40.5, 2.5, -0.5), (40.5, 68.5, -0.5))],
              W0, H0, width=3.0)
    far = lines([((5.5, 66.5, 1.0), (90.5, 66.5, 1.0)), ((5.5, 64.5, near), (90.5, 64.5, near)), ((5.5, 35.5, -1.0), (90.5, 35.5, -1.0)),
                 ((10.5, 68.5, 1.0), (80.5, 68.5, 0.0)), ((80.5, 3.5, 0.0), (10.5, 3.5, 1.0))], W0, H0, width=2.0)
    fart = tris([ccw((70.0, 40.0, 1.0), (95.0, 40.0, 1.0), (70.0, 68.0, 1.0)), ccw((72.0, 42.0, near), (90.0, 42.0, near), (72.0, 60.0, near)),
                 ccw((75.5, 3.5, 1.0), (95.0, 3.5, 0.5), (75.5, 30.0, 0.5)), ccw((1.0, 1.0, -1.0), (9.0, 1.0, -1.0), (1.0, 9.0, -1.0))], W0, H0)
    back = tris(quad(0.0, 0.0, 96.0, 62.0, near), W0, H0, colors=[[0.3, 0.3, 0.3, 1.0]] * 2)
    return _ret([a, b, c, far, fart, back], W0, H0)


def _sixty_four():
    rng = np.random.default_rng(64)
    models = []
    zs = [-0.5, -0.25, 0.0, 0.25]
    for k in range(64):
        empty = k in (0, 1, 2, 30, 31, 61, 62, 63)
        n = 0 if empty else 1 + k % 3
        prims = []
        for _ in range(n):
            z = zs[int(rng.integers(4))]
            p = [tuple(np.round(rng.uniform(-8, 104, 2) * 4) / 4) + (z,) for _ in range(3)]
            p = [(x, min(y, 78.0), z) for x, y, z in p]
            prims.append((p[0], p[1]) if k % 2 == 0 else ccw(*p))
        if empty:
            nv = 0 if k in (1, 62) else 3
            kw = dict(edges=np.zeros((0, 2), int)) if k % 2 == 0 else dict(faces=np.zeros((0, 3), int))
            m = MeshModel(np.zeros((nv, 3)), use_lighting=False, **kw)
            m.intent = np.zeros((nv, 2), np.int64) + np.array([128 * W0, 128 * H0])
        elif k % 2 == 0:
            m = lines(prims, W0, H0, width=float(1 + k % 4), colors=[_pal(k + 7 * i) for i in range(n)])
        else:
            m = tris(prims, W0, H0, colors=[_pal(k + 7 * i) for i in range(n)])
        models.append(m)
    return models


@case
def models_64():
    return _ret(_sixty_four(), W0, H0)


@case
def mesh_subset():
    return _ret(_sixty_four(), W0, H0, mesh_indices=[40, 3, 17, 3, 62, 5, 0, 33, 30, 12])


@case
def all_empty():
    ms = _sixty_four()
    return _ret([ms[0], ms[1], ms[30], ms[31], ms[62]], W0, H0)


def _scatter(n, box, W, H, seed, k, width=1.0):
    """n short primitives with vertices in box = (x0, y0, x1, y1), on a 1/4 px grid, at four depths."""
    rng = np.random.default_rng(seed)
    prims = []
    for _ in range(n):
        z = float(rng.integers(4)) * 0.125
        c = rng.uniform(box[:2], box[2:])
        p = [tuple(np.clip(np.round((c + rng.uniform(-5, 5, 2)) * 4) / 4, box[:2], box[2:])) + (z,) for _ in range(k)]
        prims.append(tuple(p) if k == 2 else ccw(*p))
    return (lines(prims, W, H, width=width) if k == 2 else tris(prims, W, H))


def _count_case(n):
    W, H = 70, 40
    return _ret([_scatter(n - 60, (-2.0, -2.0, 72.0, 42.0), W, H, n, 2, width=2.0), _scatter(60, (-2.0, -2.0, 72.0, 42.0), W, H, n + 1, 3)],
                W, H)


@case
def prims_255():
    return _count_case(255)


@case
def prims_256():
    return _count_case(256)


@case
def prims_257():
    return _count_case(257)


def _hot(n):
    W, H = 70, 40
    box = (33.0, 1.0, 62.0, 30.0)                               # inside tile (1, 0)
    return _ret([_scatter(n - 40, box, W, H, n, 2), _scatter(40, box, W, H, n + 1, 3), _scatter(5, (0.0, 0.0, 70.0, 40.0), W, H, n + 2, 2)],
                W, H)


@case
def hot_tile_300():
    return _hot(300)


@case
def hot_tile_1100():
    return _hot(1100)


@case
def dropped_rules():
    W, H = 64, 48
    n, f = 0.5, 4.0
    P = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, (f + n) / (n - f), 2 * f * n / (n - f)], [0, 0, -1, 0]], np.float64)
    V1 = np.eye(4)
    V1[2, 3] = 0.8
    v = np.array([[-0.5, -0.5, -1.0],      # 0 kept in view 0; in front of the near plane in view 1
                  [0.75, 0.45, -1.5],      # 1 kept in both
                  [0.0, 0.0, 0.5],         # 2 behind the camera: c.w < 0
                  [0.2, 0.1, 0.0],         # 3 c.w == 0
                  [0.0, 0.0, -6.0],        # 4 past the far plane in both
                  [0.1, 0.1, -0.3],        # 5 in front of the near plane
                  [600.0, 0.0, -1.0],      # 6 |x_w| > 2^14
                  [0.0, -700.0, -1.0],     # 7 |y_w| > 2^14
                  [511.0, 0.25, -1.0],     # 8 x_w == 2^14 exactly: kept
                  [0.3, -0.6, -4.6],       # 9 past the far plane in view 0 only
                  [-0.6, 0.5, -2.0],       # 10 kept in both
                  [0.9, 0.9, 0.25]])       # 11 dropped, referenced by nothing
    col = np.array([_pal(k) for k in range(len(v))])
    e = np.array([[0, 1], [0, 2], [2, 3], [1, 4], [0, 5], [1, 6], [0, 7], [10, 8], [1, 9], [10, 1], [9, 10], [3, 3], [0, 10]])
    t = np.array([[0, 1, 10], [0, 1, 2], [1, 10, 9], [0, 4, 2], [10, 1, 9], [1, 0, 10]])
    ms = [MeshModel(v, colors=col, edges=e, use_lighting=False, line_width=2.0), MeshModel(v, colors=col, faces=t, use_lighting=False)]
    return _ret(ms, W, H, views=np.stack([I4, V1]), projs=P)


def _rot_scale():
    a, b = np.deg2rad(25), np.deg2rad(-15)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    M = np.eye(4)
    M[:3, :3] = Ry @ Rx @ np.diag([1.5, 0.6, 1.1])
    M[:3, 3] = [0.01, -0.02, -0.05]
    return M


@case
def shading_persp():
    from tests.test_mesh_raster_cpu import _persp
    W, H = 64, 48
    view, proj = _persp(W, H, dist=0.3)                          # camera at z = 0.3 looking down -z: c.w = 0.3 - z
    rng = np.random.default_rng(12)
    zn, zf = 0.2, -0.7                                           # c.w = 0.1 and 1.0
    lv = np.array([[-0.03, -0.02, zn], [0.3, 0.2, zf], [0.03, -0.015, zn], [-0.35, 0.1, zf], [0.0, 0.018, zn], [0.05, -0.3, zf],
                   [-0.02, 0.0, zn], [0.02, 0.001, zn], [-0.3, -0.25, zf], [0.3, -0.2, zf]])
    le = np.array([[0, 1], [3, 2], [4, 5], [6, 7], [8, 9], [0, 9]])
    tv = np.array([[-0.035, -0.03, zn], [0.35, -0.25, zf], [-0.3, 0.3, zf], [0.03, 0.025, zn], [0.3, 0.28, zf], [-0.1, -0.3, zf]])
    tf = np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5], [3, 5, 4], [0, 3, 1], [0, 1, 3]])
    mk = lambda vv, lit, **kw: MeshModel(vv, colors=rng.uniform(0.05, 1.0, (len(vv), 4)), normals=rng.normal(size=vv.shape),
                                         use_lighting=lit, **kw)
    ms = [mk(tv, True, faces=tf, ka=0.3, kd=0.9), mk(lv, True, edges=le, line_width=3.0, ka=0.45, kd=0.7),
          mk(tv * [0.8, 0.8, 1.0], False, faces=tf), mk(lv * [1.0, -1.0, 1.0], False, edges=le, line_width=2.0),
          mk(tv, True, faces=tf, model=_rot_scale(), ka=0.2, kd=1.1), mk(lv, True, edges=le, model=_rot_scale(), ka=0.6, kd=0.6)]
    light = Lighting(light_pos=np.array([0.5, 1.0, 2.0]), ambient_color=np.array([0.3, 0.4, 0.5, 1.0]),
                     diffuse_color=np.array([0.9, 0.8, 0.7, 1.0]))
    return _ret(ms, W, H, views=view, projs=proj, lighting=light)


@case
def shading_edges():
    W, H = 40, 36
    up, down = np.tile([0.0, 0.0, 1.0], (3, 1)), np.tile([0.0, 0.0, -1.0], (3, 1))
    at = _vertex((5.5, 20.5), W, H)[0]                           # the light sits on the first vertex of the lit line
    mdl = lambda m, nrm: (setattr(m, "normals", np.asarray(nrm, np.float32)), m)[1]
    zero = mdl(tris([ccw((2.0, 2.0, 0.5), (14.0, 2.0, 0.5), (2.0, 14.0, 0.5))], W, H, use_lighting=True, ka=0.5, kd=0.5), np.zeros((3, 3)))
    away = mdl(tris([ccw((16.0, 2.0, 0.5), (30.0, 2.0, 0.5), (16.0, 14.0, 0.5))], W, H, use_lighting=True, ka=0.25, kd=0.75), up)
    toward = mdl(tris([ccw((20.0, 16.0, 0.5), (38.0, 18.0, 0.5), (22.0, 34.0, 0.25))], W, H, use_lighting=True, ka=0.25, kd=0.75), down)
    lit_line = mdl(lines([((5.5, 20.5, 0.0), (15.5, 24.5, 0.0))], W, H, width=3.0, use_lighting=True, ka=0.5, kd=0.5), up[:2])
    wild = tris([ccw((2.0, 24.0), (12.0, 24.0), (2.0, 34.0))], W, H, colors=[[-0.5, 1.7, 0.5, 1.0]])
    half = lines([((2.5, 16.5), (14.5, 16.5))], W, H, colors=[[0.5, 0.5, 0.5, 1.0]])
    lit_half = mdl(lines([((2.5, 18.5, 0.0), (14.5, 18.5, 0.0))], W, H, colors=[[1.0, 0.5, 0.25, 1.0]], use_lighting=True, ka=0.5, kd=0.0),
                   up[:2])
    light = Lighting(light_pos=np.array(at, np.float32), ambient_color=np.ones(4), diffuse_color=np.array([1.0, 0.5, 0.25, 1.0]))
    return _ret([zero, away, toward, lit_line, wild, half, lit_half], W, H, lighting=light, background=(1.2, -0.3, 0.5))


def _generic(W, H):
    s1 = [((-3.5, -2.25), (W + 4.5, H + 3.25)), ((W - 0.5, 0.5), (0.5, H - 0.5)), ((W + 10.0, H - 0.5), (-10.0, H - 0.5)),
          ((0.5, -5.0), (0.5, H + 5.0)), ((W - 0.5, H + 2.0), (W - 0.5, -2.0)), ((0.0, 0.0), (W * 1.0, H * 1.0)), ((0.5, 0.5), (W + 0.5, 0.5))]
    s3 = [((0.25, H / 2), (W - 0.25, H / 2 + 0.75)), ((W / 2, H + 1.5), (W / 2 - 0.5, -1.5)), ((-20.5, 0.5), (W + 20.5, H - 0.5))]
    ts = [((-1.0 * W, -1.0 * H, 0.5), (3.0 * W, -1.0 * H, 0.5), (-1.0 * W, 3.0 * H, 0.5)), ((0.0, 0.0, 0.25), (W * 1.0, 0.0, 0.25), (0.0, H * 1.0, 0.25)),
          ccw((W - 0.5, H - 0.5, 0.1), (W + 3.5, H - 0.5, 0.1), (W - 0.5, H + 3.5, 0.1)), ccw((W / 2, 0.0, 0.2), (W * 1.0, H / 2, 0.2), (W / 2, H * 1.0, 0.2))]
    return _ret([tris(ts, W, H), lines(s1, W, H), lines(s3, W, H, width=3.0)], W, H)


def _size_case(W, H):
    fn = lambda: _generic(W, H)
    fn.__name__ = f"size_{W}x{H}"
    return case(fn)


for _wh in ((1, 1), (31, 33), (32, 32), (33, 31), (97, 65)):
    _size_case(*_wh)


@case
def size_16384x2():
    W, H = 16384, 2
    s1 = [((0.0, 0.5), (16384.0, 1.5)), ((16384.0, 1.75), (0.0, 0.25)), ((16380.5, 0.5), (16384.0, 0.5)), ((16383.5, -3.0), (16383.5, 5.0)),
          ((8192.0, 4.0), (8192.0, -2.0)), ((8191.5, 0.5), (8192.5, 1.5)), ((0.5, 1.5), (3.5, 1.5)), ((16384.0, -16384.0), (0.0, 16384.0)),
          ((-16384.0, 1.25), (16384.0, 0.75))]
    s3 = [((5000.5, 1.5), (11000.5, 1.5)), ((16383.5, 0.5), (16370.5, 1.5)), ((31.5, -2.0), (32.5, 4.0))]
    ts = [((0.0, 0.0, 0.5), (16384.0, 0.0, 0.5), (16384.0, 2.0, 0.5)), ccw((16382.0, 0.0), (16384.0, 0.0), (16383.0, 2.0)),
          ccw((-16384.0, -16384.0, 0.25), (4000.0, 1.0, 0.25), (-16384.0, 16384.0, 0.25)), ccw((8180.0, 0.0, 0.1), (8200.0, 0.0, 0.1), (8190.0, 2.0, 0.1))]
    return _ret([tris(ts, W, H), lines(s1, W, H), lines(s3, W, H, width=3.0)], W, H)


@case
def views_3():
    models = lines_directions()[0] + tris_hard()[0] + [lines_tile_edges()[0][1]]
    views, projs = np.stack([I4] * 3), np.stack([I4] * 3)
    views[1, :3, 3] = [0.125, -0.0625, 0.25]
    views[2, :3, 3] = [-0.5, 0.375, -0.125]
    views[2, 0, 1] = 0.25                                         # a shear: x_e = x + y / 4
    projs[1] = np.diag([1.25, 0.75, 1.0, 1.0])
    projs[2] = np.diag([-0.5, 2.0, 0.5, 1.0])                     # mirrored in x: every triangle changes its winding
    return _ret(models, W0, H0, views=views, projs=projs)


_expected = {}


def expected(name):
    """The brute-force reference of a case, computed once per session and shared by the CPU and GPU tests (read only)."""
    if name not in _expected:
        from tests.mesh_raster_reference import reference
        models, views, projs, W, H, light, bg, sel = CASES[name]()
        _expected[name] = reference(models, views, projs, W, H, light, bg, sel)
    return _expected[name]
