"""Hard inputs of the neighbour searches (csrc/hgs_knn.hip: distCUDA2, hgs_knn3, hgs_radius_pairs, hgs_nearest_distance_f64).
Shared by tests/test_knn_hard_cpu.py and tests/test_knn_hard_gpu.py; the references are in tests/knn_reference.py.

Every point-cloud family is a function (P, seed) -> float32 [P, 3].  What each one stresses in the grid search of distCUDA2
(a grid of 8^L Morton cells over the bounding box that always contains the origin, a cube range of +-r per lane):

  plane_z0       z = 0: one axis has no extent -- 0/0 in the quantisation, +-r/0 in the cube range
  plane_off      z = 0.7: no zero extent (the box holds the origin), every point at cell coordinate 1023 of one axis
  line           y = z = 0: two axes without extent
  all_same       P copies of one point: r = 0 everywhere
  all_origin     P copies of the origin: every extent is zero
  far_small      N(100, 0.01^2): the whole cloud in one or two cells at every level, coordinates >> distances
  clusters       two N(+-5 e_x, 0.01^2) halves and 5 points of N(0, 50^2): nearly every cell empty, lanes whose radius reaches all
  lattice_holes  a lattice with spacings 2^-4, 2^-3, 2^-5 (exact in float32), >= 5 % of its sites missing: real ties, cell faces
  aniso          N(0, 1) * (1, 1e-3, 1e-6): extents six decades apart
  octants        N(0, 1): the origin inside the cloud, negative coordinates
  dup3 / dup5    every point 3 / 5 times: two zero distances and a real one / r = 0 with a full cell
  tiny           N(0, 1) * 1e-15: squared distances of 1e-33 .. 1e-30 (normal numbers)
  strands        25-point curved polylines: what the project feeds it
  non_finite     a blob with six rows spoiled by NaN, +Inf, -Inf, a whole-NaN row, -NaN (NON_FINITE_ROWS)
"""
import numpy as np


def _rng(seed):
    return np.random.default_rng(seed)


def plane_z0(P, seed):
    p = np.zeros((P, 3), np.float32)
    p[:, :2] = _rng(seed).uniform(-1, 1, size=(P, 2))
    return p


def plane_off(P, seed):
    p = plane_z0(P, seed)
    p[:, 2] = np.float32(0.7)
    return p


def line(P, seed):
    p = np.zeros((P, 3), np.float32)
    p[:, 0] = _rng(seed).uniform(-1, 1, size=P)
    return p


def all_same(P, seed):
    return np.tile(np.array([0.3, -0.1, 0.8], np.float32), (P, 1))


def all_origin(P, seed):
    return np.zeros((P, 3), np.float32)


def far_small(P, seed):
    return (100.0 + 0.01 * _rng(seed).normal(size=(P, 3))).astype(np.float32)


def clusters(P, seed):
    r = _rng(seed)
    p = 0.01 * r.normal(size=(P, 3))
    h = (P - 5) // 2
    p[:h, 0] += 5.0
    p[h:P - 5, 0] -= 5.0
    p[P - 5:] = 50.0 * r.normal(size=(5, 3))
    return p.astype(np.float32)


def lattice_holes(P, seed):
    n = 2
    while n ** 3 * 0.95 < P:
        n += 1
    i = np.stack(np.meshgrid(*(np.arange(n) - n // 2,) * 3, indexing="ij"), -1).reshape(-1, 3)
    i = i[_rng(seed).permutation(i.shape[0])[:P]]          # P of the n^3 sites, in random order: the others are the holes
    return (i * np.array([2.0 ** -4, 2.0 ** -3, 2.0 ** -5])).astype(np.float32)


def aniso(P, seed):
    return (_rng(seed).normal(size=(P, 3)) * np.array([1.0, 1e-3, 1e-6])).astype(np.float32)


def octants(P, seed):
    return _rng(seed).normal(size=(P, 3)).astype(np.float32)


def _dup(P, seed, k):
    u = _rng(seed).normal(size=((P + k - 1) // k, 3)).astype(np.float32)
    p = np.repeat(u, k, axis=0)[:P]
    return p[_rng(seed + 1).permutation(P)]


def dup3(P, seed):
    return _dup(P, seed, 3)


def dup5(P, seed):
    return _dup(P, seed, 5)


def tiny(P, seed):
    return (_rng(seed).normal(size=(P, 3)) * 1e-15).astype(np.float32)


def strands(P, seed, V=25):
    """Points of short curved polylines, V per strand: roots on a sphere of radius 0.1, 4 mm steps along a direction that turns."""
    r = _rng(seed)
    S = (P + V - 1) // V
    root = r.normal(size=(S, 3))
    root = 0.1 * root / np.linalg.norm(root, axis=1, keepdims=True)
    d = root / 0.1 + 0.3 * r.normal(size=(S, 3))
    bend = 0.15 * r.normal(size=(S, 3))
    pts = [root]
    for _ in range(V - 1):
        d = d + bend
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(pts[-1] + 0.004 * d)
    return np.stack(pts, 1).reshape(-1, 3)[:P].astype(np.float32)


NON_FINITE_ROWS = (7, 500, 1023, 1024, 2000, 2999)


def _spoil(p, rows):
    """Six kinds of non-finite rows, cycled over `rows`."""
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    for k, row in enumerate(rows):
        k %= 6
        if k == 0:
            p[row, 0] = np.nan
        elif k == 1:
            p[row, 1] = np.inf
        elif k == 2:
            p[row, 2] = -np.inf
        elif k == 3:
            p[row] = np.nan
        elif k == 4:
            p[row, 1] = neg_nan
        else:
            p[row, 0], p[row, 2] = np.inf, -np.inf
    return p


def non_finite(P=3000, seed=0, rows=NON_FINITE_ROWS):
    p = (_rng(seed).normal(size=(P, 3)) * 0.2 + np.array([0.3, -0.1, 0.8])).astype(np.float32)
    return _spoil(p, [r for r in rows if r < P])


FAMILIES = {f.__name__: f for f in (plane_z0, plane_off, line, all_same, all_origin, far_small, clusters, lattice_holes, aniso,
                                    octants, dup3, dup5, tiny, strands, non_finite)}
# the small size of every family: 3000 .. 9000 points (the grid's levels 2 and 3), 300 for the single-point clouds
SMALL = {"plane_z0": 4000, "plane_off": 4000, "line": 3000, "all_same": 300, "all_origin": 300, "far_small": 5000,
         "clusters": 6005, "lattice_holes": 4500, "aniso": 4000, "octants": 9000, "dup3": 3000, "dup5": 8500, "tiny": 3000,
         "strands": 5000, "non_finite": 3000}
NAMES = list(FAMILIES)
# where cellgrid_level (csrc/hgs_cellgrid.h) changes the grid (1024, 8192, 65536), one below each; 8192 and 65536 are exact pad_pow2 sizes as well
LARGE_SIZES = (1023, 1024, 8191, 8192, 65535, 65536)
LARGE_FAMILIES = ("octants", "strands", "clusters", "far_small")


def small(name):
    return FAMILIES[name](SMALL[name], 100 + NAMES.index(name))


def large(name, P):
    return FAMILIES[name](P, 200 + NAMES.index(name))


def margin_cloud():
    """Seven points on which the cube range of distCUDA2 needs its 1.000001 margin.  Point 0 (and its copies 1, 2) at x > 0 has
    its third neighbour, point 4, in the OTHER cell of the level-1 grid: x4 < 0 is the last float below the cell boundary, and
    the difference t = x0 - x4 is not a float32 -- it rounds DOWN to a, so the squared distance a a that makes point 4 the third
    neighbour gives the radius sqrt(a a) = a < t, and x0 - a rounds to the first float ABOVE x4 (floats are denser there), on
    the other side of the boundary.  Point 3, in point 0's own cell, is one ulp farther than point 4; points 5 and 6 fix the
    bounding box.  tests/test_knn_hard_cpu.py checks each of these statements with the quantisation's own expression."""
    bits = [[1050253722, 0, 0], [1050253722, 0, 0], [1050253722, 0, 0], [1050255771, 1050388859, 0], [3145988161, 0, 0],
            [3212836864, 0, 0], [1065185444, 1148846080, 0]]
    return np.array(bits, np.uint32).view(np.float32)


# ---- hgs_knn3 ----------------------------------------------------------------------------------------------------------
KNN3_FAMILIES = ("lattice_holes", "far_small", "tiny", "dup3", "clusters", "non_finite")
KNN3_SIZES = (255, 256, 257, 512, 513, 3000)


KNN3_NON_FINITE_ROWS = (3, 100, 254, 255, 256, 200, 511, 512)


def knn3_case(name, n):
    """The family at n points (non_finite: spoiled rows on both sides of the first two tile boundaries)."""
    seed = 300 + NAMES.index(name) + n
    if name == "non_finite":
        return non_finite(n, seed, KNN3_NON_FINITE_ROWS)
    return FAMILIES[name](n, seed)


def knn3_non_finite_rows(n):
    return [r for r in KNN3_NON_FINITE_ROWS if r < n]


def knn3_tile_ties():
    """600 points with one group of exact duplicates at indices 254..258 and another at 510..514: the three nearest of every
    member are decided by index alone, across the 256-point tile boundaries of hgs_knn3."""
    p = _rng(41).normal(size=(600, 3)).astype(np.float32)
    p[254:259] = p[254]
    p[510:515] = p[510]
    return p


# ---- hgs_radius_pairs ---------------------------------------------------------------------------------------------------
def _unit(r, n):
    d = r.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _blob_pairs(n, seed):
    r = _rng(seed)
    pos = r.random((n, 3)).astype(np.float32)
    d = pos[:, None, :].astype(np.float64) - pos[None, :, :]
    d = np.sqrt((d * d).sum(-1))
    np.fill_diagonal(d, np.inf)
    return pos, _unit(r, n), float(np.float32(np.median(d.min(axis=1))))


def pair_cases():
    """name -> (pos [N, 3], dir [N, 3], radius, min_cos, bidirectional, on_lattice).  on_lattice: many pairs sit exactly on a
    threshold (d2 == r2, dot == min_cos), in float32 and in float64 alike."""
    out = {}
    r = _rng(51)
    # 600 ends inside a ball of diameter radius / 2: all 179 700 pairs, against the callers' first capacity of 2400
    c = r.normal(size=(600, 3))
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * r.random((600, 1)) ** (1 / 3)
    ball = (np.array([0.4, -0.2, 0.1]) + 0.25 * 0.02 * c).astype(np.float32)
    dirs = _unit(r, 600)
    out["dense_ball"] = (ball, dirs, 0.02, -1.0, False, False)
    out["dense_ball_bidir"] = (ball, dirs, 0.02, 0.3, True, False)
    # coordinates on multiples of 2^-6 with radius 2^-5, direction components on multiples of 1/4 with min_cos = 1/4
    pos = (r.integers(0, 16, size=(1500, 3)) * 2.0 ** -6).astype(np.float32)
    dirs = (r.integers(-4, 5, size=(1500, 3)) * 0.25).astype(np.float32)
    out["on_the_radius"] = (pos, dirs, 2.0 ** -5, 0.25, False, True)
    out["on_the_radius_bidir"] = (pos, dirs, 2.0 ** -5, 0.25, True, True)
    # 300 ends on each plane x = k radius, k = 0..9, every plane holding the same 300 (y, z) sites of a radius / 4 lattice in
    # another order: every end has a partner at exactly the radius on each neighbouring plane, and sorted by x the planes'
    # runs of equal keys straddle the 256-point tiles
    rad = 2.0 ** -4
    sites = r.permutation(64 * 64)[:300]
    yz = np.stack([sites // 64, sites % 64], 1) * (rad / 4)
    planes = []
    for k in range(10):
        q = np.empty((300, 3))
        q[:, 0] = k * rad
        q[:, 1:] = yz[r.permutation(300)]
        planes.append(q)
    pos = np.concatenate(planes).astype(np.float32)
    pos = pos[r.permutation(pos.shape[0])]
    out["x_planes"] = (pos, _unit(r, pos.shape[0]), rad, -1.0, False, True)
    # two ends exactly the radius apart (the median nearest-neighbour distance of the two), facing each other: the one pair is kept,
    # its distance test decided on equality
    two = np.array([[0.25, 0.5, 0.125], [0.25 + 2.0 ** -6, 0.5, 0.125]], np.float32)
    out["blob_2"] = (two, np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], np.float32), 2.0 ** -6, 0.3, False, True)
    for n in (255, 256, 257, 513):
        pos, dirs, rad_n = _blob_pairs(n, 60 + n)
        out[f"blob_{n}"] = (pos, dirs, rad_n, 0.3, n % 2 == 0, False)
    out["identical_300"] = (np.tile(np.array([0.25, 0.5, -0.125], np.float32), (300, 1)), _unit(r, 300), 0.01, 0.3, True, False)
    return out


PAIR_NAMES = ["dense_ball", "dense_ball_bidir", "on_the_radius", "on_the_radius_bidir", "x_planes", "blob_2", "blob_255",
              "blob_256", "blob_257", "blob_513", "identical_300"]


def merge_cluster_strands():
    """64 three-vertex strands whose tips lie within a quarter of merge_dist_th_init (2 mm) of one point, their last segments
    within a few degrees of +-x, their roots scattered: with bidirectional_merge every pair of tips is a merge candidate -- 2016
    pairs against the first capacity of 1024 in _merge_candidates_device.  Returns (points [64, 3, 3], roots [64, 3])."""
    r = _rng(71)
    S = 64
    c = r.normal(size=(S, 3))
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * r.random((S, 1)) ** (1 / 3)
    tip = np.array([0.2, 0.3, 0.1]) + 0.25 * 2e-3 * c          # within 0.5 mm of the point: any two tips within 1 mm
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)[:, None]
    d = np.array([1.0, 0.0, 0.0]) + 0.03 * r.normal(size=(S, 3))
    d = sign * d / np.linalg.norm(d, axis=1, keepdims=True)
    mid = tip - 0.01 * d
    root = mid - 0.01 * d + 0.3 * r.normal(size=(S, 3)) * np.array([0.0, 1.0, 1.0])
    pts = np.stack([root, mid, tip], 1).astype(np.float32)
    return pts, pts[:, 0].copy()


# ---- hgs_nearest_distance_f64 -------------------------------------------------------------------------------------------
NEAREST_N = (1, 255, 256, 257)
NEAREST_M = (1023, 1024, 1025, 2048, 2049)


def nearest_case(N, M):
    """(points float32 [N, 3], references float64 [M, 3]) with what a float32 kernel gets wrong: points near 1e4 whose two
    nearest references are 1e-9 apart in distance (the LAST references, so that the winner sits in the last LDS tile), references
    that are exact copies of points (distance 0), and one reference at 1e6."""
    r = _rng(1000 * N + M)
    pts = r.normal(size=(N, 3)).astype(np.float32)
    refs = r.normal(size=(M, 3))
    far = np.arange(0, N, 5)                                   # every fifth point moves out to 1e4
    pts[far] = (1e4 + r.normal(size=(far.shape[0], 3))).astype(np.float32)
    refs[0] = (1e6, -1e6, 1e6)
    k = min(N // 3 + 1, M // 4)
    refs[1:1 + k] = pts[:k].astype(np.float64)                 # exact copies: distance 0
    p0 = pts[far[-1]].astype(np.float64)
    refs[M - 2] = p0 + np.array([0.01 + 1e-9, 0.0, 0.0])
    refs[M - 1] = p0 + np.array([0.0, 0.01, 0.0])
    if far[-1] < k:                                            # (its copy among the references would win at distance 0)
        refs[1 + far[-1]] = p0 + np.array([0.0, 0.0, 5.0])
    return pts, refs
