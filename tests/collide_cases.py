"""Fields, strands and parameters of the head push-out's tests (tests/test_collide_cpu.py, tests/test_collide_gpu.py): the smallest
at which hgs_strand_collide (csrc/hgs_collide.hip) and the numpy path of scene/strand_collide.py can go wrong.  A case is
(points float32 [P, 3], offsets int64 [K + 1], field name, margin, skin or None, iters)."""
import functools

import numpy as np

KS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)     # strand counts: around a wave and a workgroup of 256, and several workgroups


# ---- fields --------------------------------------------------------------------------------------------------------------------
def sphere_field(grid, pad=0.5, radius=1.0):
    """The exact distance to the sphere of `radius` about 0 on the contract's box for it: origin = -(radius + 2 pad radius) an axis,
    grid^3 nodes.  An odd grid has a node at the centre."""
    from utils.head_sdf import HeadSDF
    lo = -(radius + pad * 2.0 * radius)
    h = -2.0 * lo / (grid - 1)
    ax = lo + h * np.arange(grid)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return HeadSDF(np.array([lo, lo, lo]), h, (grid, grid, grid), (np.sqrt(x * x + y * y + z * z) - radius).astype(np.float32))


def tiny_field():
    """2 x 2 x 2 nodes, one cell: a slope along x with a twist, negative at x = 0."""
    from utils.head_sdf import HeadSDF
    phi = np.array([[[-0.5, 0.5], [-0.25, 0.75]], [[-0.375, 0.625], [-0.125, 0.5]]], np.float32)
    return HeadSDF(np.array([0.0, 0.0, 0.0]), 1.0, (2, 2, 2), phi)


def slab_field():
    """3 x 5 x 4 nodes (nx, ny, nz): an off-centre ball in a box that is no cube, odd origin and spacing: a swapped axis shows."""
    from utils.head_sdf import HeadSDF
    shape, origin, h = (3, 5, 4), np.array([-0.31, -0.73, -0.47]), 0.3
    z, y, x = np.meshgrid(*(origin[k] + h * np.arange(shape[k]) for k in (2, 1, 0)), indexing="ij")
    phi = np.sqrt((x - 0.02) ** 2 + (y + 0.11) ** 2 + (z + 0.03) ** 2) - 0.37
    return HeadSDF(origin, h, shape, phi.astype(np.float32))


def flat_field():
    """4 x 4 x 4 nodes, h = 1 from 0: -0.25 at the eight corners of the cell [1, 2]^3 (the gradient is exactly zero all over it) and
    at the nodes with x = 0, rising by one a node along x elsewhere."""
    from utils.head_sdf import HeadSDF
    phi = np.empty((4, 4, 4), np.float32)
    phi[:] = (np.arange(4, dtype=np.float32) - 0.25)[None, None, :]
    phi[1:3, 1:3, 1:3] = -0.25
    return HeadSDF(np.array([0.0, 0.0, 0.0]), 1.0, (4, 4, 4), phi)


@functools.lru_cache(maxsize=None)
def field(name):
    if name.startswith("sphere"):
        return sphere_field(int(name[6:]))
    return {"tiny": tiny_field, "slab": slab_field, "flat": flat_field}[name]()


# ---- strands ---------------------------------------------------------------------------------------------------------------------
def _pack(strands):
    """(points float32 [P, 3], offsets int64 [K + 1]) of a list of [n, 3] arrays (n >= 0)."""
    n = [len(s) for s in strands]
    pts = np.concatenate([np.asarray(s, np.float64).reshape(-1, 3) for s in strands] + [np.zeros((0, 3))]).astype(np.float32)
    return pts, np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def _line(a, b, n):
    return np.asarray(a, np.float64)[None, :] + np.linspace(0.0, 1.0, n)[:, None] * (np.asarray(b, np.float64) - np.asarray(a, np.float64))[None, :]


def special_strands():
    """On a sphere field of radius 1 in the box [-2, 2]^3: the joints and paths that take every branch of the contract."""
    nan, inf = np.nan, np.inf
    through = _line([-1.6, 0.2, 0.1], [1.6, 0.3, -0.2], 17)                  # enters and leaves
    s = [
        through,
        np.concatenate([through, _line([1.6, 0.5, -0.2], [-0.2, 0.4, 0.3], 9)]),                       # enters the head twice
        _line([0.1, 0.2, -0.3], [0.5, -0.1, 0.2], 7),                                                  # wholly inside
        _line([0.3, 0.3, 0.3], [1.7, 1.2, 0.9], 12),                                                   # a root inside, the tip outside
        _line([1.01, 0.0, 0.0], [0.99, 0.9, 0.0], 8),                                                  # grazes the margin
        np.array([[1.5, 0, 0], [1.2, 0, 0], [0.8, 0, 0], [0.8, 0, 0], [0.8, 0, 0], [0.4, 0.1, 0], [0.4, 0.1, 0]]),   # duplicates, L == 0, inside
        np.array([[1.5, 1.5, 0], [1.5, 1.5, 0], [1.4, 1.5, 0], [1.4, 1.5, 0]]),                                      # duplicates outside
        np.array([[1.5, 0, 0], [0.7, 0.1, 0.1], [nan, 0.2, 0.1], [0.5, 0.3, 0.1], [0.4, 0.5, 0.1]]),                 # a NaN behind a hit
        np.array([[1.5, 0, 0], [1.4, 0.1, 0.1], [1.3, inf, 0.1], [0.5, 0.3, 0.1], [0.4, 0.5, 0.1]]),                 # an inf before any hit
        np.array([[1.5, 0, 0], [0.6, 0.1, 0.1], [-inf, 0.2, 0.1], [0.5, 0.3, 0.1]]),                                 # an inf behind a hit
        np.array([[1.9, 1.9, 1.9], [2.0, 2.0, 2.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0], [0.5, 0.5, 0.5]]),   # t == n - 1: out of range
        np.array([[1.2, 1.2, 1.2], [5.0, 5.0, 5.0], [-2.001, 0.0, 0.0], [0.2, 0.2, 0.2], [0.0, -7.0, 0.0]]),         # outside the box, and back in
        np.array([[1.5, 0, 0], [0.75, 0, 0], [0.0, 0.0, 0.0], [-0.5, 0.0, 0.0]]),                                    # through the centre node
        np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.25, 0.0, 0.0]]),                                              # rooted at the centre
        np.array([[1.5, 0.0, 0.0], [1e30, 0.0, 0.0], [0.5, 0.0, 0.0]]),                                              # a segment too long for the box
        np.array([[1.5, 0.0, 0.0], [0.5, 0.0, 0.0], [3e38, 3e38, 3e38], [0.5, 0.1, 0.0]]),                           # the largest float32 magnitudes behind a hit
        np.zeros((0, 3)), np.array([[0.2, 0.1, 0.0]]), np.array([[nan, 0.0, 0.0]]), np.zeros((0, 3)),                 # 0 and 1 joints
        _line([1.3, -0.4, 0.2], [0.2, 0.9, -0.3], 2),                                                  # 2 joints
    ]
    return _pack(s)


def ragged_strands(seed=3):
    """Strands of 0, 1, 2, ... 40 joints in one call, an empty strand after every third one, through a sphere of radius 1."""
    rng = np.random.default_rng(seed)
    out = []
    for n in range(41):
        a = rng.normal(size=3)
        a = 1.4 * a / np.linalg.norm(a)
        b = -a + 0.8 * rng.normal(size=3)
        wobble = 0.05 * rng.normal(size=(n, 3))
        out.append(_line(a, b, n) + wobble if n else np.zeros((0, 3)))
        if n % 3 == 2:
            out.append(np.zeros((0, 3)))
    return _pack(out)


@functools.lru_cache(maxsize=None)
def counted_strands(K=1000, seed=5):
    """K strands of 0 to 9 joints (ragged, about a tenth empty) across the box of a sphere field of radius 1: about half dip in.
    The first k strands of it are the case of k strands."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 10, size=K)
    out = []
    for k in range(K):
        a = rng.uniform(-1.6, 1.6, size=3)
        b = rng.uniform(-1.6, 1.6, size=3)
        out.append(_line(a, b, n[k]) + 0.03 * rng.normal(size=(n[k], 3)) if n[k] else np.zeros((0, 3)))
    return _pack(out)


def first_strands(points, offsets, K):
    return points[:offsets[K]], offsets[:K + 1]


def box_strands(sdf, K, n, seed):
    """K strands of n joints between random places of the field's box widened by a fifth."""
    rng = np.random.default_rng(seed)
    lo = sdf.origin
    span = (np.array(sdf.shape) - 1) * sdf.spacing
    out = []
    for _ in range(K):
        a, b = (lo - 0.1 * span + rng.random(3) * 1.2 * span for _ in range(2))
        out.append(_line(a, b, n))
    return _pack(out)


def flat_strands():
    """On the flat field: a strand into the cell of zero gradient (its joints there stay inside and are counted), and one that the
    slope along x pushes out."""
    return _pack([np.array([[3.5, 1.5, 1.5], [2.5, 1.5, 1.5], [1.5, 1.5, 1.5], [1.25, 1.75, 1.5], [1.75, 1.25, 1.25]]),
                  np.array([[0.9, 0.5, 0.5], [0.6, 0.5, 0.5], [0.1, 0.4, 0.6], [0.05, 0.2, 0.6]])])


PARAMETERS = ((0.0, None, 8), (0.05, None, 8), (0.05, 0.0, 1), (0.0, 0.0, 32), (0.05, None, 32), (0.0, None, 1))   # (margin, skin, iters)


@functools.lru_cache(maxsize=None)
def hard_cases():
    """name -> case."""
    cases = {}
    sp, so = special_strands()
    for m, s, it in PARAMETERS:
        cases[f"special_m{m}_s{s}_i{it}"] = (sp, so, "sphere9", m, s, it)
    cases["special_fine_grid"] = (sp, so, "sphere24", 0.02, None, 8)
    rp, ro = ragged_strands()
    cases["ragged"] = (rp, ro, "sphere9", 0.0, None, 8)
    cases["ragged_margin_i1"] = (rp, ro, "sphere9", 0.05, 0.0, 1)
    cases["ragged_fine_grid_i32"] = (rp, ro, "sphere24", 0.02, None, 32)
    cases["tiny"] = (*box_strands(tiny_field(), 40, 6, 1), "tiny", 0.0, None, 8)
    cases["tiny_margin"] = (*box_strands(tiny_field(), 40, 6, 2), "tiny", 0.1, 0.0, 32)
    cases["slab"] = (*box_strands(slab_field(), 70, 9, 3), "slab", 0.0, None, 8)
    cases["slab_margin"] = (*box_strands(slab_field(), 70, 9, 4), "slab", 0.04, None, 4)
    cases["flat"] = (*flat_strands(), "flat", 0.0, None, 8)
    cases["no_strands"] = (np.zeros((0, 3), np.float32), np.zeros(1, np.int64), "sphere9", 0.0, None, 8)
    cases["empty_strands_only"] = (np.zeros((0, 3), np.float32), np.zeros(4, np.int64), "sphere9", 0.0, None, 8)
    return cases


HARD_NAMES = ("special_m0.0_sNone_i8", "special_m0.05_sNone_i8", "special_m0.05_s0.0_i1", "special_m0.0_s0.0_i32", "special_m0.05_sNone_i32",
              "special_m0.0_sNone_i1", "special_fine_grid", "ragged", "ragged_margin_i1", "ragged_fine_grid_i32", "tiny", "tiny_margin", "slab",
              "slab_margin", "flat", "no_strands", "empty_strands_only")
COUNTED = ("sphere9", 0.03, None, 8)              # field, margin, skin, iters of the strand-count cases


# ---- the analytic head ---------------------------------------------------------------------------------------------------------------
SPHERE_GRIDS = (24, 32, 64)
SPHERE_MARGINS = (0.0, 0.02)
SPHERE_ITERS = (4, 8)


@functools.lru_cache(maxsize=None)
def sphere_scene(seed=7, K=60, n=32):
    """60 strands of 32 points around the unit sphere: rooted just outside the largest margin, each runs 1.2 units along a random tangent
    tilted into (< 0) or away from the sphere by a factor drawn from [-0.4, 0.3], and is bent inward."""
    rng = np.random.default_rng(seed)
    out = []
    s = np.linspace(0.0, 1.2, n)[:, None]
    for _ in range(K):
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        t = np.cross(nrm, rng.normal(size=3))
        t /= np.linalg.norm(t)
        d = t + rng.uniform(-0.4, 0.3) * nrm
        d /= np.linalg.norm(d)
        out.append(1.03 * nrm[None, :] + s * d[None, :] - 0.25 * s * s * nrm[None, :])
    return _pack(out)
