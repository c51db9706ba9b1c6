"""Strands and tolerances of the strand simplification's tests (tests/test_simplify_cpu.py, tests/test_simplify_gpu.py): the smallest
at which hgs_strand_simplify (csrc/hgs_strand_simplify.hip) and the numpy path of scene/strand_simplify.py can go wrong.  Inputs only.
A case is (points float32 [P, 3], offsets int64 [K + 1], tol)."""
import functools

import numpy as np

from tests.smooth_cases import _pack, first_strands, jittered  # noqa: F401  (first_strands: for the tests)

# joints per strand: none, SHORT and the smallest OK strand, around one, two and sixteen chunks of 64, the last eligible and the first LONG
EDGE_N = (0, 1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025)
KS = (0, 1, 3, 4, 5, 64, 65, 257)                 # strand counts: wavefronts past K, partial workgroups, many workgroups
TOL = 3e-4                                        # a hair's width against the jittered helices' 2 mm a joint
# the LDS slice is 48 * max_joints + 128 bytes: four wavefronts a workgroup up to 338 joints, two up to 680, then one; and the sizes
# tests/test_smooth_gpu.py takes for its own thresholds
SLOTS = (None, 140, 338, 339, 409, 410, 680, 681, 819, 820, 1024)
REFUSED = (-1.0, -1e-300, float("nan"), float("inf"), -float("inf"), "wide", None)


# ---- single strands ----------------------------------------------------------------------------------------------------------------
def straddle():
    """130 joints on integer coordinates: straight along x to joint 60, along y to joint 70, along x again.  With tol = 0.5 the only
    inner joints that are kept are 60 and 70, and the interval (60, 70) lies across lanes 63 | 64."""
    j = np.arange(130)
    return np.stack([np.where(j <= 60, j, np.where(j <= 70, 60, j - 10)), np.clip(j - 60, 0, 10), np.zeros(130)], axis=1).astype(np.float64)


def straddle_bump():
    """straddle() with joint 64 moved 2 off the segment from joint 60 to joint 70: the winner of that interval is joint 64 exactly."""
    s = straddle()
    s[64] = [62.0, 4.0, 0.0]
    return s


def collinear(n=129):
    """n joints j * (1, 2, -1) from (3, -5, 7): with n - 1 a power of two t = j / (n - 1) is exact, and so is every d2 == 0."""
    return np.array([3.0, -5.0, 7.0]) + np.arange(n)[:, None] * np.array([1.0, 2.0, -1.0])


def closed_loop(n=41, r=5.0):
    """A circle whose last joint is its first (a == b for the interval (0, n - 1): L2 = 0, t = 0, d2 = |p - a|^2)."""
    a = 2.0 * np.pi * np.arange(n) / (n - 1)
    s = np.stack([r * np.cos(a), r * np.sin(a), 0.1 * np.arange(n)], axis=1)
    s[-1] = s[0]
    return s


def hairpin():
    """Out along x to 10, back past the root to -8 a little above, forward again to -5: against the chord from the root to the tip t
    clamps to 0 for the joints on the way out and to 1 for those beyond the tip."""
    out = [[x, 0.0, 0.0] for x in range(0, 11)]
    back = [[x, 0.25, 0.0] for x in range(9, -9, -1)]
    fwd = [[x, 0.5, 0.0] for x in range(-7, -4)]
    return np.array(out + back + fwd, np.float64)


def chain(n=36):
    """p_j = 0.1^j (cos(j pi / 2), sin(j pi / 2), 0): a square spiral shrinking tenfold a joint.  With tol = 0 every interval's
    farthest joint is the one next to its left end: the recursion is n - 2 deep and keeps every joint."""
    turn = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    return turn[np.arange(n) % 4] * (0.1 ** np.arange(n))[:, None]


SHAPES = ("straddle", "straddle_bump", "closed_loop", "hairpin", "collinear", "square")


@functools.lru_cache(maxsize=None)
def shape_strands():
    """One strand per name of SHAPES, in that order; coordinates of order 1 to 100, for tol = 0.5."""
    square = [[0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0], [0, 0, 0]]
    return _pack([straddle(), straddle_bump(), closed_loop(), hairpin(), collinear(), square])


@functools.lru_cache(maxsize=None)
def nonfinite_strands():
    """Strands of 6, 70 and 130 joints with one NaN or infinity: in an end joint, in the middle, in the second chunk; between OK strands."""
    rng = np.random.default_rng(11)
    strands = []
    for n, at, c, value in ((6, 3, 1, np.nan), (6, 0, 0, np.inf), (70, 69, 2, -np.inf), (130, 64, 0, np.nan), (130, 129, 1, np.inf)):
        s = jittered(n, rng)
        s[at, c] = value
        strands += [jittered(20, rng), s]
    return _pack(strands)


@functools.lru_cache(maxsize=None)
def tie_strands():
    """300 strands of 2 to 140 joints on integer coordinates in [-3, 3]: many joints of an interval share its largest d2."""
    rng = np.random.default_rng(5)
    return _pack([rng.integers(-3, 4, size=(int(n), 3)) for n in rng.integers(2, 141, size=300)])


# ---- launches ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_strands():
    """One strand of every size of EDGE_N, in that order."""
    rng = np.random.default_rng(3)
    return _pack([jittered(n, rng) for n in EDGE_N])


@functools.lru_cache(maxsize=None)
def mixed_strands():
    """3-joint and 1024-joint strands side by side: the longest sizes the LDS slice for all (one wavefront a workgroup)."""
    rng = np.random.default_rng(4)
    return _pack([jittered(n, rng) for n in (3, 1024, 3, 3, 1024, 3, 1024)])


@functools.lru_cache(maxsize=None)
def pool_strands():
    """300 ragged strands of 0 to 140 joints: the first of them 0, 1, 2, 3 and 130 joints long, one with a NaN, jittered helices with
    a straight strand, a smooth one and one on integer millimetres in every ten."""
    rng = np.random.default_rng(7)
    sizes = [0, 1, 2, 3, 130] + [int(v) for v in rng.integers(0, 141, size=295)]
    sizes[9] = 20
    strands = []
    for s, n in enumerate(sizes):
        if s % 10 == 6:
            strands.append(np.array([0.01, 0.02, 0.03]) + 2e-3 * np.arange(n)[:, None] * np.array([0.6, 0.0, -0.8]))
        elif s % 10 == 7:
            strands.append(jittered(n, rng, sigma=0.0))
        elif s % 10 == 8:
            strands.append(1e-3 * rng.integers(-2, 3, size=(n, 3)))
        else:
            strands.append(jittered(n, rng))
    strands[9][10, 2] = np.nan
    return _pack(strands)


HARD = {"edges": (edge_strands, TOL), "edges_tol0": (edge_strands, 0.0), "edges_wide": (edge_strands, 5e-3),
        "mixed": (mixed_strands, TOL), "nonfinite": (nonfinite_strands, TOL),
        "shapes": (shape_strands, 0.5), "shapes_tol0": (shape_strands, 0.0), "shapes_wide": (shape_strands, 3.0),
        "ties": (tie_strands, 1.0), "ties_tol0": (tie_strands, 0.0),
        "chain": (lambda: _pack([chain()]), 0.0), "chain_tol": (lambda: _pack([chain()]), 1e-20),
        "pool": (pool_strands, TOL)}
HARD_NAMES = tuple(HARD)


@functools.lru_cache(maxsize=None)
def hard_cases():
    return {name: make() + (tol,) for name, (make, tol) in HARD.items()}


def shape_index(name):
    return SHAPES.index(name)


# ---- a hand-worked strand ----------------------------------------------------------------------------------------------------------
# tol = 0.5.  The interval (0, 4): ab = (4, 0, 0); d2 = 0, 1, 0 for the joints 1, 2, 3: joint 2 is kept (1 > 0.25), depth 1.  The
# interval (0, 2): ab = (2, 1, 0), L2 = 5; joint 1: ap = (1, 0, 0), t = 2 / 5, q = (0.2, -0.4, 0), d2 = 0.2 <= 0.25: dropped.  The
# interval (2, 4) mirrors it: ab = (2, -1, 0); joint 3: ap = (1, -1, 0), t = 3 / 5, q = (-0.2, -0.4, 0), d2 = 0.2: dropped.
WORKED = [[0, 0, 0], [1, 0, 0], [2, 1, 0], [3, 0, 0], [4, 0, 0]]
