"""Strands and parameters of the strand smoothing's tests (tests/test_smooth_cpu.py, tests/test_smooth_gpu.py): the smallest at which
hgs_strand_smooth (csrc/hgs_strand_smooth.hip) and the numpy path of scene/strand_smooth.py can go wrong.  Inputs only.  A case is
(points float32 [P, 3], offsets int64 [K + 1], (iters, lam, mu, max_move))."""
import functools

import numpy as np

# joints per strand: none, below and at the least that is smoothed, around one, two and sixteen chunks of 64, and past MAX_JOINTS
EDGE_N = (0, 1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025)
KS = (0, 1, 3, 4, 5, 257)                         # strand counts: around a workgroup of four wavefronts, and many workgroups

DEFAULTS = (10, 0.5, -0.53, None)
ZIGZAG_MOVE = 5e-4                                # against the zigzag's amplitude of 1.27e-3: most of its joints are held
PARAMS = {"default": DEFAULTS, "i1": (1, 0.5, -0.53, None), "i256": (256, 0.5, -0.53, None), "mu0": (10, 0.5, 0.0, None),
          "narrow": (7, 0.33, -0.34, None), "full": (3, 1.0, 0.0, None), "move": (10, 0.5, -0.53, ZIGZAG_MOVE)}
# refused by the parameter check, with the word its message carries (lam = 1 with mu = -1: mu is not below -lam)
REFUSED = (((0, 0.5, -0.53, None), "iters"), ((257, 0.5, -0.53, None), "iters"), ((2.5, 0.5, -0.53, None), "iters"),
           ((10, 0.0, -0.53, None), "lam"), ((10, -0.5, 0.0, None), "lam"), ((10, 1.5, 0.0, None), "lam"), ((10, float("nan"), 0.0, None), "lam"),
           ((10, 1.0, -1.0, None), "mu"), ((10, 0.5, -0.5, None), "mu"), ((10, 0.5, 0.3, None), "mu"), ((10, 0.5, -1.01, None), "mu"),
           ((10, 0.5, -0.4, None), "mu"), ((10, 0.5, float("nan"), None), "mu"), ((10, 0.9, -1.0, None), "grow"), ((10, 0.1, -1.0, None), "grow"),
           ((10, 0.5, -0.53, 0.0), "max_move"), ((10, 0.5, -0.53, -1.0), "max_move"), ((10, 0.5, -0.53, float("inf")), "max_move"),
           ((10, 0.5, -0.53, float("nan")), "max_move"))


def _pack(strands):
    """(points float32 [P, 3], offsets int64 [K + 1]) of a list of [n, 3] arrays (n >= 0)."""
    n = [len(s) for s in strands]
    pts = np.concatenate([np.asarray(s, np.float64).reshape(-1, 3) for s in strands] + [np.zeros((0, 3))]).astype(np.float32)
    return pts, np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def jittered(n, rng, step=2e-3, sigma=3e-4):
    """n joints along a gentle helix from a random place, `step` apart, with a trained strand's jitter on every joint."""
    t = step * np.arange(n)
    r, w, ph = rng.uniform(0.01, 0.03), rng.uniform(20.0, 60.0), rng.uniform(0.0, 6.28)
    curve = np.stack([r * np.cos(w * t + ph), r * np.sin(w * t + ph), -0.8 * t], axis=1)
    return rng.uniform(-0.1, 0.1, size=3) + curve + rng.normal(scale=sigma, size=(n, 3))


# ---- the special strands -----------------------------------------------------------------------------------------------------------
ARC_N, ARC_RADIUS, ARC_SIGMA = 100, 0.1, 3e-4


def clean_arc():
    a = np.linspace(0.0, 0.5 * np.pi, ARC_N)
    return np.stack([ARC_RADIUS * np.cos(a), ARC_RADIUS * np.sin(a), np.zeros(ARC_N)], axis=1)


def noisy_arc():
    """A quarter arc of radius 0.1 with noise of sigma 3e-4 on its 98 inner joints; the ends are the clean arc's."""
    arc = clean_arc()
    arc[1:-1] += np.random.default_rng(5).normal(scale=ARC_SIGMA, size=(ARC_N - 2, 3))
    return arc


def zigzag(n=40, d=1e-3, h=1.27e-3):
    """Joints d apart along x, alternately h above and below the axis: every inner joint turns by 2 atan(2h / d), about 137 degrees."""
    j = np.arange(n)
    return np.stack([d * j, h * (1 - 2 * (j & 1)), np.full(n, 0.05)], axis=1)


def straight_line(n=50):
    t = np.linspace(0.0, 1.0, n)[:, None]
    return np.array([0.1, 0.2, 0.3]) + t * np.array([0.4, -0.3, 0.6])


SPECIAL = ("collapsed", "collapsed_beside_long", "nan_middle", "inf_middle", "nan_end", "inf_end", "far", "zigzag", "line", "arc", "five")


@functools.lru_cache(maxsize=None)
def special_strands():
    """One strand per name of SPECIAL, in that order."""
    rng = np.random.default_rng(11)
    p, q, r = np.array([0.01, 0.02, 0.03]), np.array([0.012, 0.021, 0.03]), np.array([0.015, 0.02, 0.031])
    collapsed = [p, p, p, q, r, r, r + 0.001]                                      # joint 1: s_j == 0, both neighbours equal
    beside = [p, q, q, q + np.array([0.05, 0.0, 0.0]), q + np.array([0.051, 0.001, 0.0])]     # a zero segment beside a long one
    bad = []
    for value, at in ((np.nan, 3), (np.inf, 2), (np.nan, 0), (-np.inf, 5)):          # in the middle of a strand, and in an end joint
        s = jittered(6, rng)
        s[at, 1] = value
        bad.append(s)
    far = 1e4 + np.stack([0.01 * np.arange(30), np.zeros(30), np.zeros(30)], axis=1) + rng.normal(scale=1e-3, size=(30, 3))
    five = ARC_RADIUS * np.stack([np.cos(np.linspace(0, 1.2, 5)), np.sin(np.linspace(0, 1.2, 5)), np.zeros(5)], axis=1)
    return _pack([collapsed, beside] + bad + [far, zigzag(), straight_line(), noisy_arc(), five])


def special_index(name):
    return SPECIAL.index(name)


# ---- launches ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_strands():
    """One strand of every size of EDGE_N, in that order."""
    rng = np.random.default_rng(3)
    return _pack([jittered(n, rng) for n in EDGE_N])


@functools.lru_cache(maxsize=None)
def mixed_strands():
    """3-joint and 1024-joint strands side by side: the longest sizes the LDS slice for all."""
    rng = np.random.default_rng(4)
    return _pack([jittered(n, rng) for n in (3, 1024, 3, 3, 1024, 3, 1024)])


@functools.lru_cache(maxsize=None)
def pool_strands():
    """257 ragged strands of 0 to 140 joints, the first of them 0, 1, 2, 3 and 130 joints long, one with a NaN."""
    rng = np.random.default_rng(7)
    sizes = [0, 1, 2, 3, 130] + [int(v) for v in rng.integers(0, 141, size=max(KS) - 5)]
    sizes[9] = 20
    strands = [jittered(n, rng) for n in sizes]
    strands[9][10, 2] = np.nan
    return _pack(strands)


def first_strands(pts, off, K):
    """The first K strands of a launch: strands are independent, so their results are the first K strands' of the whole."""
    return pts[:off[K]], off[:K + 1]


HARD_NAMES = ("edges_default", "edges_i1", "edges_mu0", "edges_move", "edges_full", "special_default", "special_i1", "special_i256",
              "special_mu0", "special_narrow", "special_move", "mixed_default", "mixed_move")


@functools.lru_cache(maxsize=None)
def hard_cases():
    launches = {"edges": edge_strands, "special": special_strands, "mixed": mixed_strands}
    return {name: launches[name.split("_")[0]]() + (PARAMS[name.split("_")[1]],) for name in HARD_NAMES}
