"""Inputs of the groom interpolation's tests (tests/test_groom_cpu.py, tests/test_groom_gpu.py): the size grid, the hand-built hard
cases and the analytic groom.  Everything is generated from fixed seeds."""
import numpy as np

NS = (0, 1, 63, 64, 65, 257)
KS = (0, 1, 7, 255, 256, 257, 513)        # the LDS tile edge (256) and K < k
KNN = (1, 4, 8)
MS = (2, 3, 65)
CS = (1, 5)
MAX_D2 = (np.inf, 4.0, 1.0)               # 4 is the d2 of a lattice root to the guides two cells away: admitted; 1 leaves few guides or none
ANGLES = (0.0, 60.0, 180.0)
# (N, K, k, M, C, max_d2, max_angle) of the blend comparisons: every value of every size at least once; the square roots of these max_d2
# are exact, so the distance a caller passes squares to them
BLEND_CASES = ((1, 1, 1, 2, 1, np.inf, 60.0), (63, 7, 4, 3, 5, np.inf, 180.0), (64, 255, 8, 65, 1, 4.0, 60.0), (65, 256, 4, 2, 5, np.inf, 60.0),
               (257, 257, 4, 3, 5, 4.0, 0.0), (65, 513, 8, 3, 1, np.inf, 180.0), (65, 7, 8, 65, 5, np.inf, 60.0), (0, 7, 4, 3, 1, np.inf, 60.0),
               (65, 0, 4, 3, 1, np.inf, 60.0), (64, 1, 8, 2, 5, 0.25, 60.0), (257, 513, 1, 2, 1, 0.25, 60.0))


def grid_roots():
    """257 float64 roots: a third on the integer lattice of the guide roots (d2 == 0 and exact ties), a third on half-integers (exact
    ties between lattice neighbours), a third anywhere; NaN, inf and 1e200 (d2 overflows) among them."""
    rng = np.random.default_rng(7)
    n = 257
    r = np.empty((n, 3), np.float64)
    lat = rng.integers(-3, 4, size=(n, 3)).astype(np.float64)
    r[0::3] = lat[0::3]
    r[1::3] = lat[1::3] + 0.5
    r[2::3] = rng.uniform(-3.5, 3.5, size=(n, 3))[2::3]
    r[3, 0] = np.nan
    r[5, 1] = np.inf
    r[7, 0] = 1e200
    r[11] = -1e200
    return r


def grid_case(K, M=3, C=1):
    """(gp float32 [K, M, 3], ga float32 [K, M, C], roots float64 [257, 3]).  The guides' roots and tips do not depend on M or C: roots on
    the integer lattice [-3, 3]^3 (duplicates from K = 255 on), two families of opposite chords by the parity of g, a zero chord where
    g % 11 == 5, and a NaN root (g = 2), an infinite root coordinate (g = 4) and a NaN tip (g = 9)."""
    rng = np.random.default_rng(100 + K)
    root = rng.integers(-3, 4, size=(K, 3)).astype(np.float32)
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)[:, None]
    vec = (sign * np.array([0.3, 0.2, -1.0]) + 0.3 * rng.normal(size=(K, 3))).astype(np.float32)
    vec[np.arange(K) % 11 == 5] = 0
    tip = root + vec
    fill = np.random.default_rng(1000 * M + 10 * C + K)
    s = (np.arange(M, dtype=np.float32) / np.float32(M - 1))[None, :, None]
    gp = (root[:, None, :] + s * vec[:, None, :] + np.float32(0.05) * fill.normal(size=(K, M, 3)).astype(np.float32)).astype(np.float32)
    gp[:, 0], gp[:, -1] = root, tip
    if K > 2:
        gp[2, 0] = np.nan
    if K > 4:
        gp[4, 0, 1] = np.inf
    if K > 9:
        gp[9, -1, 0] = np.nan
    ga = fill.uniform(-1, 2, size=(K, M, C)).astype(np.float32)
    return np.ascontiguousarray(gp), np.ascontiguousarray(ga), grid_roots()


def straight(roots, chords, M=3, C=1):
    """Guides that run straight from `roots` along `chords` in M points; attribute a of guide g is g + 0.25 a + j / 8."""
    roots, chords = np.asarray(roots, np.float32).reshape(-1, 3), np.asarray(chords, np.float32).reshape(-1, 3)
    s = (np.arange(M, dtype=np.float32) / np.float32(M - 1))[None, :, None]
    gp = (roots[:, None, :] + s * chords[:, None, :]).astype(np.float32)
    K = roots.shape[0]
    ga = (np.arange(K)[:, None, None] + 0.25 * np.arange(C)[None, None, :] + np.arange(M)[None, :, None] / 8.0).astype(np.float32)
    return np.ascontiguousarray(gp), np.ascontiguousarray(ga)


DOWN = (0.0, 0.0, -1.0)


def hard_cases():
    """[(name, gp, ga, roots, k, max_d2, max_angle, expected lists of guides per root or None)]."""
    out = []
    # exact ties, broken by g; a duplicate guide root; a root ON a guide root (the list is cut to it)
    gp, ga = straight([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, 2)], [DOWN] * 6)
    roots = np.array([(0, 0, 0), (1, 0, 0), (0, 0, 1)], np.float64)
    out.append(("ties", gp, ga, roots, 3, np.inf, 60.0, [[0, 1, 2], [0], [5, 0, 1]]))
    out.append(("ties k=8 > K", gp, ga, roots, 8, np.inf, 60.0, [[0, 1, 2, 3, 4, 5], [0], [5, 0, 1, 2, 3, 4]]))
    # a finite max_d2: 0, 1 and fewer than k guides; d2 == max_d2 exactly is admitted
    gp, ga = straight([(1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0)], [DOWN] * 4)
    roots = np.array([(0, 0, 0), (-1, 0, 0), (-2, 0, 0), (-6, 0, 0)], np.float64)
    out.append(("radius 9", gp, ga, roots, 4, 9.0, 60.0, [[0, 1, 2], [0, 1], [0], []]))
    out.append(("radius 0.5", gp, ga, roots, 4, 0.5, 60.0, [[], [], [], []]))
    out.append(("radius 1", gp, ga, roots, 4, 1.0, 60.0, [[0], [], [], []]))
    # NaN, inf and 1e200 in a root; NaN and inf in a guide root
    gp, ga = straight([(0.5, 0, 0), (0.25, 0, 0), (1, 0, 0), (2, 0, 0)], [DOWN] * 4)
    gp[0, 0, 0], gp[1, 0, 2] = np.nan, np.inf
    roots = np.array([(0, 0, 0), (np.nan, 0, 0), (0, np.inf, 0), (1e200, 0, 0), (0, 0, -1e200), (3, 0, 0)], np.float64)
    out.append(("non-finite", gp, ga, roots, 4, np.inf, 180.0, [[2, 3], [], [], [], [], [3, 2]]))
    # a parting: two families of opposite falls, a root between them keeps the nearest's family
    gp, ga = straight([(-1, 0, 0), (-2, 0, 0), (-3, 0, 0), (1.5, 0, 0), (2.5, 0, 0), (3.5, 0, 0)], [(-1, 0, -1)] * 3 + [(1, 0, -1)] * 3, M=5, C=2)
    roots = np.array([(0, 0, 0), (0.5, 0, 0)], np.float64)
    out.append(("parting 60", gp, ga, roots, 4, np.inf, 60.0, [[0, 1], [3, 4]]))
    out.append(("parting 180", gp, ga, roots, 4, np.inf, 180.0, [[0, 3, 1, 4], [3, 0, 4, 1]]))
    out.append(("parting 0", gp, ga, roots, 4, np.inf, 0.0, None))
    # the nearest guide has a zero chord: the others are dropped; a zero chord at rank >= 1 is dropped
    gp, ga = straight([(0.5, 0, 0), (1, 0, 0), (2, 0, 0), (-4, 0, 0)], [(0, 0, 0), DOWN, DOWN, (0, 0, 0)])
    roots = np.array([(0, 0, 0), (1.75, 0, 0), (-1, 0, 0)], np.float64)
    out.append(("zero chords", gp, ga, roots, 4, np.inf, 60.0, [[0], [2, 1], [0]]))
    out.append(("zero chords 180", gp, ga, roots, 4, np.inf, 180.0, [[0], [2, 1], [0]]))
    return out


def analytic_groom(n=2000, M=17):
    """(roots float64 [n, 3], strands float64 [n, M, 3]): Fibonacci roots on the upper part of the unit sphere (z = 1 - 0.8 (i + 0.5) / n)
    and p(s) = root + L (0.6 s n + 0.8 s^2 (0, 0, -1) + s 0.2 sin(3 x) (0, sin 6 s, 0)), L = 0.5 + 0.3 y, s = linspace(0, 1, M)."""
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - 0.8 * (i + 0.5) / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    rad = np.sqrt(1.0 - z * z)
    roots = np.stack([rad * np.cos(phi), rad * np.sin(phi), z], axis=1)
    s = np.linspace(0.0, 1.0, M)[None, :, None]
    L = (0.5 + 0.3 * roots[:, 1])[:, None, None]
    wave = np.zeros((n, M, 3))
    wave[:, :, 1] = (s[..., 0] * 0.2) * np.sin(3.0 * roots[:, 0])[:, None] * np.sin(6.0 * s[..., 0])
    p = roots[:, None, :] + L * (0.6 * s * roots[:, None, :] + 0.8 * s * s * np.array([0.0, 0.0, -1.0]) + wave)
    return roots, p
