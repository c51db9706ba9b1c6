"""The case catalogue of the guide selection (hair-gs_amd/scene/strand_guides.py), shared by tests/test_guides_cpu.py and
tests/test_guides_gpu.py.  Every case is (points float32 [N*M, 3], offsets int64 [N + 1], k, samples, iters); all of them are tiny:
the loop restatement (tests/guides_reference.py) walks N x K x S x iterations scalar steps.  The kernels stage their centroids in
LDS tiles of 64 (S <= 16), 16 (S <= 32) and 8 (S <= 64) centroids; the k of the cases cross each of them, and 255 / 256 / 257."""
import functools

import numpy as np

F32_MAX = float(np.finfo(np.float32).max)


def pack(strands):
    """points, offsets of a list of [M, 3] arrays."""
    pts = np.concatenate([np.asarray(s, np.float64).reshape(-1, 3) for s in strands]).astype(np.float32) if strands else np.zeros((0, 3), np.float32)
    off = np.concatenate([[0], np.cumsum([len(s) for s in strands])]).astype(np.int64)
    return pts, off


def blob(N, M, seed, scale=1.0):
    """N wavy strands of M points, roots spread over a unit cube: nothing is separated."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, M)[None, :, None]
    root, dirn = rng.uniform(-1.0, 1.0, (N, 1, 3)), rng.normal(size=(N, 1, 3))
    wave = 0.1 * np.sin(6.0 * t + rng.uniform(0.0, 6.28, (N, 1, 1))) * rng.normal(size=(N, 1, 3))
    return list(scale * (root + 0.5 * t * dirn + wave))


def clumps(n_clumps, per, M, seed, jitter=1e-3):
    """n_clumps locks of `per` strands each, clump after clump: lock centre lines 10 apart, strands within `jitter` of them."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, M)[:, None]
    out = []
    for c in range(n_clumps):
        line = np.array([10.0 * c, 0.0, 0.0]) + t * rng.normal(size=(1, 3)) + 0.05 * np.sin(5.0 * t)
        out += [line + rng.normal(scale=jitter, size=(M, 3)) for _ in range(per)]
    return out


def with_bad(strands, where):
    """The strands with a value put at (strand, point, coordinate)."""
    out = [np.array(s, np.float64) for s in strands]
    for (i, j, c), v in where.items():
        out[i][j, c] = v
    return out


def _duplicates():
    a, b, c = blob(3, 5, 11)
    return [a, a, b, b, a, c, b, a, c, c, b, a]


def _duplicate_seeds():
    """K = 4 of 8 strands seeds the strands 1, 3, 5, 7: all of them X, so the four clusters tie wherever X is nearest, and the
    clusters 2 and 3 never get a member."""
    x = blob(1, 4, 12)[0]
    rest = blob(4, 4, 13)
    return [rest[0], x, rest[1], x, rest[2], x, rest[3], x]


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    c["one"] = (*pack(blob(1, 2, 1)), 1, 2, 10)
    c["n63_m3_k2"] = (*pack(blob(63, 3, 2)), 2, 16, 10)                             # S = M < samples
    c["n64_m17_k1"] = (*pack(blob(64, 17, 3)), 1, 16, 3)                            # S = samples < M, 16 % 15 != 0
    c["n65_m100_s64_k9"] = (*pack(blob(65, 100, 4)), 9, 64, 4)                      # S = 64, 99 % 63 != 0; across a tile of 8
    c["n65_m17_s64_k17"] = (*pack(blob(65, 17, 5)), 17, 64, 3)                      # S = 17; across a tile of 16
    c["n129_m17_k65"] = (*pack(blob(129, 17, 6)), 65, 16, 3)                        # S = 16; across a tile of 64
    for k in (255, 256, 257):
        c[f"n257_m2_k{k}"] = (*pack(blob(257, 2, 7)), k, 2, 2)                      # (257: every strand its own cluster)
    c["n1000_m3_k2"] = (*pack(blob(1000, 3, 8)), 2, 2, 10)
    c["k_over_n"] = (*pack(blob(65, 3, 9)), 100, 16, 10)
    c["duplicates"] = (*pack(_duplicates()), 3, 16, 10)
    c["duplicate_seeds"] = (*pack(_duplicate_seeds()), 4, 16, 10)
    c["nonfinite_unsampled"] = (*pack(with_bad(blob(20, 17, 14), {(3, 5, 1): np.nan, (7, 8, 0): np.inf, (12, 16, 2): -np.inf})), 3, 2, 10)
    c["all_nonfinite"] = (*pack(with_bad(blob(5, 3, 15), {(i, 1, 0): np.nan for i in range(5)})), 2, 16, 10)
    c["near_max"] = (*pack(blob(10, 3, 16, scale=F32_MAX / 2.0)), 2, 16, 10)
    c["clumps_known"] = (*pack(clumps(4, 16, 17, 17)), 4, 16, 10)
    c["iters1"] = (*pack(blob(63, 3, 18)), 5, 16, 1)
    c["not_converged"] = (*pack(blob(200, 3, 19)), 8, 16, 2)
    return c


NAMES = ("one", "n63_m3_k2", "n64_m17_k1", "n65_m100_s64_k9", "n65_m17_s64_k17", "n129_m17_k65", "n257_m2_k255", "n257_m2_k256",
         "n257_m2_k257", "n1000_m3_k2", "k_over_n", "duplicates", "duplicate_seeds", "nonfinite_unsampled", "all_nonfinite", "near_max",
         "clumps_known", "iters1", "not_converged")
FIELDS = ("labels", "dist2", "guide", "count", "status", "iterations", "converged", "centroids", "first_dist2")

# (k, samples, iters) that check_parameters refuses, and the word its message has
REFUSED = (((0, 16, 10), "k"), ((65537, 16, 10), "k"), ((2.5, 16, 10), "k"), ((True, 16, 10), "k"), ((4, 1, 10), "samples"),
           ((4, 65, 10), "samples"), ((4, 16, 0), "iters"), ((4, 16, 257), "iters"))


def ragged():
    return pack([np.zeros((3, 3)), np.zeros((4, 3))])


def one_point():
    return pack([np.zeros((1, 3)), np.ones((1, 3))])


def as_export(pts, off):
    """A StrandExport with attributes, ids and lengths that tell the strands apart."""
    from scene.strand_export import StrandExport
    N = off.shape[0] - 1
    attrs = np.arange(pts.shape[0] * 2, dtype=np.float32).reshape(-1, 2)
    return StrandExport(pts, attrs, off, np.arange(N, dtype=np.int64) * 3 + 7, np.arange(N, dtype=np.float64) + 0.5)
