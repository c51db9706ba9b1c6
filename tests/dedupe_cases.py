"""Inputs of the strand deduplication's tests (tests/test_dedupe_cpu.py, tests/test_dedupe_gpu.py): small grooms that sit on the places
at which hgs_dedupe_count / hgs_dedupe_fill / hgs_dedupe_resolve (csrc/hgs_dedupe.hip) and the numpy path of scene/strand_dedupe.py
can go wrong.  Inputs only: (points float32 [N*M, 3], offsets int64 [N + 1], tol).  The kernels give a lane a strand, a wavefront 64, a
workgroup 256, and stage the earlier strands' roots in LDS tiles of 256: NS has a strand count below, at and above each of those."""
import functools

import numpy as np

NS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
MS = (2, 3, 100)
TOL = 1e-3
REFUSED = (-1.0, float("nan"), float("inf"), float("-inf"), "wide", None)


def pack(strands):
    """(points, offsets) of a list of [M, 3] arrays."""
    sizes = [len(s) for s in strands]
    pts = np.concatenate([np.asarray(s, np.float64).reshape(-1, 3) for s in strands]).astype(np.float32) if strands else np.zeros((0, 3), np.float32)
    return pts, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def first_strands(pts, off, N):
    return pts[:off[N]], off[:N + 1]


def blob(N, M, seed, tol=TOL):
    """N random walks of M joints (2 mm steps) in a 20 cm box.  Two strands in five are planted: a copy of an EARLIER strand (so that any
    prefix of the blob is a blob) with every coordinate jittered by at most 0.4 tol -- within 0.7 tol at every joint, a pair -- and every
    other one of them with ONE joint, anywhere from the root to the tip, moved by 1.5 tol more: no pair.  Copies of copies make chains."""
    rng = np.random.default_rng(seed)
    strands = []
    for i in range(N):
        kind = rng.integers(0, 5) if i else 4
        if kind >= 2:
            steps = 2e-3 * rng.normal(size=(M, 3))
            steps[0] = rng.uniform(-0.1, 0.1, 3)
            strands.append(np.cumsum(steps, axis=0).astype(np.float32))
            continue
        s = strands[int(rng.integers(0, i))].astype(np.float64) + rng.uniform(-0.4 * tol, 0.4 * tol, (M, 3))
        if kind == 1:
            s[int(rng.integers(0, M)), int(rng.integers(0, 3))] += 1.5 * tol * (1.0 if rng.integers(0, 2) else -1.0)
        strands.append(s.astype(np.float32))
    return pack(strands)


def one_joint(where, M=5):
    """Groups of strands that agree everywhere but at one joint (0: the root, -1: the tip): per group the strand, an exact copy, one
    moved by 2 tol there, one by 0.5 tol there, and a copy of the moved one."""
    rng = np.random.default_rng(3 + where)
    strands = []
    for g in range(6):
        base = rng.uniform(-0.05, 0.05, (M, 3)).astype(np.float32).astype(np.float64)
        far, near = base.copy(), base.copy()
        far[where, g % 3] += 2.0 * TOL
        near[where, (g + 1) % 3] -= 0.5 * TOL
        strands += [base, base, far, near, far]
    return pack(strands)


def boundary():
    """tol = 3 on integers: an offset of (3, 0, 0) at one joint is a pair (d2 == tol2), (3, 0, 1) is not, nor is (2, 2, 2) (12 > 9); (2,
    2, 1) is (9)."""
    base = np.array([[0, 0, 0], [10, 20, 30], [-5, 7, 100]], np.float64)
    strands = [base]
    for joint, d in ((1, (3, 0, 0)), (1, (3, 0, 1)), (2, (0, -3, 0)), (0, (2, 2, 2)), (0, (2, 2, 1)), (2, (0, 0, 4))):
        s = base + 50.0 * len(strands)                                              # every probe has a twin of the base beside it, far from the others
        strands.append(s)
        t = s.copy()
        t[joint] += d
        strands.append(t)
    return pack(strands)


BOUNDARY_PAIRS = [True, False, True, False, True, False]                            # of the probes above with their twins


def exact():
    """tol = 0: exact copies, a copy that differs in one bit, and -0.0 against 0.0 (one value)."""
    rng = np.random.default_rng(11)
    base = rng.uniform(-1, 1, (4, 3)).astype(np.float32)
    base[2, 1] = 0.0
    bit = base.copy()
    bit[3, 0] = np.nextafter(bit[3, 0], np.float32(2.0))
    zero = base.copy()
    zero[2, 1] = -0.0
    other = rng.uniform(-1, 1, (4, 3)).astype(np.float32)
    return pack([base, base, bit, zero, other, bit, other])


def identical(n=130, M=3):
    s = np.array([[0.01, 0.02, 0.03], [0.02, 0.02, 0.05], [0.03, 0.01, 0.07]])[:M]
    return pack([s] * n)


def chain(n=40, tol=1.0):
    """Strand c lies 0.9 tol c along x: c pairs with c - 1 and c + 1 only (1.8 tol to the next but one)."""
    base = np.array([[0, 0, 0], [0, 1, 0], [0, 2, 1]], np.float64)
    return pack([base + [0.9 * tol * c, 0.0, 0.0] for c in range(n)])


def nonfinite(M=5):
    """Strands with a NaN, +inf or -inf at the root, in the middle and at the tip, each followed by its exact copy, among finite strands
    with copies of their own."""
    rng = np.random.default_rng(17)
    good = rng.uniform(-0.05, 0.05, (M, 3)).astype(np.float32)
    strands = [good]
    for joint in (0, M // 2, M - 1):
        for v in (np.nan, np.inf, -np.inf):
            bad = good.astype(np.float64)
            bad[joint, len(strands) % 3] = v
            strands += [bad, bad, good]
    both = good.astype(np.float64)
    both[1, 0], both[1, 1] = np.inf, -np.inf
    return pack(strands + [both, both])


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (points, offsets, tol)}."""
    out = {f"blob_m{M}": blob(NS[-1], M, seed=M) + (TOL,) for M in MS}
    out["tip"] = one_joint(-1) + (TOL,)
    out["root"] = one_joint(0) + (TOL,)
    out["boundary"] = boundary() + (3.0,)
    out["exact"] = exact() + (0.0,)
    out["identical"] = identical() + (TOL,)
    out["identical_tol0"] = identical(70, 2) + (0.0,)
    out["chain"] = chain() + (1.0,)
    out["nonfinite"] = nonfinite() + (TOL,)
    out["one"] = pack([np.zeros((2, 3))]) + (TOL,)
    return out


NAMES = tuple(f"blob_m{M}" for M in MS) + ("tip", "root", "boundary", "exact", "identical", "identical_tol0", "chain", "nonfinite", "one")
