"""The strand simplification restated as the recursion itself, strand by strand with an explicit stack of intervals, from the docstring
of scene/strand_simplify.py; it shares no code with the product and does not work round by round.  Float64 values are Python floats
(IEEE doubles: +, -, * and / round once).

The contract: all arithmetic is float64 on the float32 inputs, one rounding per operation, in the order written; dot(u, v) =
(u0*v0 + u1*v1) + u2*v2.  Per strand with joints p_0 .. p_{n-1}: status 1 (short) for n < 3, 2 (long) for n > 1024, 3 where a
coordinate is not finite -- every joint is kept, rounds 0 -- and otherwise 0:
    d2(p; a, b): ab = b - a; ap = p - a; L2 = dot(ab, ab); t = dot(ap, ab) / L2 if L2 > 0, else 0; t < 0 becomes 0, t > 1 becomes 1;
        q_c = ap_c - t*ab_c; d2 = dot(q, q);
    joints 0 and n - 1 are kept; the interval (0, n - 1) has depth 1;
    in an interval (i, k) with k > i + 1, j* is the joint between them with the largest d2(p_j; p_i, p_k), the smallest j among
        equals; if d2(j*) > tol*tol (strict, the product formed once), j* is kept, and (i, j*) and (j*, k) have the next depth;
    rounds = the largest depth at which a joint was kept."""
import math

import numpy as np

MAX_JOINTS = 1024


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def deviation2(p, a, b):
    """(d2, t) of the contract for three joints given as sequences of three Python floats."""
    ab = [b[c] - a[c] for c in range(3)]
    ap = [p[c] - a[c] for c in range(3)]
    L2 = _dot(ab, ab)
    t = _dot(ap, ab) / L2 if L2 > 0.0 else 0.0
    if t < 0.0:
        t = 0.0
    if t > 1.0:
        t = 1.0
    q = [ap[c] - t * ab[c] for c in range(3)]
    return _dot(q, q), t


def simplify_strand(p, tol):
    """(keep list of 0 / 1, rounds) of one OK strand p: a list of n >= 3 joints, three finite Python floats each."""
    n = len(p)
    tol2 = float(tol) * float(tol)
    keep = [0] * n
    keep[0] = keep[n - 1] = 1
    rounds = 0
    stack = [(0, n - 1, 1)]
    while stack:
        i, k, depth = stack.pop()
        if k <= i + 1:
            continue
        best, at = -1.0, -1
        for j in range(i + 1, k):
            d2, _ = deviation2(p[j], p[i], p[k])
            if d2 > best:                                                          # (strict: the smallest j among equals stays)
                best, at = d2, j
        if best > tol2:
            keep[at] = 1
            rounds = max(rounds, depth)
            stack.append((i, at, depth + 1))
            stack.append((at, k, depth + 1))
    return keep, rounds


def simplify(points, offsets, tol):
    """(keep uint8 [P], status int32 [K], rounds int32 [K])."""
    K = len(offsets) - 1
    keep = np.ones(len(points), np.uint8)
    status, rounds = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for s in range(K):
        first, n = int(offsets[s]), int(offsets[s + 1] - offsets[s])
        if n < 3:
            status[s] = 1
            continue
        if n > MAX_JOINTS:
            status[s] = 2
            continue
        p = [[float(points[first + j, c]) for c in range(3)] for j in range(n)]
        if not all(math.isfinite(v) for row in p for v in row):
            status[s] = 3
            continue
        flags, rounds[s] = simplify_strand(p, tol)
        keep[first:first + n] = flags
    return keep, status, rounds


def final_deviations(points, offsets, keep):
    """For every dropped joint of every strand, (row, d2, t, left row, right row) against the segment between the kept joints around
    it, by the contract's statement."""
    out = []
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        kept = [r for r in range(a, b) if keep[r]]
        for left, right in zip(kept[:-1], kept[1:]):
            for r in range(left + 1, right):
                d2, t = deviation2([float(v) for v in points[r]], [float(v) for v in points[left]], [float(v) for v in points[right]])
                out.append((r, d2, t, left, right))
    return out
