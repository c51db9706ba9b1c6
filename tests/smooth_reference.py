"""The strand smoothing restated as a plain loop, strand by strand and joint by joint, from the docstring of scene/strand_smooth.py; it
shares no code with the product.  Float64 values are Python floats (IEEE doubles: +, -, *, / and math.sqrt round once); the result is
rounded once to float32 by numpy.

The contract: all arithmetic is float64 on the float32 inputs, one rounding per operation, in the order written; dot(u, v) =
(u0*v0 + u1*v1) + u2*v2.  Per strand with joints p_0 .. p_{n-1}: status 1 (short) for n < 3, 2 (long) for n > 1024, 3 where a
coordinate is not finite -- the strand is copied -- and otherwise 0:
    l_i = sqrt(dot(e_i, e_i)) for e_i = p_{i+1} - p_i;
    for inner j: s_j = l_{j-1} + l_j; a_j = l_j / s_j and b_j = l_{j-1} / s_j if s_j > 0, else both 0.5;
    a sweep with factor f (Jacobi): m = a_j*x_{j-1}[c] + b_j*x_{j+1}[c]; x'_j[c] = x_j[c] + f*(m - x_j[c]); the end joints stay;
    iters times: a sweep with lam, then, unless mu == 0, a sweep with mu;
    with max_move, for inner j: u = x_j - p_j; du = sqrt(dot(u, u)); if du > max_move: x_j = p_j + (max_move/du)*u, clamped += 1;
    out_j = float32(x_j) for inner joints; the two end joints get their input bits."""
import math

import numpy as np

MAX_JOINTS = 1024


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sweep(x, a, b, f):
    new = [x[0]]
    for j in range(1, len(x) - 1):
        row = []
        for c in range(3):
            m = a[j] * x[j - 1][c] + b[j] * x[j + 1][c]
            row.append(x[j][c] + f * (m - x[j][c]))
        new.append(row)
    new.append(x[-1])
    return new


def smooth(points, offsets, iters, lam, mu, max_move):
    """(out float32 [P, 3], status int32 [K], clamped int32 [K])."""
    lam, mu = float(lam), float(mu)
    K = len(offsets) - 1
    out = np.array(points, dtype=np.float32, copy=True)
    status, clamped = np.zeros(K, np.int32), np.zeros(K, np.int32)
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
        length = []
        for i in range(n - 1):
            e = [p[i + 1][c] - p[i][c] for c in range(3)]
            length.append(math.sqrt(_dot(e, e)))
        a, b = [None] * n, [None] * n
        for j in range(1, n - 1):
            sj = length[j - 1] + length[j]
            if sj > 0.0:
                a[j], b[j] = length[j] / sj, length[j - 1] / sj
            else:
                a[j], b[j] = 0.5, 0.5
        x = [list(row) for row in p]
        for _ in range(int(iters)):
            x = _sweep(x, a, b, lam)
            if mu != 0.0:
                x = _sweep(x, a, b, mu)
        if max_move is not None:
            for j in range(1, n - 1):
                u = [x[j][c] - p[j][c] for c in range(3)]
                du = math.sqrt(_dot(u, u))
                if du > max_move:
                    g = max_move / du
                    x[j] = [p[j][c] + g * u[c] for c in range(3)]
                    clamped[s] += 1
        for j in range(1, n - 1):
            out[first + j] = [np.float32(v) for v in x[j]]
    return out, status, clamped


def turning_angle(points):
    """The mean angle in degrees between the two segments at the inner joints of one strand [n, 3], in float64."""
    p = np.asarray(points, np.float64)
    total, count = 0.0, 0
    for j in range(1, len(p) - 1):
        e0, e1 = p[j] - p[j - 1], p[j + 1] - p[j]
        l0, l1 = math.sqrt(_dot(e0, e0)), math.sqrt(_dot(e1, e1))
        if l0 > 0.0 and l1 > 0.0:
            total += math.degrees(math.acos(max(-1.0, min(1.0, _dot(e0, e1) / (l0 * l1)))))
            count += 1
    return total / max(1, count)


def polyline_length(points):
    p = np.asarray(points, np.float64)
    return float(sum(math.sqrt(_dot(p[i + 1] - p[i], p[i + 1] - p[i])) for i in range(len(p) - 1)))
