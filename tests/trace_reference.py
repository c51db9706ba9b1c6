"""utils/trace.py's contract restated with Python floats (IEEE doubles: one rounding per operation) and plain loops, independent of
that module: the splat over ALL (node, point) pairs with no box, the trace root by root.  round() of a Python float is round-half-even."""
import math

import numpy as np

STEPS, BOUNDS, TURN, GAP = 0, 1, 2, 3
ONE = 4294967296.0


def dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def splat(points, dirs, origin, h, shape, r):
    """(acc int64 [nz, ny, nx, 7], skipped)."""
    nx, ny, nz = shape
    o = [float(c) for c in origin]
    h = float(h)
    r2 = float(r) * float(r)
    acc = np.zeros((nz, ny, nx, 7), np.int64)
    skipped = 0
    for pt, dr in zip(np.asarray(points, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)):
        x = [float(c) for c in pt]
        e = [float(c) for c in dr]
        dd = dot(e, e)
        if not all(math.isfinite(c) for c in x) or not (math.isfinite(dd) and dd > 0.0):
            skipped += 1
            continue
        ln = math.sqrt(dd)
        d = [e[0] / ln, e[1] / ln, e[2] / ln]
        m = [d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]]
        for iz in range(nz):
            for iy in range(ny):
                for ix in range(nx):
                    dx = [(o[0] + ix * h) - x[0], (o[1] + iy * h) - x[1], (o[2] + iz * h) - x[2]]
                    d2 = dot(dx, dx)
                    if not d2 < r2:
                        continue
                    k = 1.0 - d2 / r2
                    acc[iz, iy, ix, 0] += round(k * ONE)
                    for j in range(6):
                        acc[iz, iy, ix, j + 1] += round((k * m[j]) * ONE)
    return acc, skipped


def trace(roots, p0, origin, h, shape, dirs, conf, step, max_steps, cos_max, min_conf, max_gap):
    """(joints f64 [S, max_steps + 1, 3] (zero from count on), count i32 [S], reason i32 [S])."""
    nx, ny, nz = shape
    o = [float(c) for c in origin]
    k = 1.0 / float(h)
    step, cos_max, min_conf = float(step), float(cos_max), float(min_conf)
    n_axis = (nx, ny, nz)
    roots = np.asarray(roots, np.float64).reshape(-1, 3)
    S = roots.shape[0]
    joints = np.zeros((S, max_steps + 1, 3), np.float64)
    count, reason = np.zeros(S, np.int32), np.zeros(S, np.int32)
    for s in range(S):
        x = [float(c) for c in roots[s]]
        p = [float(c) for c in p0[s]]
        rows = [list(x)]
        gap, entered, n, last, why = 0, False, 1, 0, STEPS
        for _ in range(max_steps):
            t = [(x[a] - o[a]) * k for a in range(3)]
            if not all(math.isfinite(t[a]) and 0.0 <= t[a] < n_axis[a] - 1 for a in range(3)):
                why = BOUNDS
                break
            i = [int(math.floor(c)) for c in t]
            f = [t[a] - math.floor(t[a]) for a in range(3)]
            g = [[1.0 - f[a], f[a]] for a in range(3)]
            w, v = 0.0, [0.0, 0.0, 0.0]
            for cz in (0, 1):
                for cy in (0, 1):
                    for cx in (0, 1):
                        tw = (g[0][cx] * g[1][cy]) * g[2][cz]
                        a = tw * float(conf[i[2] + cz, i[1] + cy, i[0] + cx])
                        w = w + a
                        e = [float(c) for c in dirs[i[2] + cz, i[1] + cy, i[0] + cx]]
                        if dot(e, p) < 0.0:
                            a = -a
                        v = [v[j] + a * e[j] for j in range(3)]
            nn = dot(v, v)
            if w >= min_conf and math.isfinite(nn) and nn > 0.0:
                ln = math.sqrt(nn)
                d = [v[0] / ln, v[1] / ln, v[2] / ln]
                if entered and dot(d, p) < cos_max:
                    why = TURN
                    break
                entered, gap = True, 0
            else:
                gap = gap + 1
                if gap > max_gap:
                    why = GAP
                    break
                d = list(p)
            x = [x[j] + step * d[j] for j in range(3)]
            p = d
            rows.append(list(x))
            n = n + 1
            if gap == 0:
                last = n - 1
        count[s], reason[s] = last + 1, why
        joints[s, :last + 1] = rows[:last + 1]
    return joints, count, reason


def relative_gap(acc):
    """(l2 - l1)/l2 of the matrices of sums acc int64 [n, 7] (0 where l2 is not > 0): what decides the top eigenvector."""
    a = np.asarray(acc).reshape(-1, 7)[:, 1:].astype(np.float64) / ONE
    lam = np.linalg.eigvalsh(a[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3))
    with np.errstate(all="ignore"):
        return np.where(lam[:, 2] > 0, (lam[:, 2] - lam[:, 1]) / lam[:, 2], 0.0), lam[:, 2]


def compare_solves(acc, got, host, gap_floor=1e-6):
    """got, host: (dir, conf) of two solvers on the sums acc [n, 7].  Zero rows are the same rows (W == 0); the others are unit vectors
    to 1e-12; where the relative eigen-gap (l2 - l1)/l2 is at least gap_floor, 1 - |dot| <= 1e-12 and the confidences differ by at most
    1e-12 l2 (tests/test_lift_gpu.py's bar for hgs_lift_solve: a few ulp of l2 over that gap turn the vector by about 1e-9 rad, and
    an eigenvalue is good to a few ulp of l2).  Returns (rows below the gap, non-empty rows)."""
    a = np.asarray(acc).reshape(-1, 7)
    (dg, cg), (dh, ch) = (got[0].reshape(-1, 3), got[1].reshape(-1)), (host[0].reshape(-1, 3), host[1].reshape(-1))
    empty = a[:, 0] == 0
    assert not dg[empty].any() and not dh[empty].any() and not cg[empty].any() and not ch[empty].any()
    live = ~empty
    assert np.isfinite(dg).all() and np.isfinite(cg).all()
    for d in (dg, dh):
        assert np.allclose(np.linalg.norm(d[live], axis=1), 1.0, rtol=0, atol=1e-12)
        top = np.abs(d[live]).argmax(axis=1)
        assert (d[live][np.arange(top.size), top] > 0).all()                  # the sign rule
    gap, l2 = relative_gap(a)
    tight = live & (gap >= gap_floor)
    if tight.any():
        worst_d = float((1.0 - np.abs((dg[tight] * dh[tight]).sum(axis=1))).max())
        worst_c = float((np.abs(cg[tight] - ch[tight]) / l2[tight]).max())
        print(f"{int(tight.sum())} of {int(live.sum())} rows above the gap: max 1 - |dot| = {worst_d:.3e}, max |conf difference| / l2 = {worst_c:.3e}")
        assert worst_d <= 1e-12 and worst_c <= 1e-12
    return int((live & ~tight).sum()), int(live.sum())
