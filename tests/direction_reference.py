"""The 3-D direction term restated as a plain per-segment loop (utils/direction_term.py states the contract): once in float32, one
numpy scalar operation per operation of the text -- what the numpy path and the kernel must equal bit for bit --, and once in float64
on the same float32 inputs -- what the float32 statement is accurate against.  Nothing here is vectorised, on purpose.

The accuracy bar.  With u = 2^-24 the unit roundoff, kappa = w / |v| the cancellation of the corner sum, everything to first order:
  the corner sum, given the fractions f.  g0 = 1 - f carries 1 rounding, so tw = (gx*gy)*gz carries at most 3 + 2 = 5 u, q = tw*conf
    6 u, q*c_j 7 u; the seven additions of the running sum round by at most u times the sum of the |q| each.  With unit lines
    |dv| <= (7 + 7) u w, i.e. the line's direction is off by at most 14 u kappa.
  the rest.  u_seg = b - a rounds each component once: an angle of at most u, 2 u in the term.  |fd| is off from 1 by the roundings
    of nn (3 u), the square root (u + u / 2) and the division (u): a scale error of at most 3.5 u in fd, 7 u in cu*k;
    cu = dot(u_seg, fd) carries 3 u |u_seg| absolutely, twice in cu*k: 6 u; uu 3 u; the division and the product 2 u;
    the last subtraction u.  7 + 6 + 3 + 2 + 1 + 2 = 21 u, times no kappa -- but kappa >= 1.
  the position.  m = (a + b) * 0.5 rounds once (u |m|), m - origin once (u |m - origin|), the product with 1/h not at all where 1/h is
    a power of two (the volumes of tests/direction_cases.py that this bar is used on).  On swirl33 (1/h = 16) an active midpoint has
    r < 0.82, so |m| / h < 13.2 and t < 29.2: dt < 42.4 u an axis.  The aligned corner values q*c change by at most 2 h = 0.125 of
    themselves (the line turns by at most |d/dx (-y, x, -0.5)/norm| <= 2 a unit length) plus 2 h / 0.75 = 0.167 (the ramp of conf) a cell
    and axis; an active segment has w >= 0.5, so relative to w that is at most 0.125 + 0.167 / 0.5 = 0.46 a cell and axis, and over the
    three axes the line's direction is off by at most 3 * 0.46 * 42.4 u kappa = 58.5 u kappa.  On hand7 (1/h = 8, origin 0) dt <= 6 u
    an axis and a corner value changes by at most 2 of itself: 3 * 2 * 6 = 36 u kappa, less.
  A direction error d_theta changes sin^2 by at most d_theta.  In all (14 + 21 + 58.5) u kappa = 93.5 u kappa = 46.75 kappa 2^-23:
  C = 47.  gs = (-2 k)(fd - k u_seg) has the size 2 / |u_seg| times the same relative roundings: the same C, times 2 / |u_seg|."""
import functools

import numpy as np

C = 47.0


def _loop(points, pairs, volume, min_conf, T):
    """The contract's per-segment loop with every value of the type T (np.float32 or np.float64)."""
    nx, ny, nz = volume.shape
    vol = volume.vol.reshape(-1, 4)
    S = pairs.shape[0]
    o, kk, gate = [T(x) for x in volume.origin32], T(volume.inv_h32), T(np.float32(min_conf))
    top = [T(nx - 1), T(ny - 1), T(nz - 1)]
    term, w_out, gs = np.zeros(S, T), np.zeros(S, T), np.zeros((S, 3), T)
    active, in_range, signs, vnorm = np.zeros(S, bool), np.zeros(S, bool), np.zeros(S, np.int64), np.zeros(S, T)
    half, one, zero = T(0.5), T(1), T(0)

    def dot(p, q):
        return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]
    with np.errstate(all="ignore"):
        for s in range(S):
            a = [T(x) for x in points[pairs[s, 0]]]
            b = [T(x) for x in points[pairs[s, 1]]]
            u = [b[j] - a[j] for j in range(3)]
            m = [(a[j] + b[j]) * half for j in range(3)]
            uu = dot(u, u)
            t = [(m[j] - o[j]) * kk for j in range(3)]
            if not all(np.isfinite(t[j]) and zero <= t[j] < top[j] for j in range(3)):
                continue
            in_range[s] = True
            fl = [np.floor(t[j]) for j in range(3)]
            i = [int(fl[j]) for j in range(3)]
            f = [t[j] - fl[j] for j in range(3)]
            g = [[one - f[j], f[j]] for j in range(3)]
            w, v, bits = zero, [zero, zero, zero], 0
            for z in (0, 1):
                for y in (0, 1):
                    for x in (0, 1):
                        tw = (g[0][x] * g[1][y]) * g[2][z]
                        c = [T(e) for e in vol[((i[2] + z) * ny + (i[1] + y)) * nx + (i[0] + x)]]
                        q = tw * c[3]
                        w = w + q
                        if dot(c, u) < zero:
                            q = -q
                            bits |= 1 << (4 * z + 2 * y + x)
                        v = [v[j] + q * c[j] for j in range(3)]
            nn = dot(v, v)
            w_out[s], signs[s] = w, bits
            if not (w >= gate and np.isfinite(nn) and nn > zero and np.isfinite(uu) and uu > zero):
                continue
            active[s] = True
            ln = np.sqrt(nn)
            vnorm[s] = ln
            fd = [v[j] / ln for j in range(3)]
            cu = dot(u, fd)
            k = cu / uu
            term[s] = one - cu * k
            m2 = T(-2.0) * k
            gs[s] = [m2 * (fd[j] - k * u[j]) for j in range(3)]
    return dict(term=term, w=w_out, gs=gs, active=active, in_range=in_range, signs=signs, vnorm=vnorm)


def _gather(gs, pairs, E, upstream, T):
    """The contract's gradient statement, endpoint by endpoint, over entries found by a plain scan in (s, side) order."""
    S = pairs.shape[0]
    d = np.zeros((E, 3), T)
    runs = [[] for _ in range(E)]
    for s in range(S):
        for side in (0, 1):
            runs[int(pairs[s, side])].append((s, side))
    with np.errstate(all="ignore"):
        scale = T(np.float32(upstream)) / T(S) if S > 0 else T(0)
        for e in range(E):
            acc = [T(0), T(0), T(0)]
            for s, side in runs[e]:
                acc = [acc[j] + (gs[s, j] if side else -gs[s, j]) for j in range(3)]
            d[e] = [acc[j] * scale for j in range(3)]
    return d


def reference(points, pairs, volume, min_conf, upstream=1.0, T=np.float32):
    """The loop's dict plus "value" (T) and "d_points" ([E, 3])."""
    points, pairs = np.asarray(points, np.float32), np.asarray(pairs, np.int64)
    r = _loop(points, pairs, volume, min_conf, T)
    S = pairs.shape[0]
    total = float(np.sum(r["term"].astype(np.float64)))                        # (numpy's own order: the value is compared to an ulp)
    r["value"] = T(total / S) if S else T(0)
    r["d_points"] = _gather(r["gs"], pairs, points.shape[0], upstream, T)
    return r


@functools.lru_cache(maxsize=None)
def of_case(name, wide=False):
    """The float32 (wide: float64) loop on a case of tests/direction_cases.py, computed once."""
    from tests import direction_cases as DC
    vol, pts, pairs, min_conf = DC.case(name)
    return reference(pts, pairs, vol, min_conf, T=np.float64 if wide else np.float32)


def accuracy(name):
    """(worst ratio of the term, worst ratio of gs, rows compared, rows left out, rows whose gate differs) of a case: float32 loop
    against float64 loop over the active segments whose gate and eight signs agree, in units of kappa 2^-23 (times 2 / |u| for gs)."""
    from tests import direction_cases as DC
    _, pts, pairs, _ = DC.case(name)
    lo, hi = of_case(name), of_case(name, wide=True)
    gate_differs = lo["active"] != hi["active"]
    same = ~gate_differs & (lo["signs"] == hi["signs"])
    left_out = np.nonzero(~same & (lo["active"] | hi["active"]))[0]
    rows = np.nonzero(same & hi["active"])[0]
    if rows.size == 0:
        return 0.0, 0.0, 0, left_out, np.nonzero(gate_differs)[0]
    kappa = hi["w"][rows] / hi["vnorm"][rows]
    ulen = np.linalg.norm(pts[pairs[rows, 1]].astype(np.float64) - pts[pairs[rows, 0]].astype(np.float64), axis=1)
    unit = kappa * 2.0 ** -23
    rt = np.abs(lo["term"][rows].astype(np.float64) - hi["term"][rows]) / unit
    rg = np.abs(lo["gs"][rows].astype(np.float64) - hi["gs"][rows]).max(axis=1) / (unit * 2.0 / ulen)
    return float(rt.max()), float(rg.max()), int(rows.size), left_out, np.nonzero(gate_differs)[0]
