"""An independent float64 restatement of utils/head_sdf.py's contract (tests/test_head_sdf_cpu.py, tests/test_head_sdf_gpu.py): the
field by a loop over the faces, each over all nodes; the term by a loop over the points, trilinear value and gradient in float64 on the
float32 field; a central-difference check of that gradient inside a cell; and the comparator, tests/magnet_reference.py's convention:
max|x - x64| <= K max(e_ref, 4 ulp scale) with e_ref the float32 statement's own error and K = 8."""
import numpy as np

from tests import param_reference as R

K = 8.0


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _closest_vector(p, v0, v1, v2):
    """q [N, 3]: from the closest point of the triangle to every p [N, 3], by the region form, region by region with masks."""
    ap, bp, cp = p - v0, p - v1, p - v2
    e1, e2 = v1 - v0, v2 - v0
    d1, d2, d3, d4, d5, d6 = _dot(ap, e1[None]), _dot(ap, e2[None]), _dot(bp, e1[None]), _dot(bp, e2[None]), _dot(cp, e1[None]), _dot(cp, e2[None])
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    q = np.full(p.shape, np.nan)
    todo = np.ones(p.shape[0], dtype=bool)

    def take(mask, value):
        nonlocal todo
        m = todo & mask
        q[m] = value[m]
        todo = todo & ~m
    take((d1 <= 0) & (d2 <= 0), ap)
    take((d3 >= 0) & (d4 <= d3), bp)
    take((vc <= 0) & (d1 >= 0) & (d3 <= 0), ap - (d1 / (d1 - d3))[:, None] * e1[None])
    take((d6 >= 0) & (d5 <= d6), cp)
    take((vb <= 0) & (d2 >= 0) & (d6 <= 0), ap - (d2 / (d2 - d6))[:, None] * e2[None])
    take((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), bp - ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (v2 - v1)[None])
    s = 1.0 / ((va + vb) + vc)
    take(np.ones_like(todo), ap - (e1[None] * (vb * s)[:, None] + e2[None] * (vc * s)[:, None]))
    return q


def field(verts, faces, origin, h, shape):
    """(magnitude f64 [nz, ny, nx], winding f64, dropped, degenerate): a loop over the faces, each over all the nodes."""
    nx, ny, nz = shape
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([origin[0] + ix.reshape(-1) * h, origin[1] + iy.reshape(-1) * h, origin[2] + iz.reshape(-1) * h], axis=1)
    best, S = np.full(p.shape[0], np.inf), np.zeros(p.shape[0])
    dropped = degenerate = 0
    with np.errstate(all="ignore"):
        for f in np.asarray(faces):
            v0, v1, v2 = (np.asarray(verts, np.float64)[k] for k in f)
            if not (np.isfinite(v0).all() and np.isfinite(v1).all() and np.isfinite(v2).all()):
                dropped += 1
                continue
            n = np.cross(v1 - v0, v2 - v0)
            nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            if not (np.isfinite(nn) and nn > 0):
                degenerate += 1
                continue
            q = _closest_vector(p, v0, v1, v2)
            d2 = _dot(q, q)
            better = d2 < best
            best[better] = d2[better]
            a, b, c = v0 - p, v1 - p, v2 - p
            la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
            det = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2])) \
                + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])
            den = (((la * lb) * lc + _dot(a, b) * lc) + _dot(b, c) * la) + _dot(c, a) * lb
            S += 2.0 * np.arctan2(det, den)
    return np.sqrt(best).reshape(nz, ny, nx), (S / (4.0 * np.pi)).reshape(nz, ny, nx), dropped, degenerate


def decided(winding, near):
    """Nodes whose reference winding number is farther than `near` from 0.5: where the sign is compared."""
    return np.abs(winding - 0.5) > near


def trilinear(phi, f):
    """(value, d/df [3]) of the trilinear interpolant of the 2 x 2 x 2 block phi[z][y][x] (float64) at fractions f = (fx, fy, fz)."""
    fx, fy, fz = f
    value, grad = 0.0, np.zeros(3)
    for z in (0, 1):
        for y in (0, 1):
            for x in (0, 1):
                wx, wy, wz = (fx if x else 1.0 - fx), (fy if y else 1.0 - fy), (fz if z else 1.0 - fz)
                c = float(phi[z, y, x])
                value += c * wx * wy * wz
                grad += c * np.array([(1.0 if x else -1.0) * wy * wz, wx * (1.0 if y else -1.0) * wz, wx * wy * (1.0 if z else -1.0)])
    return value, grad


def sample(points, sdf, margin):
    """(pen f64 [E], g f64 [E, 3], d f64 [E], in_range [E]), a loop over the points.  The cell is the float32 statement's (t formed and
    floored in float32: a decision, like the selection of tests/magnet_reference.py); everything behind it is float64."""
    pts = np.asarray(points, np.float32)
    E = pts.shape[0]
    nx, ny, nz = sdf.shape
    pen, g, d, ok = np.zeros(E), np.zeros((E, 3)), np.full(E, np.inf), np.zeros(E, dtype=bool)
    o32, k32 = sdf.origin32, sdf.inv_h32
    top = (nx - 1, ny - 1, nz - 1)
    phi = sdf.phi.astype(np.float64)
    with np.errstate(all="ignore"):
        for e in range(E):
            t32 = (pts[e] - o32) * k32
            if not all(np.isfinite(t32[k]) and 0 <= t32[k] < top[k] for k in range(3)):
                continue
            ok[e] = True
            i = np.floor(t32).astype(np.int64)
            t64 = (pts[e].astype(np.float64) - o32.astype(np.float64)) * np.float64(k32)
            value, grad = trilinear(phi[i[2]:i[2] + 2, i[1]:i[1] + 2, i[0]:i[0] + 2], t64 - i)
            d[e] = value
            r = float(np.float32(margin)) - value
            if r > 0:
                pen[e] = r * r
                g[e] = (-2.0 * r) * grad * np.float64(k32)
    return pen, g, d, ok


def penalty(points, sdf, margin, upstream=1.0):
    """(L, dL/dpoints) in float64."""
    pen, g, _, _ = sample(points, sdf, margin)
    E = pen.shape[0]
    if E == 0:
        return 0.0, g
    return float(pen.sum() / E), g * (float(np.float32(upstream)) / E)


def error_bounds(sdf):
    """(e_d, e_grad): what the float32 statement may be off by in d and in a component of grad d, from its own roundings (u = 2^-24).
    t = (p - o)*k takes two roundings of at most u*n each (n: the longest axis' nodes), so a fraction f is off by 2 u n; d moves by at
    most D (the largest difference of two neighbouring nodes) per unit of each of its three fractions, and its seven lerps take
    fourteen roundings of at most u*M (M = max |phi|).  A gradient component is a lerp of corner differences (each <= D, one rounding)
    over two fractions, its second differences <= 2 D, then times k: two fractions, six lerp roundings, four differences, one product."""
    u = 2.0 ** -24
    phi = sdf.phi.astype(np.float64)
    n, M, k = max(sdf.shape), float(np.abs(phi).max()), float(sdf.inv_h32)
    D = max(float(np.abs(np.diff(phi, axis=a)).max()) if phi.shape[a] > 1 else 0.0 for a in range(3))
    f_err = 2.0 * u * n
    return 3.0 * f_err * D + 14.0 * u * M, (2.0 * f_err * 2.0 * D + 11.0 * u * D) * k


def central_difference(point, sdf, margin, step):
    """d pen / d point [3] of one point by central differences of the float64 restatement: `step` must keep all six probes in the
    point's cell and on its side of r = 0."""
    out = np.zeros(3)
    for k in range(3):
        hi, lo = np.array(point, np.float64), np.array(point, np.float64)
        hi[k] += step
        lo[k] -= step
        out[k] = (_pen64(hi, sdf, margin) - _pen64(lo, sdf, margin)) / (2.0 * step)
    return out


def _pen64(p, sdf, margin):
    """pen of a float64 point, everything in float64 (origin and 1/h as the statement rounds them)."""
    t = (p - sdf.origin32.astype(np.float64)) * np.float64(sdf.inv_h32)
    i = np.floor(t).astype(np.int64)
    value, _ = trilinear(sdf.phi.astype(np.float64)[i[2]:i[2] + 2, i[1]:i[1] + 2, i[0]:i[0] + 2], t - i)
    r = float(np.float32(margin)) - value
    return r * r if r > 0 else 0.0


def ratios(value, grad, points, sdf, margin, upstream=1.0):
    """(value ratio, gradient ratio) of a candidate (L, dL/dpoints) against float64, with the numpy float32 path's own error as the
    allowance (tests/param_reference.py class_ratios)."""
    from utils import head_sdf as H
    v64, g64 = penalty(points, sdf, margin, upstream)
    v32, g32 = H.penalty(points, sdf, margin, upstream)
    one = np.array(["*"])
    rv = R.worst(R.class_ratios(np.array([[value]]), np.array([[v64]]), np.array([[v32]]), one))
    E = g64.shape[0]
    if E == 0:
        return rv, 0.0
    rg = R.worst(R.class_ratios(np.asarray(grad).reshape(E, 3), g64, g32, np.array(["*"] * E)))
    return rv, rg


def accepts(value, grad, points, sdf, margin, upstream=1.0):
    rv, rg = ratios(value, grad, points, sdf, margin, upstream)
    return rv <= K and rg <= K
