"""The head push-out restated as a plain loop, strand by strand and joint by joint, from the docstring of scene/strand_collide.py; it
shares no code with the numpy path.  Float64 values are Python floats (IEEE doubles: +, -, *, / and math.sqrt round once); float32
values are numpy float32 scalars, whose operations round once to float32."""
import math

import numpy as np

F = np.float32


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan           # (a NaN fails the comparison; dot(u, u) is never negative)


def _lerp(u, v, f):
    return u + f * (v - u)


def sample(x, sdf):
    """S(x): (ok, d, (gx, gy, gz)) with d and g float32 scalars; (False, None, None) for a point not finite or out of range."""
    nx, ny, nz = sdf.shape
    o, k, phi = sdf.origin32, sdf.inv_h32, sdf.phi
    with np.errstate(all="ignore"):
        p = [F(x[0]), F(x[1]), F(x[2])]
        t = [(p[c] - o[c]) * k for c in range(3)]
        for c, n in enumerate((nx, ny, nz)):
            if not (np.isfinite(t[c]) and t[c] >= F(0) and t[c] < F(n - 1)):
                return False, None, None
        fl = [np.floor(v) for v in t]
        ix, iy, iz = (int(v) for v in fl)
        fx, fy, fz = (t[c] - fl[c] for c in range(3))
        c = {(a, b, e): phi[iz + e, iy + b, ix + a] for a in (0, 1) for b in (0, 1) for e in (0, 1)}      # c[x, y, z]
        c00, c10 = _lerp(c[0, 0, 0], c[1, 0, 0], fx), _lerp(c[0, 1, 0], c[1, 1, 0], fx)
        c01, c11 = _lerp(c[0, 0, 1], c[1, 0, 1], fx), _lerp(c[0, 1, 1], c[1, 1, 1], fx)
        c0, c1 = _lerp(c00, c10, fy), _lerp(c01, c11, fy)
        d = _lerp(c0, c1, fz)
        gx = _lerp(_lerp(c[1, 0, 0] - c[0, 0, 0], c[1, 1, 0] - c[0, 1, 0], fy), _lerp(c[1, 0, 1] - c[0, 0, 1], c[1, 1, 1] - c[0, 1, 1], fy), fz) * k
        gy = _lerp(_lerp(c[0, 1, 0] - c[0, 0, 0], c[1, 1, 0] - c[1, 0, 0], fx), _lerp(c[0, 1, 1] - c[0, 0, 1], c[1, 1, 1] - c[1, 0, 1], fx), fz) * k
        gz = _lerp(_lerp(c[0, 0, 1] - c[0, 0, 0], c[1, 0, 1] - c[1, 0, 0], fx), _lerp(c[0, 1, 1] - c[0, 1, 0], c[1, 1, 1] - c[1, 1, 0], fx), fy) * k
    assert all(type(v) is F for v in (d, gx, gy, gz))
    return True, d, (gx, gy, gz)


def resolve(points, offsets, sdf, margin, skin, iters):
    """(out float32 [P, 3], moved int32 [K], unresolved int32 [K], first_hit int64 [K]): first_hit is the joint of a strand's first
    push, or its number of joints."""
    margin = F(margin)
    skin = F(1e-3 * sdf.spacing) if skin is None else F(skin)
    K = len(offsets) - 1
    out = np.array(points, dtype=np.float32, copy=True)
    moved_count, unresolved, first_hit = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int64)
    for s in range(K):
        a, n = int(offsets[s]), int(offsets[s + 1] - offsets[s])
        first_hit[s] = n
        if n < 2:
            continue
        q = [float(points[a, c]) for c in range(3)]
        moved = False
        for j in range(1, n):
            pj = [float(points[a + j, c]) for c in range(3)]
            pp = [float(points[a + j - 1, c]) for c in range(3)]
            e = [pj[c] - pp[c] for c in range(3)]
            L = _sqrt(_dot(e, e))

            def relen(x):
                u = [x[c] - q[c] for c in range(3)]
                lu = _sqrt(_dot(u, u))
                if math.isfinite(L) and math.isfinite(lu) and lu > 0.0:
                    f = L / lu
                    return [q[c] + f * u[c] for c in range(3)]
                return [q[c] + e[c] for c in range(3)]

            x = pj
            if moved:
                x = relen(x)
            hit = False
            for _ in range(iters):
                ok, d, g = sample(x, sdf)
                if not (ok and d < margin):
                    break
                G = [float(v) for v in g]
                gn = _sqrt(_dot(G, G))
                if not (math.isfinite(gn) and gn > 0.0):
                    break
                step = ((float(margin) + float(skin)) - float(d)) / gn
                x = [x[c] + step * G[c] for c in range(3)]
                hit = True
                x = relen(x)
            if hit:
                if not moved:
                    first_hit[s] = j
                moved = True
                moved_count[s] += 1
            q = x
            with np.errstate(all="ignore"):
                out[a + j] = [F(v) for v in q]
            ok, d, _ = sample(q, sdf)
            if ok and d < margin:
                unresolved[s] += 1
    return out, moved_count, unresolved, first_hit
