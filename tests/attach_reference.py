"""The root attachment restated as plain loops, strand by strand and step by step, from the docstring of scene/strand_attach.py; it
shares no code with the numpy path.  Float64 values are Python floats (IEEE doubles: +, -, *, / and math.sqrt round once); float32
values are numpy float32 scalars.  The head's field is sampled by tests/collide_reference.sample, the restatement of S(x)."""
import math

import numpy as np

from tests.collide_reference import sample, same_bytes  # noqa: F401  (same_bytes: for the tests)

F = np.float32
REACHED, NEAR, DEGENERATE, RANGE, FLAT, STEPS, UNLANDED, FAR, OFF_SCALP = range(9)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else math.nan           # (a NaN fails the comparison; dot(u, u) is never negative)


def _div(a, b):
    """IEEE a / b for doubles (Python raises where the hardware gives an infinity or a NaN)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _positive(v):
    return math.isfinite(v) and v > 0.0


def _S(x, sdf):
    ok, d, g = sample(x, sdf)
    if not ok:
        return False, None, None
    return True, d, [float(v) for v in g]


def steer(field, x, p, min_conf):
    """The volume's direction at x, sign-aligned to p, or None: the corner loop of utils/trace.py's Trace statement."""
    nx, ny, nz = field.shape
    k = 1.0 / field.spacing
    t = [(x[c] - float(field.origin[c])) * k for c in range(3)]
    for c, n in enumerate((nx, ny, nz)):
        if not (math.isfinite(t[c]) and 0.0 <= t[c] < float(n - 1)):
            return None
    fl = [math.floor(v) for v in t]
    f = [t[c] - fl[c] for c in range(3)]
    g = [1.0 - f[c] for c in range(3)]
    w, v = 0.0, [0.0, 0.0, 0.0]
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                node = (int(fl[2]) + cz, int(fl[1]) + cy, int(fl[0]) + cx)
                tw = ((f[0] if cx else g[0]) * (f[1] if cy else g[1])) * (f[2] if cz else g[2])
                a = tw * float(field.conf[node])
                w = w + a
                e = [float(field.dir[node + (j,)]) for j in range(3)]
                if _dot(e, p) < 0.0:
                    a = -a
                v = [v[j] + a * e[j] for j in range(3)]
    nn = _dot(v, v)
    if not (w >= min_conf and _positive(nn)):
        return None
    ln = math.sqrt(nn)
    return [v[j] / ln for j in range(3)]


def march(points, offsets, sdf, field=None, margin=0.0, tol=None, step=None, max_steps=256, land_iters=4, pull=1.0, descent=0.25,
          max_distance=None, min_conf=0.5):
    """(ext float64 [K, max_steps + 1, 3] (zero from count on), count int32 [K], reason int32 [K], landed float32 [K])."""
    margin = F(margin)
    tol = F(1e-3 * sdf.spacing) if tol is None else F(tol)
    step = 0.5 * sdf.spacing if step is None else float(step)
    max_distance = math.inf if max_distance is None else float(max_distance)
    m, tl = float(margin), float(tol)
    K = len(offsets) - 1
    ext = np.zeros((K, max_steps + 1, 3), np.float64)
    count, reason, landed = np.zeros(K, np.int32), np.full(K, DEGENERATE, np.int32), np.full(K, np.inf, np.float32)
    for s in range(K):
        a, n = int(offsets[s]), int(offsets[s + 1] - offsets[s])
        if n < 2:
            continue
        x = [float(points[a, c]) for c in range(3)]
        ok, d, G = _S(x, sdf)
        if not ok:
            reason[s] = RANGE
            continue
        if float(d) <= m + tl:
            reason[s], landed[s] = NEAR, d
            continue
        if float(d) - m > max_distance:
            reason[s] = FAR
            continue
        e = [x[c] - float(points[a + 1, c]) for c in range(3)]
        le = _sqrt(_dot(e, e))
        if _positive(le):
            p = [e[c] / le for c in range(3)]
        else:
            g0 = _sqrt(_dot(G, G))
            p = [_div(-G[c], g0) for c in range(3)]
        why = STEPS
        for _ in range(max_steps):
            gn = _sqrt(_dot(G, G))
            if not _positive(gn):
                why = FLAT
                break
            if float(d) - m <= step:
                why = UNLANDED
                for _ in range(land_iters):
                    c_ = (m - float(d)) / gn
                    x = [x[c] + (c_ * G[c]) / gn for c in range(3)]
                    ok, d, G = _S(x, sdf)
                    if not ok:
                        why = RANGE
                        break
                    if abs(float(d) - m) <= tl:
                        ext[s, count[s]] = x
                        count[s] += 1
                        landed[s] = d
                        why = REACHED
                        break
                    gn = _sqrt(_dot(G, G))
                    if not _positive(gn):
                        why = FLAT
                        break
                break
            nrm = [-G[c] / gn for c in range(3)]
            f = p
            if field is not None:
                fv = steer(field, x, p, min_conf)
                if fv is not None:
                    f = fv
            v = [f[c] + pull * nrm[c] for c in range(3)]
            vn = _sqrt(_dot(v, v))
            dd = [v[c] / vn for c in range(3)] if _positive(vn) else nrm
            if _dot(dd, nrm) < descent:
                dd = nrm
            x = [x[c] + step * dd[c] for c in range(3)]
            p = dd
            ext[s, count[s]] = x
            count[s] += 1
            ok, d, G = _S(x, sdf)
            if not ok:
                why = RANGE
                break
        reason[s] = why
    return ext, count, reason, landed


def rejoin(points, attrs, offsets, ext, count, reason, M):
    """(out_points float32 [N, 3], out_attrs float32 [N, C], out_offsets int64 [K + 1])."""
    K, C = len(offsets) - 1, attrs.shape[1]
    pts, att, sizes = [], [], []
    for s in range(K):
        a, n = int(offsets[s]), int(offsets[s + 1] - offsets[s])
        own_p, own_a = points[a:a + n], attrs[a:a + n]
        cnt = int(count[s])
        if not (reason[s] == REACHED and cnt >= 1 and n >= 1):
            pts.append(own_p), att.append(own_a), sizes.append(n)
            continue
        with np.errstate(all="ignore"):
            new = ext[s, :cnt][::-1].astype(np.float32)
        V = np.concatenate([new, own_p])
        A = np.concatenate([np.repeat(own_a[:1], cnt, axis=0), own_a])
        if M == 0:
            pts.append(V), att.append(A), sizes.append(cnt + n)
            continue
        m = V.shape[0]
        v = [[float(V[i, c]) for c in range(3)] for i in range(m)]
        ln, cum = [], [0.0]
        for i in range(m - 1):
            e = [v[i + 1][c] - v[i][c] for c in range(3)]
            ln.append(_sqrt(_dot(e, e)))
            cum.append(cum[-1] + ln[-1])
        L = cum[-1]
        op, oa = np.empty((M, 3), np.float32), np.empty((M, C), np.float32)
        op[0], op[M - 1], oa[0], oa[M - 1] = V[0], V[m - 1], A[0], A[m - 1]
        for j in range(1, M - 1):
            t = (j / (M - 1)) * L
            i = 0
            for k in range(m - 1):                                             # the largest index <= m - 2 with cum_i <= t, 0 if none
                if cum[k] <= t:
                    i = k
            w = (t - cum[i]) / ln[i] if ln[i] > 0.0 else 0.0
            with np.errstate(all="ignore"):
                op[j] = [F(v[i][c] + w * (v[i + 1][c] - v[i][c])) for c in range(3)]
                oa[j] = [F(float(A[i, c]) + w * (float(A[i + 1, c]) - float(A[i, c]))) for c in range(C)]
        pts.append(op), att.append(oa), sizes.append(M)
    out = np.concatenate(pts + [np.zeros((0, 3), np.float32)]).astype(np.float32)
    oat = np.concatenate(att + [np.zeros((0, C), np.float32)]).astype(np.float32)
    return out, oat, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
